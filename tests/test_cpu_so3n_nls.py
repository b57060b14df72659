"""Chordal rotation averaging as a nonlinear least-squares problem, without a GPU: the longdouble restatement of F, dF, dF*
(tests/so3n_nls_reference.py) against itself (adjoint identity, central difference of F o retract, the diagonal blocks of
dF* dF) and against the fp64 oracle of the same problem (1/2 |F|^2 = f, dF* F = grad f), and mode (h) of
tests/cpp/harness_tnls_so3n.cpp -- this repository's TNLS.h on a host vector with a plain-C++ restatement of the problem --
against the committed fixture tests/golden/tnls_so3n.json."""
import json
import os
import sys

import numpy as np
import pytest

import so3n_nls_reference as nr
from so3_cases import LD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_tnls_so3n as mg  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "tnls_so3n.json")


@pytest.fixture(scope="module")
def fixture_file():
    return json.load(open(GOLDEN))


@pytest.mark.parametrize("name", nr.GRAPH_NAMES)
def test_adjoint_identity(name):
    """<dF xi, Y> = <xi, dF* Y> to 1e-14 relative"""
    g = nr.graph(name)
    ref = nr.NlsRef(g)
    xi, Y, _, _ = nr.probes(name)
    a = (ref.dF(xi) * Y.astype(LD)).sum()
    b = (xi.astype(LD) * ref.dFt(Y)).sum()
    assert abs(a - b) <= 1e-14 * max(abs(a), abs(b)), (name, float(a), float(b))


@pytest.mark.parametrize("name", nr.GRAPH_NAMES)
def test_jacobian_is_the_derivative_of_the_residual_along_the_retraction(name):
    """dF xi against the central difference (F(retract(R, h xi)) - F(retract(R, -h xi))) / 2h, h = 1e-6: 1e-8 relative,
    the O(h^2) bound with room"""
    g = nr.graph(name)
    ref = nr.NlsRef(g)
    xi = nr.probes(name)[0].astype(LD)
    h = LD(1e-6)
    fd = (ref.F(ref.retract(h * xi)) - ref.F(ref.retract(-h * xi))) / (2 * h)
    assert nr.rel_inf(fd, ref.dF(xi)) <= 1e-8


@pytest.mark.parametrize("name", nr.GRAPH_NAMES)
def test_half_squared_residual_and_adjoint_are_objective_and_gradient(oracle, name):
    """1/2 |F(R)|^2 = f(R) and dF* F(R) = grad f(R) of the oracle's SO(3)^N problem, to 1e-13"""
    g = nr.graph(name)
    ref = nr.NlsRef(g)
    F = ref.F()
    pr = oracle.so3n(g.N, g.ei, g.ej, g.Rt, g.w)
    try:
        f, grad = oracle.eval_f(pr, g.R.ravel()), oracle.eval_grad(pr, g.R.ravel())
    finally:
        oracle.free(pr)
    half = (F * F).sum() / 2
    assert abs(half - LD(f)) <= 1e-13 * abs(half)
    gl = ref.dFt(F)
    assert np.sqrt(((gl - grad.astype(LD)) ** 2).sum()) <= 1e-13 * np.sqrt((gl * gl).sum())


@pytest.mark.parametrize("name", nr.GRAPH_NAMES)
def test_diagonal_blocks_of_the_normal_operator(name):
    """the 3 x 3 diagonal blocks of dF* dF are 2 degw_i I (|R hat(xi) S|^2 = 2 |xi|^2 for rotations R, S): what
    mi_so3n_gn_scaling rests on.  Not so for measurements that are not rotations: there the block is 2 degw_i I only up
    to the scaling of the measurement, which the test states too."""
    g = nr.graph(name)
    ref = nr.NlsRef(g)
    dw = nr.degw(g)
    deg = np.bincount(np.concatenate([g.ei, g.ej]), minlength=g.N)
    nodes = sorted({0, 1, g.N - 1, int(np.argmax(deg)), int(np.argmin(deg)), g.N // 2})
    tol = 1e-14 if not name.startswith("nonrot") else 0.03    # (1.01^2 - 1 on the first-node incidences)
    for i in nodes:
        for a in range(3):
            e = np.zeros(3 * g.N)
            e[3 * i + a] = 1
            col = ref.dFt(ref.dF(e))[3 * i:3 * i + 3]
            want = np.zeros(3, dtype=LD)
            want[a] = 2 * dw[i]
            assert np.max(np.abs(col - want)) <= tol * 2 * dw[i], (name, i, a)


def test_fixture_meets_its_conditions(fixture_file):
    assert sorted(fixture_file) == sorted(c[0] for c in mg.CASES)
    for key, rec in fixture_file.items():
        mg.check_conditions(key, rec)
        assert len(rec["x"]) == 9 * rec["N"]
    rej = fixture_file[mg.REJECTED_CASE]
    k = rej["accepted"].index(False)
    assert rej["rho"][k] < 0 and rej["outer"] > k + 1       # (a clear rejection, and solves after it)


@pytest.mark.parametrize("key", [c[0] for c in mg.CASES])
def test_host_mode_reproduces_the_fixture(fixture_file, key):
    """mode (h) -- TNLS.h on a host vector, the plain-C++ problem -- gives the committed record exactly"""
    from harness_tnls_so3n_py import HOST, TnlsSo3nHarness
    from optimization_amd import workloads as wl
    rec = fixture_file[key]
    ei, ej, Rt, w = wl.pose_graph(rec["N"], seed=rec["graph_seed"])[:4]
    R0 = mg.start_point(rec["N"], rec["graph_seed"], rec["start_seed"])
    r = TnlsSo3nHarness().tnls(rec["N"], ei, ej, Rt, w, R0, rec["params"], HOST, rec["with_precon"])
    assert r["rc"] == 0, r["err"]
    assert (r["status"], r["outer"], r["inner_iterations"], r["accepted"]) == \
        (rec["status"], rec["outer"], rec["inner_iterations"], rec["accepted"])
    assert np.array_equal(r["x"], np.asarray(rec["x"])) and r["f"] == rec["f"] and r["gradfx_norm"] == rec["gradfx_norm"]
    assert np.array_equal(r["rho"], np.asarray(rec["rho"]))
    assert np.array_equal(r["trust_region_radius"], np.asarray(rec["trust_region_radius"]))
