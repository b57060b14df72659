"""Chordal rotation averaging as a nonlinear least-squares problem on the device (optimization_amd/csrc/so3.hip:
k_so3_residual, k_so3_jac, k_so3_jact; mi_so3n_residual / mi_so3n_jacobian / mi_so3n_gn_scaling; the accessors of
MI355::RotationAveraging for Riemannian::TNLS).

(a) single applications of F, dF, dF* and of the two fused LSQR forms (apply_sub_scaled, driven directly as mi_lsqr drives
    them) against the longdouble restatement of tests/so3n_nls_reference.py: 1e-12 relative to the infinity norm of the exact
    result, the project's bar for a vector after one fused pass; the worst case per graph is printed;
(b) on the graphs of so3n_nls_reference.GRAPH_NAMES: the fixtures' pose graphs, padding lanes in the last slice, a second
    1024-node window, a hub of degree 70 with leaves of degree 1 and E no multiple of 256, measurements that are not
    rotations (matrix forms), points with and without valid quaternion records;
(c) whole TNLS runs: the tagged accessors (every inner solve in mi_lsqr) and the same operators behind plain lambdas (the
    generic loop) against mode (h) live and against tests/golden/tnls_so3n.json: status, outer count, every LSQR count and
    the accept sequence exactly, x to 1e-10;
(d) the rejected step of the fixture's designated case: a further LSQR solve with the operators of the old linearisation
    after F was evaluated at the rejected trial point."""
import json
import os
import sys

import numpy as np
import pytest

import so3n_nls_reference as nr
from so3_cases import LD

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_tnls_so3n as mg  # noqa: E402

TOL = 1e-12
ALPHA, BETA = 0.7310585786300049, 1.6487212707001282     # the scales of the fused forms (any numbers of order 1)


@pytest.fixture(scope="module")
def ctx():
    from optimization_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fixture_file():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "tnls_so3n.json")))


def _problem(ctx, g):
    from optimization_amd import capi
    return capi.So3N(ctx, g.N, g.ei, g.ej, g.Rt, g.w)


def _check_all(ctx, prob, name, R_dev, ref, expect_quat, worst):
    """every operator of the least-squares view at the point R_dev (whose exact values `ref` holds) against longdouble"""
    xi, Y, u0, v0 = nr.probes(name)
    F, sq = prob.residual(R_dev, sqnorm=True)
    Fx = ref.F()
    worst["F"] = nr.rel_inf(F.numpy(), Fx)
    worst["|F|^2"] = float(abs(LD(sq) - (Fx * Fx).sum()) / (Fx * Fx).sum())
    dF, dFt = prob.jacobian(R_dev)
    y = dF.apply(ctx.upload(xi)).numpy()
    yx = ref.dF(xi)
    worst["dF"] = nr.rel_inf(y, yx)
    x = dFt.apply(ctx.upload(Y)).numpy()
    xx = ref.dFt(Y)
    worst["dF*"] = nr.rel_inf(x, xx)
    # fused forms: u = dF xi - alpha u0 with |u|^2, v = dF* Y - beta v0 with |v|^2 (IterativeSolvers.h:707,712)
    u = ctx.upload(u0)
    su = dF.apply_sub_scaled(ctx.upload(xi), ALPHA, u)
    ux = yx - LD(ALPHA) * u0.astype(LD)
    worst["dF fused"] = nr.rel_inf(u.numpy(), ux)
    worst["|u|^2"] = float(abs(LD(su) - (ux * ux).sum()) / (ux * ux).sum())
    v = ctx.upload(v0)
    sv = dFt.apply_sub_scaled(ctx.upload(Y), BETA, v)
    vx = xx - LD(BETA) * v0.astype(LD)
    worst["dF* fused"] = nr.rel_inf(v.numpy(), vx)
    worst["|v|^2"] = float(abs(LD(sv) - (vx * vx).sum()) / (vx * vx).sum())
    # ... and against apply followed by the update in double (the separate-kernel route): same bar
    assert nr.rel_inf(u.numpy(), y.astype(LD) - LD(ALPHA) * u0.astype(LD)) <= TOL
    assert nr.rel_inf(v.numpy(), x.astype(LD) - LD(BETA) * v0.astype(LD)) <= TOL
    # the gate: *mode != 0 -> the kernel does nothing
    u2, v2 = ctx.upload(u0), ctx.upload(v0)
    assert dF.apply_sub_scaled(ctx.upload(xi), ALPHA, u2, mode=1) is None and np.array_equal(u2.numpy(), u0)
    assert dFt.apply_sub_scaled(ctx.upload(Y), BETA, v2, mode=1) is None and np.array_equal(v2.numpy(), v0)
    print(name, "quaternion gathers" if expect_quat else "matrix gathers",
          "  ".join(f"{k}={e:.2e}" for k, e in worst.items()))
    for k, e in worst.items():
        assert e <= TOL, (name, k, e)


@pytest.mark.parametrize("name", nr.GRAPH_NAMES)
def test_single_applications_at_a_point_of_the_caller(ctx, name):
    """R as the caller uploads it (no quaternion records: 72-byte rows)"""
    g = nr.graph(name)
    prob = _problem(ctx, g)
    assert prob.info()["sinc_quat"] == (not name.startswith("nonrot"))
    _check_all(ctx, prob, name, ctx.upload(g.R.ravel()), nr.NlsRef(g), False, {})


@pytest.mark.parametrize("name", ("pose_150", "star_chain", "nonrot_1100"))
def test_single_applications_at_a_point_of_a_fused_trial(ctx, name):
    """R+ produced by the retraction of a fused Armijo trial: its quaternion records are valid and are what F gathers
    and what the Jacobian copies"""
    g = nr.graph(name)
    prob = _problem(ctx, g)
    R = ctx.upload(g.R.ravel())
    _, Rp, _ = prob.armijo_trial(R, prob.gradient(R), 0.05)
    _check_all(ctx, prob, name, Rp, nr.NlsRef(g, R=Rp.numpy()), True, {})


def test_bound_operators_survive_evaluations_elsewhere(ctx):
    """the trial-point hazard, directly: linearise at R+ (quaternion records valid), then evaluate F, the objective and a
    further fused trial at OTHER points (all of which rewrite the problem's quaternion buffer), then apply dF and dF*:
    they must still be those of R+"""
    name = "pose_1100"
    g = nr.graph(name)
    prob = _problem(ctx, g)
    R = ctx.upload(g.R.ravel())
    grad = prob.gradient(R)
    _, Rp, _ = prob.armijo_trial(R, grad, 0.05)
    ref = nr.NlsRef(g, R=Rp.numpy())
    xi, Y, _, _ = nr.probes(name)
    dF, dFt = prob.jacobian(Rp)
    y0, x0 = dF.apply(ctx.upload(xi)).numpy(), dFt.apply(ctx.upload(Y)).numpy()
    prob.residual(R)
    prob.objective(R)
    _, Rq, _ = prob.armijo_trial(R, grad, 0.3)
    prob.residual(Rq)
    y1, x1 = dF.apply(ctx.upload(xi)).numpy(), dFt.apply(ctx.upload(Y)).numpy()
    assert np.array_equal(y0, y1) and np.array_equal(x0, x1)
    assert nr.rel_inf(y1, ref.dF(xi)) <= TOL and nr.rel_inf(x1, ref.dFt(Y)) <= TOL


def test_results_are_the_same_bits_on_every_run(ctx):
    name = "star_chain"
    g = nr.graph(name)
    prob = _problem(ctx, g)
    R = ctx.upload(g.R.ravel())
    _, Y, _, v0 = nr.probes(name)
    _, dFt = prob.jacobian(R)
    runs = []
    for _ in range(3):
        v = ctx.upload(v0)
        s = dFt.apply_sub_scaled(ctx.upload(Y), BETA, v)
        runs.append((v.numpy(), s))
    assert all(np.array_equal(runs[0][0], r[0]) and runs[0][1] == r[1] for r in runs[1:])


def test_gn_scaling_and_the_refused_calls(ctx):
    from optimization_amd import capi
    g = nr.graph("star_chain")
    prob = _problem(ctx, g)
    v = nr.probes("star_chain")[3]
    d = np.repeat(1.0 / np.sqrt(2 * nr.degw(g).astype(np.float64)), 3)
    assert nr.rel_inf(prob.gn_scaling().apply(ctx.upload(v)).numpy(), d.astype(LD) * v.astype(LD)) <= 4e-16
    empty = capi.So3N(ctx, 3, np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros((0, 9)), np.zeros(0))
    with pytest.raises(capi.MiError) as e:
        empty.jacobian(ctx.upload(np.tile(np.eye(3).ravel(), 3)))
    assert e.value.status == 1 and "no edges" in str(e.value)       # 1: MI_ERR_INVALID_ARGUMENT
    neg = capi.So3N(ctx, g.N, g.ei, g.ej, g.Rt, -g.w)
    with pytest.raises(capi.MiError):
        neg.residual(ctx.upload(g.R.ravel()))


@pytest.fixture(scope="module")
def runs(fixture_file):
    """every fixture case in modes (h), (d), (g): computed once"""
    from harness_tnls_so3n_py import DEVICE, GENERIC, HOST, TnlsSo3nHarness
    from optimization_amd import workloads as wl
    H = TnlsSo3nHarness()
    out = {}
    for key, rec in fixture_file.items():
        ei, ej, Rt, w = wl.pose_graph(rec["N"], seed=rec["graph_seed"])[:4]
        R0 = mg.start_point(rec["N"], rec["graph_seed"], rec["start_seed"])
        out[key] = {m: H.tnls(rec["N"], ei, ej, Rt, w, R0, rec["params"], m, rec["with_precon"])
                    for m in (HOST, DEVICE, GENERIC)}
    return out


def _same_run(r, rec_or_run, key):
    assert r["rc"] == 0, r["err"]
    assert r["status"] == rec_or_run["status"], key
    assert r["outer"] == rec_or_run["outer"], key
    assert list(r["inner_iterations"]) == list(rec_or_run["inner_iterations"]), key
    assert list(r["accepted"]) == list(rec_or_run["accepted"]), key
    xr = np.asarray(rec_or_run["x"])
    assert np.linalg.norm(r["x"] - xr) <= 1e-10 * np.linalg.norm(xr), key


@pytest.mark.parametrize("key", [c[0] for c in mg.CASES])
def test_tnls_device_runs(fixture_file, runs, key):
    from harness_tnls_so3n_py import DEVICE, GENERIC, HOST
    rec, h, d, g = fixture_file[key], runs[key][HOST], runs[key][DEVICE], runs[key][GENERIC]
    for r in (d, g):
        _same_run(r, h, key)        # against mode (h) live
        _same_run(r, rec, key)      # against the committed fixture
    print(key, "outer", d["outer"], "LSQR", d["inner_iterations"], "counters", d["counters"],
          "|x_d - x_h| / |x_h| = %.2e" % (np.linalg.norm(d["x"] - h["x"]) / np.linalg.norm(h["x"])))
    # (d): every inner solve in mi_lsqr, and no host-synchronising inner product inside one: the outer loop of TNLS.h
    # takes 2 at the start, 3 per outer iteration (|h|, |F(x+)|^2, |dF h + F|^2) and 1 per accepted step (|grad L|)
    cd = d["counters"]
    assert cd["fused_lsqr_solves"] == d["outer"] and cd["generic_lsqr_solves"] == 0
    assert cd["generic_inner_products"] == 2 + 3 * d["outer"] + sum(d["accepted"])
    # (g): the generic loop, same counts
    cg = g["counters"]
    assert cg["fused_lsqr_solves"] == 0 and cg["generic_lsqr_solves"] == g["outer"]


def test_rejected_step_keeps_the_old_linearisation(fixture_file, runs):
    """the designated case: outer iteration k is rejected (F was evaluated at the trial point), iteration k + 1 solves
    again at the same point with the operators handed out before -- device and host agree on it and on what follows"""
    from harness_tnls_so3n_py import DEVICE, HOST
    rec = fixture_file[mg.REJECTED_CASE]
    h, d = runs[mg.REJECTED_CASE][HOST], runs[mg.REJECTED_CASE][DEVICE]
    k = rec["accepted"].index(False)
    assert d["accepted"][k] is False and d["outer"] > k + 1
    assert d["inner_iterations"][k + 1] == h["inner_iterations"][k + 1] == rec["inner_iterations"][k + 1]
    # the gain ratios around the rejection (steps with decreases of order |F|^2: no cancellation) agree far closer than
    # a stale or overwritten linearisation could leave them; so do the radii, which follow the LSQR step norms
    assert np.allclose(d["rho"][:k + 3], h["rho"][:k + 3], rtol=1e-6, atol=0)
    assert np.allclose(d["trust_region_radius"][:k + 3], h["trust_region_radius"][:k + 3], rtol=1e-8, atol=0)
