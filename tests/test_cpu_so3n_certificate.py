"""The SO(3)^N global-optimality certificate without a GPU: the numpy restatement against itself (float64 against
longdouble at the operator bar, the identities, the winding's closed-form spectrum, the lower bound), the compiled forms
of the new kernels, the host harness and the capi surface."""
import ctypes as C
import os

import numpy as np
import pytest

import so3_cases as sc
import so3n_certificate_reference as cr
from test_cpu_kernel_resources import HIPCC, _resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (TotalSGPRs, VGPRs, compiler's waves/SIMD, scratch bytes per lane) of the certificate kernels as first compiled
CERT_FIGURES = {
    "k_so3_cert_diag<false, false>": (52, 116, 4, 0),
    "k_so3_cert_diag<false, true>": (54, 116, 4, 0),
    "k_so3_cert_diag<true, false>": (50, 120, 4, 0),
    "k_so3_cert_diag<true, true>": (52, 120, 4, 0),
    "k_so3_cert_panel<1, false>": (48, 58, 8, 0),
    "k_so3_cert_panel<1, true>": (44, 62, 8, 0),
    "k_so3_cert_panel<4, false>": (68, 90, 5, 0),
    "k_so3_cert_panel<4, true>": (68, 90, 5, 0),
    "k_so3_cert_panel<8, false>": (100, 114, 4, 0),
    "k_so3_cert_panel<8, true>": (100, 114, 4, 0),
}
OPERATOR_CASES = ("tiny_2", "ring_chords_1025_spread", "ring_chords_1024_negative", "hub_first_some_zero", "hub_last_spread",
                  "multigraph_linspace", "nonrot_perturbed", "powerlaw_5000")


def _panel(m, k, seed=0):
    return np.random.Generator(np.random.PCG64(seed + 11)).normal(size=(m, k))


@pytest.mark.parametrize("name", OPERATOR_CASES)
def test_float64_restatement_is_inside_the_operator_bar_of_the_longdouble_one(name):
    """|S X (float64) - S X (longdouble)| <= 1e-12 (sum_inc |w| + |degw_i|) max |X_c| row block by row block -- the bar the
    device is held to (powerlaw_5000: a node of degree ~ 300; the hubs: degree 1499)"""
    c = sc.case(name)
    X = _panel(3 * c.N, 3)
    lo, hi = cr.of_case(c), cr.of_case(c, cr.LD)
    err = np.abs((lo.apply(X).astype(cr.LD) - hi.apply(X)).astype(np.float64))
    bar = hi.row_bar(X)
    worst = float((err / np.maximum(bar, 1e-300)).max())
    print(name, "worst error / bar", worst)
    assert np.all(err <= bar)
    assert abs(float(lo.f() - hi.f())) <= 1e-13 * max(float(hi.f()), 1e-300)


@pytest.mark.parametrize("name", ("ring_chords_1025_spread", "multigraph_negative", "nonrot_scaled", "isolated_1500"))
def test_identities_of_the_certificate_matrix(name):
    """tr(Y'SY) = 0 and |S Y|_F = |skew Q|_F at a point that is no critical point, in longdouble"""
    c = sc.case(name)
    ref = cr.of_case(c, cr.LD)
    Y = ref.Y()
    SY = ref.apply(Y)
    scale = float(2 * ref.abs_degw().sum())                # |tr(Y' Lap Y)| <= 2 sum_i sum_inc |w|
    assert abs(float((Y * SY).sum())) <= 1e-15 * scale
    assert abs(float(np.sqrt((SY * SY).sum()) - ref.stationarity())) <= 1e-15 * scale
    assert float(ref.stationarity()) > 1e-3                # (the identity is not 0 = 0)
    # symmetry of the operator form: X' (S X') == (S X)' X'
    X, X2 = _panel(3 * c.N, 2, 1), _panel(3 * c.N, 2, 2)
    assert np.abs((X.T.astype(cr.LD) @ ref.apply(X2) - (ref.apply(X).T @ X2.astype(cr.LD))).astype(np.float64)).max() \
        <= 1e-15 * scale * c.N


@pytest.mark.parametrize("N", (5, 8, 130))
def test_winding_spectrum_matches_the_closed_form(N):
    n, ei, ej, Rt, w, R = cr.winding(N)
    ref = cr.CertRef(n, ei, ej, Rt, w, R)
    assert abs(ref.f() - cr.winding_f(N)) <= 1e-12 * N
    assert ref.stationarity() <= 1e-13 * N                 # a critical point
    S = ref.dense()
    assert np.abs(S - S.T).max() == 0.0
    X = _panel(3 * N, 2)
    assert np.abs(S @ X - ref.apply(X)).max() <= 1e-13     # dense and operator forms are the same matrix
    ev = np.linalg.eigvalsh(S)
    lam = cr.winding_lambda_min(N)
    assert lam < 0
    assert np.abs(ev[:2] - lam).max() <= 1e-12 and np.abs(ev[2:5]).max() <= 1e-12
    assert ref.f() + 1.5 * N * ev[0] <= 0                  # the lower bound does not certify: every objective is >= 0


def test_lower_bound_holds_against_the_ground_truth_of_a_noise_free_graph():
    """f(truth) = 0 is the minimum; at the truth lambda_min = 0 (three times) and the bound is tight, at other points
    f(R) + 1.5 N min(lambda_min, 0) <= 0"""
    N, ei, ej, Rt, w, Rgt = cr.ring_with_chords(70, 40, 0.0, 1)
    at_truth = cr.CertRef(N, ei, ej, Rt, w, Rgt)
    ev = np.linalg.eigvalsh(at_truth.dense())
    scale = float(2 * at_truth.abs_degw().max())
    assert at_truth.f() <= 1e-25 * N and np.abs(ev[:3]).max() <= 1e-13 * scale and ev[3] > 1e-3
    assert at_truth.f() + 1.5 * N * min(ev[0], 0.0) <= at_truth.f()
    rng = np.random.default_rng(5)
    for step in (1e-3, 0.3, 3.0):
        R = np.stack([Rgt[i].reshape(3, 3) @ cr._exp(step * rng.normal(size=3)) for i in range(N)]).reshape(N, 9)
        ref = cr.CertRef(N, ei, ej, Rt, w, R)
        lam = np.linalg.eigvalsh(ref.dense())[0]
        lb = ref.f() + 1.5 * N * min(lam, 0.0)
        print("step", step, "f", ref.f(), "lambda_min", lam, "lower bound", lb)
        assert lb <= 1e-12 * scale * N and lb <= ref.f()


def test_certificate_kernels_compile_without_scratch_to_the_recorded_figures():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    r = _resource_usage("so3.hip")
    for name, figures in CERT_FIGURES.items():
        assert name in r, (name, sorted(k for k in r if "cert" in k))
        print(name, r[name])
        assert r[name][3] == 0, name + " spills"
        assert r[name] == figures, (name, r[name], figures)


def test_certify_harness_compiles_and_links():
    """tests/cpp/harness_certify_so3n.cpp through clang's front end and g++, linked against the library: every symbol of
    the new C ABI that the template layer uses resolves"""
    from optimization_amd import build
    out = build.build_harness()
    so = os.path.join(ROOT, "tests", "cpp", "libharness_certify_so3n.so")
    assert so in out and os.path.exists(so)
    L = C.CDLL(so)
    assert L.hc_certify_so3n and L.hc_last_error


def test_capi_mirrors_the_certificate_abi():
    from optimization_amd import capi
    assert callable(capi.So3N.certificate)
    for name in ("apply", "apply_blocks", "null_panel"):
        assert callable(getattr(capi.So3NCertificate, name))
    L = capi.load()
    for name in ("mi_so3n_certificate", "mi_so3n_cert_apply", "mi_so3n_cert_apply_blocks", "mi_so3n_cert_null_panel"):
        assert getattr(L, name).argtypes is not None
    text = open(os.path.join(ROOT, "include", "mi355opt.h")).read()
    for name in ("mi_so3n_certificate", "mi_so3n_cert_apply", "mi_so3n_cert_apply_blocks", "mi_so3n_cert_null_panel"):
        assert "MI_API int " + name + "(" in text


def test_certificate_entry_points_have_no_cpu_fallback():
    """Without a device they answer MI_ERR_NO_DEVICE, as the other SO(3)^N entry points do"""
    from optimization_amd import capi
    L = capi.load()
    if capi.device_count() > 0:
        pytest.skip("a GPU is present")
    info = (C.c_double * 3)()
    assert L.mi_so3n_certificate(None, None, None, info) == 4
    assert b"no HIP device" in L.mi_last_error()
    assert L.mi_so3n_cert_apply(None, 1, None, None) == 4
    assert L.mi_so3n_cert_apply_blocks(None, None, None) == 4
    assert L.mi_so3n_cert_null_panel(None, None) == 4
