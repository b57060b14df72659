"""The spectral initialisation of SO(3)^N without a GPU: the numpy restatement against the facts it is used for, the
compiled forms of the new kernels, the rounding code on the host, the harness and the capi surface."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import so3n_spectral_reference as sr
from test_cpu_kernel_resources import HIPCC, _resource_usage
from test_cpu_so3n_certificate import CERT_FIGURES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mi_so3n_laplacian", "mi_so3n_lap_jacobi", "mi_so3n_round", "mi_so3n_project")
NEW_KERNELS = ("k_so3_lap_diag", "k_so3_lap_jacobi", "k_so3_round_init", "k_so3_round_sign", "k_so3_round<true>",
               "k_so3_round<false>")
REFLECTED = {2, 3, 4}     # seeds of RING_CASES whose eigenvector basis lands in the reflected gauge


@pytest.mark.parametrize("case", sr.RING_CASES + sr.WINDING_CASES, ids=str)
def test_reference_spectral_point_and_lower_bound(case):
    N, ei, ej, Rt, w, Rgt = sr.problem(case)
    s = sr.spectral(N, ei, ej, Rt, w)
    f_truth = sr.objective(ei, ej, Rt, w, Rgt)
    sum_w = float(np.sum(w))
    print(case, "f(R0)", s["f"], "f(truth)", f_truth, "lower bound", s["lower_bound"], "negative", s["negative"],
          "gap", s["lam"][3] - s["lam"][2])
    assert np.abs(s["L"] - s["L"].T).max() == 0.0
    noise_free = isinstance(case, int) or case[2] == 0.0
    if noise_free:
        assert s["f"] <= 1e-20 * sum_w
        assert abs(s["lower_bound"]) <= 1e-12 * sum_w * N          # three eigenvalues at 0 to rounding
    else:
        assert s["f"] <= f_truth
        assert s["lower_bound"] <= s["f"]
    if isinstance(case, int):
        assert f_truth > 1.0                                        # the winding is far from the optimum
    else:
        # both branches of the sign rule: all or all but one det < 0, or none or one
        if case[3] in REFLECTED:
            assert s["negative"] >= N - 1 and s["flipped"]
        else:
            assert s["negative"] <= 1 and not s["flipped"]
    R = s["R"].reshape(N, 3, 3)
    assert np.abs(np.swapaxes(R, 1, 2) @ R - np.eye(3)).max() <= 1e-14 and np.abs(np.linalg.det(R) - 1).max() <= 1e-14


def test_sign_rule_of_the_reference_on_a_tie_and_under_negation():
    M, _ = sr.synthetic_blocks(65)
    V = np.swapaxes(M, 1, 2).reshape(-1, 3)
    a, b = sr.round_panel(V), sr.round_panel(-V)
    assert a["flipped"] != b["flipped"] or a["sign_sum"] == 0
    live = ~a["degenerate"] & (np.nan_to_num(a["sep"]) >= 0.05)
    assert np.abs(a["R"][live] - b["R"][live]).max() <= 1e-13
    tie = np.stack([np.eye(3), np.diag([1.0, 1.0, -1.0])])
    assert not sr.round_panel(np.swapaxes(tie, 1, 2).reshape(-1, 3))["flipped"]


def test_rounding_code_on_the_host_against_svd_rounding(tmp_path):
    """csrc/so3_round.h is straight-line C++ that a host compiler takes: the device's arithmetic, here against numpy's SVD
    rounding on the synthetic blocks of the GPU test at the GPU test's bar, 1e-12 sigma_1 / (sigma_2 + d sigma_3)"""
    src = tmp_path / "round_host.cpp"
    src.write_text('#include "so3_round.h"\nextern "C" void round_many(long n, const double *M, double *R, double *sep, '
                   'double *d, int *deg) {\n  for (long i = 0; i < n; ++i) {\n    bool g;\n    '
                   'mi::so3_nearest_rotation(M + 9 * i, R + 9 * i, sep[i], d[i], g);\n    deg[i] = g;\n  }\n}\n')
    so = tmp_path / "libround_host.so"
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I",
                        os.path.join(ROOT, "optimization_amd", "csrc"), str(src), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    L = C.CDLL(str(so))
    dp = C.POINTER(C.c_double)
    for N in (7, 65, 257, 4099):
        M, kinds = sr.synthetic_blocks(N)
        M[N - 1, 1, 1] = np.inf if N == 65 else M[N - 1, 1, 1]
        ref = sr.round_blocks(M)
        Mf = np.ascontiguousarray(M.reshape(N, 9))
        R, sep, d, deg = np.zeros((N, 9)), np.zeros(N), np.zeros(N), np.zeros(N, dtype=np.int32)
        L.round_many(C.c_long(N), Mf.ctypes.data_as(dp), R.ctypes.data_as(dp), sep.ctypes.data_as(dp), d.ctypes.data_as(dp),
                     deg.ctypes.data_as(C.POINTER(C.c_int)))
        R = R.reshape(N, 3, 3)
        assert np.array_equal(deg.astype(bool), ref["degenerate"])
        assert np.array_equal(R[ref["degenerate"]], np.broadcast_to(np.eye(3), (int(ref["degenerate"].sum()), 3, 3)))
        live = ~ref["degenerate"]
        err = np.linalg.norm((R - ref["R"]).reshape(N, 9), axis=1)[live]
        with np.errstate(divide="ignore"):
            bar = 1e-12 / np.maximum(ref["sep"][live], 0.0)
        print(N, "worst error / bar", float((err / bar).max()))
        assert np.all(err <= bar)
        assert np.abs(np.swapaxes(R, 1, 2) @ R - np.eye(3)).max() <= 1e-14 and np.abs(np.linalg.det(R) - 1).max() <= 1e-14
        general = live & (kinds != 2)
        assert np.abs(sep[general] - ref["sep"][general]).max() <= 1e-13 and np.array_equal(d[general], ref["d"][general])


def test_new_kernels_compile_without_scratch_and_leave_the_certificate_figures():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    r = _resource_usage("so3.hip")
    for name in NEW_KERNELS:
        assert name in r, (name, sorted(k for k in r if "round" in k or "lap" in k))
        print(name, r[name])
        assert r[name][3] == 0, name + " spills"
    for name, figures in CERT_FIGURES.items():
        assert r[name] == figures, (name, r[name], figures)


def test_spectral_harness_compiles_and_links():
    """tests/cpp/harness_spectral_so3n.cpp through clang's front end and g++, linked against the library"""
    from optimization_amd import build
    out = build.build_harness()
    so = os.path.join(ROOT, "tests", "cpp", "libharness_spectral_so3n.so")
    assert so in out and os.path.exists(so)
    L = C.CDLL(so)
    assert L.hs_spectral_so3n and L.hs_last_error
    assert os.path.join(ROOT, "examples", "bin", "spectral_rotation_averaging") in out


def test_capi_mirrors_the_spectral_abi():
    from optimization_amd import capi
    for name in ("laplacian", "lap_jacobi", "round", "project"):
        assert callable(getattr(capi.So3N, name))
    L = capi.load()
    text = open(os.path.join(ROOT, "include", "mi355opt.h")).read()
    for name in SYMBOLS:
        assert getattr(L, name).argtypes is not None
        assert "MI_API int " + name + "(" in text


def test_spectral_entry_points_have_no_cpu_fallback():
    """Without a device they answer MI_ERR_NO_DEVICE, as the other SO(3)^N entry points do"""
    from optimization_amd import capi
    L = capi.load()
    if capi.device_count() > 0:
        pytest.skip("a GPU is present")
    assert L.mi_so3n_laplacian(None, None) == 4
    assert b"no HIP device" in L.mi_last_error()
    assert L.mi_so3n_lap_jacobi(None, 1, None, None) == 4
    assert L.mi_so3n_round(None, None, None, None) == 4
    assert L.mi_so3n_project(None, None, None, None) == 4
