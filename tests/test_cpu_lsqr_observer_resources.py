"""The two kernels the observed fused LSQR adds (lsqr.hip: k_lsqr_peek, one wave behind k_lsqr_xw of every pass of
mi_lsqr_observed; k_lsqr_user_stop, the observer's stop) use no scratch memory, and adding them leaves every kernel of
mi_lsqr with exactly the registers, occupancy and scratch it had before: the un-observed solve launches the code it always
launched.  Read from the compiler's resource-usage remarks (no GPU needed)."""
import inspect
import os

import numpy as np
import pytest

from test_cpu_kernel_resources import HIPCC, _resource_usage

# (TotalSGPRs, VGPRs, waves/SIMD, scratch bytes per lane) as the commit before the observed solve compiled them
LSQR_KERNELS_BEFORE = {
    "k_lsqr_init_u": (24, 19, 8, 0),
    "k_lsqr_init_v": (26, 19, 8, 0),
    "k_lsqr_init_scale<mi::FoldArgs>": (62, 38, 8, 0),
    "k_lsqr_init_scale<mi::NoFold>": (34, 38, 8, 0),
    "k_lsqr_u": (30, 20, 8, 0),
    "k_lsqr_v": (30, 20, 8, 0),
    "k_lsqr_unorm<mi::FoldArgs>": (78, 37, 8, 0),
    "k_lsqr_unorm<mi::NoFold>": (66, 36, 8, 0),
    "k_lsqr_vnorm<mi::FoldArgs>": (78, 37, 8, 0),
    "k_lsqr_vnorm<mi::NoFold>": (64, 37, 8, 0),
    "k_lsqr_xw<mi::FoldArgs>": (78, 43, 8, 0),
    "k_lsqr_xw<mi::NoFold>": (78, 43, 8, 0),
}
NEW = ("k_lsqr_peek", "k_lsqr_user_stop")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_observer_kernels_use_no_scratch_and_leave_the_pass_kernels_alone():
    ks = _resource_usage("lsqr.hip")
    for n in NEW:
        assert n in ks, sorted(ks)
        assert ks[n][3] == 0 and ks[n][1] <= 16, (n, ks[n])
    now = {n: tuple(v) for n, v in ks.items() if n not in NEW}
    assert sorted(now) == sorted(LSQR_KERNELS_BEFORE), sorted(set(now) ^ set(LSQR_KERNELS_BEFORE))
    changed = {n: (LSQR_KERNELS_BEFORE[n], now[n]) for n in now if now[n] != LSQR_KERNELS_BEFORE[n]}
    assert not changed, changed


def test_library_and_binding_export_the_observed_lsqr():
    from optimization_amd import capi
    L = capi.load()
    assert hasattr(L, "mi_lsqr_observed") and hasattr(L, "mi_lsqr_observer_available")
    assert "observer" in inspect.signature(capi.Context.lsqr).parameters
    assert callable(capi.Context.lsqr_observer_available)


def test_host_driver_with_and_without_a_pack_and_its_k_sequence():
    """the host side of tests/cpp/harness_lsqr_observer.cpp: the user function is called once per pass that no stopping
    rule ended, with k = 0, 1, ...; a stop at k returns num_iterations = k; the pack changes nothing but the counter"""
    import lsqr_observer_py as lo
    H = lo.LsqrObserverHarness()
    lo_, di, up, b = lo.tridiagonal(257)
    a = H.tridiag(0, 0, lo_, di, up, b, btol=1e-10, Atol=1e-10)
    p = H.tridiag(0, 1, lo_, di, up, b, btol=1e-10, Atol=1e-10)
    assert a["rc"] == 0 and p["rc"] == 0
    assert a["calls"] == a["iterations"] > 5          # left through a stopping rule: that pass is not observed
    assert [int(k) for k in a["rec"][:, 0]] == list(range(a["calls"]))
    assert p["counter"] == p["calls"] == a["calls"] and np.array_equal(a["x"], p["x"]) and np.array_equal(a["rec"], p["rec"])
    m = H.tridiag(0, 0, lo_, di, up, b, btol=1e-10, Atol=1e-10, max_iterations=4)
    assert (m["iterations"], m["calls"]) == (4, 4)    # the pass that reaches max_iterations is observed
    s = H.tridiag(0, 1, lo_, di, up, b, btol=1e-10, Atol=1e-10, stop_at=3)
    assert (s["iterations"], s["calls"], s["counter"]) == (3, 4, 4) and np.array_equal(s["x"], m["x"])
