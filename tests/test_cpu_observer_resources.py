"""The two kernels the observed fused STPCG adds (stpcg.hip: k_cg_peek, one workgroup between the operator pass and
k_cg_update of every pass of mi_stpcg_observed; k_cg_user_stop, the observer's stop) use no scratch memory, and adding
them leaves every instantiation of the step kernels -- k_cg_update*, k_cg_pupdate* -- with exactly the registers,
occupancy and scratch it had before: the un-observed solve launches the code it always launched.  Read from the
compiler's resource-usage remarks (no GPU needed).

Also on the CPU: the host side of tests/cpp/harness_observer.cpp, i.e. where the records of
tests/test_gpu_stpcg_observer.py can be held to 1e-10 at all."""
import inspect
import os

import numpy as np
import pytest

from test_cpu_kernel_resources import HIPCC, _resource_usage

# (TotalSGPRs, VGPRs, waves/SIMD, scratch bytes per lane) of every k_cg_update* / k_cg_pupdate* instantiation as the
# commit before the observed solve compiled them
STEP_KERNELS_BEFORE = {
    "k_cg_pupdate<false, 0, mi::NoFold>": (76, 52, 8, 0),
    "k_cg_pupdate<false, 2, mi::NoFold>": (84, 78, 6, 0),
    "k_cg_pupdate<false, 3, mi::NoFold>": (82, 118, 4, 0),
    "k_cg_pupdate<false, 4, mi::NoFold>": (82, 128, 4, 156),
    "k_cg_pupdate<true, 2, mi::NoFold>": (91, 78, 6, 0),
    "k_cg_pupdate<true, 3, mi::NoFold>": (91, 118, 4, 0),
    "k_cg_pupdate<true, 4, mi::NoFold>": (91, 128, 4, 156),
    "k_cg_pupdate_ds<false>": (78, 49, 8, 0),
    "k_cg_pupdate_ds<true>": (78, 54, 8, 0),
    "k_cg_pupdate_early": (77, 64, 8, 0),
    "k_cg_pupdate_s80<false, 0, mi::FoldArgs>": (78, 53, 8, 0),
    "k_cg_pupdate_s80<false, 0, mi::FoldPush>": (78, 53, 8, 0),
    "k_cg_pupdate_s80<false, 1, mi::NoFold>": (78, 48, 8, 0),
    "k_cg_pupdate_s80<true, 0, mi::NoFold>": (78, 41, 8, 0),
    "k_cg_pupdate_s80<true, 1, mi::NoFold>": (78, 47, 8, 0),
    "k_cg_update<0, false, 18, mi::NoFold>": (92, 68, 7, 0),
    "k_cg_update<0, false, 24, mi::NoFold>": (92, 80, 6, 0),
    "k_cg_update<0, false, 3, mi::NoFold>": (74, 47, 8, 0),
    "k_cg_update<0, false, 31, mi::NoFold>": (92, 96, 5, 0),
    "k_cg_update<0, false, 39, mi::NoFold>": (92, 112, 4, 0),
    "k_cg_update<0, false, 4, mi::NoFold>": (80, 47, 8, 0),
    "k_cg_update<0, false, 6, mi::NoFold>": (80, 47, 8, 0),
    "k_cg_update<0, false, 9, mi::NoFold>": (80, 52, 8, 0),
    "k_cg_update<0, true, 18, mi::NoFold>": (104, 36, 7, 0),
    "k_cg_update<0, true, 24, mi::NoFold>": (106, 36, 7, 0),
    "k_cg_update<0, true, 3, mi::NoFold>": (74, 31, 8, 0),
    "k_cg_update<0, true, 31, mi::NoFold>": (106, 36, 7, 0),
    "k_cg_update<0, true, 39, mi::NoFold>": (106, 36, 7, 0),
    "k_cg_update<1, false, 3, mi::NoFold>": (78, 50, 8, 0),
    "k_cg_update<1, true, 3, mi::NoFold>": (78, 46, 8, 0),
    "k_cg_update<2, false, 3, mi::NoFold>": (74, 50, 8, 0),
    "k_cg_update<2, true, 3, mi::NoFold>": (74, 48, 8, 0),
    "k_cg_update<3, false, 3, mi::NoFold>": (74, 47, 8, 0),
    "k_cg_update<3, true, 3, mi::NoFold>": (74, 32, 8, 0),
    "k_cg_update_ns<0, false, 18, mi::NoFold>": (92, 70, 7, 0),
    "k_cg_update_ns<0, false, 24, mi::NoFold>": (92, 82, 5, 0),
    "k_cg_update_ns<0, false, 3, mi::NoFold>": (70, 47, 8, 0),
    "k_cg_update_ns<0, false, 31, mi::NoFold>": (92, 95, 5, 0),
    "k_cg_update_ns<0, false, 39, mi::NoFold>": (92, 111, 4, 0),
    "k_cg_update_ns<0, false, 4, mi::NoFold>": (74, 47, 8, 0),
    "k_cg_update_ns<0, false, 6, mi::NoFold>": (74, 47, 8, 0),
    "k_cg_update_ns<0, false, 9, mi::NoFold>": (74, 52, 8, 0),
    "k_cg_update_ns<1, false, 3, mi::NoFold>": (76, 50, 8, 0),
    "k_cg_update_ns<2, false, 3, mi::NoFold>": (68, 50, 8, 0),
    "k_cg_update_ns<3, false, 3, mi::NoFold>": (70, 47, 8, 0),
    "k_cg_update_ns_s80<0, false, 16, mi::NoFold>": (74, 64, 8, 20),
    "k_cg_update_s80<0, false, 16, mi::FoldArgs>": (78, 64, 8, 0),
    "k_cg_update_s80<0, false, 16, mi::NoFold>": (78, 60, 8, 20),
    "k_cg_update_s80<0, false, 4, mi::FoldArgs>": (78, 50, 8, 0),
    "k_cg_update_s80<0, false, 6, mi::FoldArgs>": (78, 50, 8, 0),
    "k_cg_update_s80<0, false, 9, mi::FoldArgs>": (78, 50, 8, 0),
    "k_cg_update_s80<0, true, 16, mi::NoFold>": (78, 36, 8, 0),
    "k_cg_update_s80<0, true, 4, mi::NoFold>": (78, 36, 8, 0),
    "k_cg_update_s80<0, true, 6, mi::NoFold>": (78, 36, 8, 0),
    "k_cg_update_s80<0, true, 9, mi::NoFold>": (78, 36, 8, 0),
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_observer_kernels_use_no_scratch_and_leave_the_step_kernels_alone():
    cg = _resource_usage("stpcg.hip")
    for n in ("k_cg_peek", "k_cg_user_stop"):
        assert n in cg, sorted(cg)[:8]
        assert cg[n][3] == 0, (n, cg[n])
    assert cg["k_cg_peek"][1] <= 64
    now = {n: v for n, v in cg.items() if n.startswith(("k_cg_update", "k_cg_pupdate"))}
    assert sorted(now) == sorted(STEP_KERNELS_BEFORE), sorted(set(now) ^ set(STEP_KERNELS_BEFORE))
    changed = {n: (STEP_KERNELS_BEFORE[n], now[n]) for n in now if tuple(now[n]) != STEP_KERNELS_BEFORE[n]}
    assert not changed, changed


def test_binding_and_header_declare_the_observed_solve():
    from optimization_amd import capi
    L = capi.load()
    assert hasattr(L, "mi_stpcg_observed")
    assert "observer" in inspect.signature(capi.Context.stpcg).parameters
    assert capi.STATUS[7] == "MI_DECLINED" and capi.STPCG_EXIT[4] == "USER"
    assert L.mi_status_string(7).decode().startswith("declined")
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mi355opt.h")).read()
    assert "NO_FUSED_OBSERVER" in hdr and "MI_STPCG_EXIT_USER = 4" in hdr


@pytest.fixture(scope="module")
def obs():
    import observer_py
    return observer_py.ObserverHarness()


def test_host_driver_equals_the_fixture_of_the_reference(obs, golden):
    """the templated driver on the host vector IS the generic loop the reference fixture was made with: every case of
    tests/golden/stpcg_user_stop.json, bit for bit"""
    import oracle_py
    fx = golden("stpcg_user_stop.json")
    pr = oracle_py.stpcg_stop_problem(fx["n"], fx["seed"])
    for c in fx["cases"]:
        r = obs.diag(0, pr["g"], pr["D"], pr["Minv"] if c["precon"] else None, 1e6, 100, 1e-10, 1.0, stop_at=c["stop_at"])
        assert r["rc"] == 0 and (r["iterations"], r["calls"]) == (c["iterations"], c["calls"])
        assert np.array_equal(r["s"], np.array(c["s"])) and r["M_norm"] == c["M_norm"]
        assert [int(k) for k in r["rec"][:, 0]] == list(range(r["calls"]))


@pytest.mark.parametrize("precon", [False, True])
def test_depth_at_which_the_host_record_is_its_own_to_1e_11(obs, precon):
    """kappa_fgr of the host-against-device comparison (test_gpu_stpcg_observer.py): the host loop leaves by the
    residual test well before max_iterations, and its own record -- k, alpha, <s,s>, <r,r>, <r,v>, <p,p>, <s,p> per call --
    moves by less than 1e-11 when every element of g moves by one ulp, so that 1e-10 can be asked of another summation
    order.  (On the fixture's preconditioned problem the same measurement gives 1e-9 at pass 18 and O(1) from pass 26.)"""
    import oracle_py
    from observer_py import KAPPA_PLAIN, KAPPA_PRECON
    pr = oracle_py.stpcg_stop_problem()
    kappa = KAPPA_PRECON if precon else KAPPA_PLAIN
    rng = np.random.default_rng(1)
    base = obs.diag(0, pr["g"], pr["D"], pr["Minv"] if precon else None, 1e6, 400, kappa, 1.0)
    assert 4 <= base["iterations"] < 100 and base["calls"] == base["iterations"]
    worst = 0.0
    for _ in range(5):
        g2 = np.nextafter(pr["g"], np.where(rng.random(pr["g"].size) < .5, np.inf, -np.inf))
        r = obs.diag(0, g2, pr["D"], pr["Minv"] if precon else None, 1e6, 400, kappa, 1.0)
        assert r["calls"] == base["calls"]
        d = np.abs(r["rec"][:, 1:] - base["rec"][:, 1:]) / np.maximum(np.abs(base["rec"][:, 1:]), 1e-300)
        worst = max(worst, float(d.max()))
    print("precon %s: %d passes, record moves by %.1e under one ulp of g" % (precon, base["iterations"], worst))
    assert worst < 1e-11
