"""The whole drop-in TNT on St(n, 12) through the device harness: inner solves on the tall-row family's two-pass
Hessian (curvature dots fused into the finish pass), fused trial steps, against the CPU oracle's run on the same
arrays -- the parameters and checks of test_tnt_stiefel_wide_rows_device_vs_oracle."""
import numpy as np
import pytest

from conftest import floor_or, rel_err
from optimization_amd import workloads as wl

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def harness():
    import harness_py
    return harness_py.DeviceHarness()


def test_tnt_stiefel_tall_rows_device_vs_oracle(harness, oracle, oracle_omp):
    nx, ny, nz, p = 30, 28, 26, 12
    n = nx * ny * nz
    rowptr, col, val = wl.laplacian_3d(nx, ny, nz)
    X0 = wl.random_stiefel(n, p, seed=17 + p)
    prm = oracle.default_params(gradient_tolerance=1e-6, relative_decrease_tolerance=0, stepsize_tolerance=0,
                                preconditioned_gradient_tolerance=0, Delta_tolerance=0, max_iterations=10,
                                max_TPCG_iterations=40)
    oprob = oracle.stiefel_rq(n, p, rowptr, col, val)
    o = oracle.tnt(oprob, X0.ravel(), prm)
    r = harness.tnt_stiefel(n, p, rowptr, col, val, X0, prm, 0)
    assert r["rc"] == 0, r.get("err")
    assert r["outer_iterations"] == o["outer_iterations"]
    assert list(r["inner_iterations"]) == list(o["inner_iterations"])
    assert r["accepted"] == o["accepted"]
    assert np.allclose(r["objective_values"], o["objective_values"], rtol=1e-11)
    assert np.allclose(r["gradient_norms"], o["gradient_norms"], rtol=1e-7, atol=1e-12)
    ex, floor = rel_err(r["x"], o["x"]), None
    if oracle_omp is not None:
        op = oracle_omp.stiefel_rq(n, p, rowptr, col, val)
        floor = rel_err(oracle_omp.tnt(op, X0.ravel(), prm)["x"], o["x"])
        oracle_omp.free(op)
    print(f"tnt stiefel p = {p}: iterate error {ex:.2e}, re-associated reference {floor}")
    assert ex <= floor_or(1e-10, floor)
    X = r["x"].reshape(n, p)
    assert np.abs(X.T @ X - np.eye(p)).max() < 1e-12
    oracle.free(oprob)
