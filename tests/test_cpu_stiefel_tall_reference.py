"""The longdouble restatement of the tall-row Stiefel family (tests/stiefel_tall_cases.py) held on the CPU, so that a GPU
test of test_gpu_stiefel_tall_parity.py cannot fail for a reason that is not the kernel's: the Jacobi polar factor has
the defining properties of a polar factor, the restatement agrees with the float64 oracle where the oracle is good, and
the named cases have the condition numbers and the matrix forms their names promise."""
import ctypes as C

import numpy as np
import pytest

import stiefel_tall_cases as tc
from conftest import rel_err
from optimization_amd import workloads as wl
from so3_cases import TOL_G

LD = tc.LD


def _pivots(M):
    """the pivots of the symmetric M by elimination without exchanges, in longdouble: all positive iff M is positive definite"""
    M = np.array(M, dtype=LD)
    piv = []
    for k in range(M.shape[0]):
        piv.append(M[k, k])
        if M[k, k] != 0:
            M[k + 1:, k:] = M[k + 1:, k:] - np.outer(M[k + 1:, k] / M[k, k], M[k, k:])
    return np.array(piv)


def _retraction_cases():
    for name in tc.HARD_CASES:
        h = tc.hard_retraction(name)
        yield name, h["X"], h["V"], h["U"]
    for n, p in ((9, 9), (17, 16), (241, 13), (1025, 12)):       # the moderate step of the ragged cases
        q = tc.inputs(n, p)
        yield f"moderate n = {n}, p = {p}", q["X"], q["V"], tc.polar(q["X"].astype(LD) + q["V"].astype(LD))[0]
    X = tc.stiefel_point(17, 16, seed=1)
    yield "zero step", X, np.zeros_like(X), tc.polar(X)[0]


def test_jacobi_polar_factor_has_the_properties_of_a_polar_factor():
    """U'U = I, U'Y symmetric, U'Y positive definite (positive pivots), each to 1e-17 in longdouble, for every retraction
    case: the properties that define the polar factor, so no second method is needed to trust it"""
    for name, X, V, U in _retraction_cases():
        Y = X.astype(LD) + V.astype(LD)
        p = Y.shape[1]
        M = U.T @ Y
        orth = float(np.abs(U.T @ U - np.eye(p, dtype=LD)).max())
        symm = float(np.abs(M - M.T).max() / np.abs(Y).max())
        piv = _pivots(tc.sym(M))
        print(f"  {name}: |U'U - I| {orth:.1e}, asymmetry of U'Y {symm:.1e}, pivots {float(piv.min()):.2e} ... {float(piv.max()):.2e}")
        assert orth <= 1e-17 and symm <= 1e-17 and piv.min() > 0


def test_hard_retractions_have_the_condition_numbers_their_names_state():
    for name in tc.HARD_CASES:
        h = tc.hard_retraction(name)
        Y = h["X"] + h["V"]
        print(f"  {name}: cond(Y'Y) {h['cond']:.6e} (cap {h['cap']:.0e}), float64-Gram floor {h['floor']:.2e}")
        assert h["cap"] / 2 <= h["cond"] <= h["cap"] * (1 + 1e-6)
        assert np.array_equal(Y, (h["X"].astype(LD) + h["V"].astype(LD)).astype(np.float64))
        # V is tangent at X to the rounding of its largest entry
        K = h["X"].astype(LD).T @ h["V"].astype(LD)
        assert np.abs(K + K.T).max() <= 8 * np.finfo(np.float64).eps * np.abs(h["V"]).max() * h["p"]


def test_float64_reenactment_of_the_kernels_iteration_meets_the_retraction_bar():
    """tall_invsqrt_wave's method in float64 numpy (Newton-Schulz, then one corrective step on a residual formed in
    extended precision), started from the exactly rounded Gram G64, lies within 8 x floor + TOL_G of the Jacobi polar
    factor on every hard case (0.6 ... 3.0 x floor; 2.4 ... 7.1 x without the corrective step), and the iteration runs to
    its 100-step limit at cond(Y'Y) = 1e6 for n = p: the method meets the bar.  Printed beside it, not asserted: the same
    from a Gram SUMMED in float64 by numpy's Y.T @ Y, whose sum of 300 rounded products loses more than one rounding of the
    exact Gram"""
    for name in tc.HARD_CASES:
        h = tc.hard_retraction(name)
        Y = h["X"] + h["V"]
        Yl = Y.astype(LD)
        Minv, steps = tc.newton_schulz64(tc.sym(Yl.T @ Yl).astype(np.float64))
        d = tc.field_err(Yl @ Minv.astype(LD), h["U"])
        summed = tc.field_err(Yl @ tc.newton_schulz64(Y.T @ Y)[0].astype(LD), h["U"])
        print(f"  {name}: {steps} steps, distance {d:.2e}, floor {h['floor']:.2e} ({d / h['floor']:.1f} x); "
              f"from a float64-summed Gram {summed / h['floor']:.1f} x")
        assert d <= 8 * h["floor"] + TOL_G


def test_matrices_have_the_form_their_name_promises():
    """symmetric, every 5th row and column empty, and more than 256 distinct bit patterns (no packed copy) exactly where
    the size allows it; three values and the padding zero (packed copy) for "few" """
    sizes = sorted(set(tc.TALL_P + tc.RAGGED_N + tc.STRIDE_N + tuple(256 * c - 100 for c in tc.PROLOGUE_COUNTS)))
    for n in sizes:
        for form in ("general", "few"):
            rowptr, col, val = tc.matrix(n, form)
            D = np.zeros((n, n))
            for i in range(n):
                D[i, col[rowptr[i]:rowptr[i + 1]]] = val[rowptr[i]:rowptr[i + 1]]
                assert np.all(np.diff(col[rowptr[i]:rowptr[i + 1]]) > 0)
            assert np.array_equal(D, D.T)
            assert not D[::5].any() and not D[:, ::5].any() and np.count_nonzero(np.diff(rowptr)) >= (n * 3) // 5
            k = tc.distinct_values(val)
            print(f"  n = {n}, {form}: {val.size} entries, {k} distinct values")
            assert tc.expect_packed(val) == (form == "few" or n < tc.MIN_N_UNPACKABLE)
            assert form != "few" or k == 4
    rowptr, col, val = tc.matrix(tc.LARGE_N, "banded")
    assert not tc.expect_packed(val) and np.diff(rowptr).max() == 7
    assert tc.MIN_N_UNPACKABLE * (tc.MIN_N_UNPACKABLE + 1) // 2 > 255 >= (tc.MIN_N_UNPACKABLE - 1) * tc.MIN_N_UNPACKABLE // 2


def test_curvature_along_eta_is_safely_positive_in_every_case():
    for n in (17, 241, 600, 1025):
        for p in tc.TALL_P:
            for form in ("general", "few"):
                k, hh, ee = tc.reference_values(n, p, form)["dots"]
                assert k > 0.3 * np.sqrt(hh * ee)
    assert tc.reference_values(9, 9, "general")["dots"] is None
    assert np.abs(tc.reference_values(9, 9, "general")["grad"]).max() < 1e-14     # St(p, p): f is constant


def test_float64_gram_of_the_largest_case_stays_within_the_gram_bar():
    """numpy's own float64 X.T @ Z at n = 66 000, p = 16 against the longdouble Gram, relative to |X|'|Z| entrywise: the
    bar of the GPU test is reachable in float64 at that size"""
    q = tc.inputs(tc.LARGE_N, 16)
    X, Z = q["X"].astype(LD), q["Z"].astype(LD)
    e = float((np.abs((q["X"].T @ q["Z"]).astype(LD) - X.T @ Z) / (np.abs(X).T @ np.abs(Z))).max())
    print(f"  float64 Gram at n = {tc.LARGE_N}: {e:.2e}")
    assert e <= TOL_G


@pytest.mark.parametrize("p", tc.TALL_P)
def test_restatement_agrees_with_the_oracle_on_the_laplacian_case(oracle, p):
    """the 13 x 11 x 9 Laplacian of test_tall_rows_manifold_operations_vs_oracle: sparse product, objective, gradient,
    Hessian, retraction and preconditioner of the longdouble restatement against the float64 oracle, to the 1e-13 that
    test holds the kernels to"""
    nx, ny, nz = 13, 11, 9
    n = nx * ny * nz
    rowptr, col, val = wl.laplacian_3d(nx, ny, nz)
    rowptr, col = np.ascontiguousarray(rowptr, np.int32), np.ascontiguousarray(col, np.int32)
    X0 = wl.random_stiefel(n, p, seed=3 + p)
    rng = np.random.default_rng(p)
    Z = rng.normal(size=(n, p))
    dinv = 1.0 / np.linspace(3.0, 12.0, n)
    ref = tc.TallRef(rowptr, col, val, X0)
    oprob = oracle.stiefel_rq(n, p, rowptr, col, val, dinv=dinv)
    Wo = np.zeros((n, p))
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    oracle.lib.orc_csr_spmm(n, p, rowptr.ctypes.data_as(ip), col.ctypes.data_as(ip), val.ctypes.data_as(dp),
                            np.ascontiguousarray(Z).ctypes.data_as(dp), Wo.ctypes.data_as(dp))
    V = 0.3 * ref.project(Z).astype(np.float64)
    eta = ref.project(rng.normal(size=(n, p))).astype(np.float64)
    go = oracle.eval_grad(oprob, X0.ravel())       # (binds the oracle's model to X0)
    e = dict(spmm=rel_err(tc.spmm(rowptr, col, val, Z).ravel(), Wo.ravel()),
             f=float(abs(ref.f() - oracle.eval_f(oprob, X0.ravel())) / abs(ref.f())),
             grad=rel_err(ref.grad().ravel(), go),
             hess=rel_err(ref.hess(eta).ravel(), oracle.eval_hess(oprob, X0.ravel(), eta.ravel())),
             retract=rel_err(ref.retract(V).ravel(), oracle.eval_retract(oprob, X0.ravel(), V.ravel())),
             precon=rel_err(ref.precon(dinv, go.reshape(n, p)).ravel(), oracle.eval_precon(oprob, X0.ravel(), go)))
    oracle.free(oprob)
    print(f"  p = {p}: " + ", ".join(f"{k} {v:.1e}" for k, v in e.items()))
    assert max(e.values()) <= 1e-13
