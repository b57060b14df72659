"""GPU parity of the tall-row kernel family (stiefel_tall.hip: k_tall_spmm_gram, k_tall_gram, k_tall_reduce, k_tall_finish,
k_tall_polar) against the longdouble restatement of tests/stiefel_tall_cases.py, at the sizes, grids, matrix forms and
steps the kernels' own tests (test_gpu_stiefel_tall.py) do not reach:
  (a) ragged sizes: n = p (all of O(p)), one row in the last 16-row tile, exactly one workgroup step, ...; a matrix
      with general values (no packed copy: k_tall_spmm_gram<false, true>) and one with three values (<true, true>)
  (b) grids of 1, 2, 3 workgroups (every tile loop takes several strides, the last one partial; the slice partition
      runs at a grid below the work) and 66 000 rows (255 workgroups, a partial second stride)
  (c) MI355OPT_TALL_PROLOGUE=1 against the default: the same bits, at 1, 7, 8, 9 and 17 Gram rows
  (d) retractions with cond(Y'Y) = 1e2, 1e4, 1e6
Bars: so3_cases.TOL_G = 1e-13 for operations, TOL_H = 1e-12 for H eta and the curvature dots.  Gram entries relative to
(|X|'|Z|) entrywise, the objective (half the trace of a Gram) relative to 1/2 tr(|X|'(|A||X|)), fields relative to their
largest entry, sparse products row by row relative to sum |a||v|.  At n = p the objective is constant, so the exact
gradient and Hessian are zero: they are measured in units of the largest entry of A X and of A eta there.

(d) has no bar fixed in advance.  floor = the distance from the longdouble polar factor to Y G64^-1/2, G64 = Y'Y rounded
once to float64 (stiefel_tall_cases.gram_floor): what any method through a float64 Gram pays.  The kernel gets
8 x floor + TOL_G (a float64 iteration adds rounding of its own: its float64 re-enactment from G64 lies 0.6 ... 3.0 x
floor away, test_cpu_stiefel_tall_reference.py).  Floors (max over n = p, 17, 300), measured by the reference alone:
      cond(Y'Y)    p = 9      p = 16
        1e2       6.1e-16    8.7e-16
        1e4       1.0e-13    6.9e-14
        1e6       1.1e-11    8.2e-12"""
import numpy as np
import pytest

import stiefel_tall_cases as tc
from so3_cases import TOL_G, TOL_H

pytestmark = pytest.mark.gpu
LD = tc.LD


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def make_csr(c, r):
    """the matrix of a case on context c, in the form its name promises: the packed copy exists exactly for "few".  A
    symmetric matrix of fewer than 23 rows cannot hold 256 distinct values, so there the general matrix is created with
    the context's NO_PACKED switch on: k_tall_spmm_gram<false, ...> runs at those sizes too"""
    n, form = r["n"], r["form"]
    want_packed = form == "few"
    assert tc.expect_packed(r["val"]) == (want_packed or n < tc.MIN_N_UNPACKABLE)
    force_plain = not want_packed and tc.expect_packed(r["val"])
    if force_plain:
        c.set_option("NO_PACKED", 1)
    try:
        A = c.csr(n, r["rowptr"], r["col"], r["val"])
    finally:
        if force_plain:
            c.set_option("NO_PACKED", 0)
    assert A.format_info()["packed"] == want_packed, (n, form, A.format_info())
    return A


def run_ops(c, r, large=False):
    """every operation of a case on context c: dict of float64 results"""
    n, p = r["n"], r["p"]
    A = make_csr(c, r)
    prob = c.stiefel_rq(A, n, p)
    X, Z, eta = c.upload(r["X"]), c.upload(r["Z"]), c.upload(r["eta"])
    out = dict(gram=c.stiefel_gram(n, p, X, Z),
               project=c.stiefel_project(n, p, X, Z).numpy().reshape(n, p).copy(),
               retract=c.stiefel_retract(n, p, X, c.upload(r["V"])).numpy().reshape(n, p).copy())
    if not large:
        out["spmm"] = A.spmm(p, c.upload(r["W"])).numpy().reshape(n, p).copy()
        out["f"] = prob.objective(X)
    g, H = prob.model(X)
    out["grad"] = g.numpy().reshape(n, p).copy()
    out["hess"] = H.apply(eta).numpy().reshape(n, p).copy()
    if not large:
        out["precon"] = prob.precon(X, c.upload(r["dinv"])).apply(c.upload(r["r"])).numpy().reshape(n, p).copy()
        if r["dots"] is not None:
            # the three dots of k_tall_finish<true> as a solve sees them: one pass from g = eta, p = -eta:
            # kappa_0 = <eta, H eta>, alpha_0 kappa_0 = <eta, eta>
            s = c.stpcg(eta, H, None, Delta=1e150, max_iterations=1, kappa_fgr=1e-10, theta=1.0, trace_cap=4)
            assert len(s["trace"]["kappa"]) == 1, s
            out["kappa"], out["alpha"] = s["trace"]["kappa"][0], s["trace"]["alpha"][0]
    return out


def check_ops(out, r, label):
    """every result of run_ops against longdouble, printed, then asserted"""
    n, p, ref = r["n"], r["p"], r["ref"]
    X = ref.X
    e = {}
    e["gram"] = float((np.abs(out["gram"].astype(LD) - r["gram"]) / r["gram_scale"]).max())
    e["project"] = tc.field_err(out["project"], r["project"])
    Sk = X.T @ out["project"].astype(LD)
    e["skew"] = float(np.abs(Sk + Sk.T).max())
    e["retract"] = tc.field_err(out["retract"], r["retract"])
    Yd = out["retract"].astype(LD)
    e["orth"] = float(np.abs(Yd.T @ Yd - np.eye(p, dtype=LD)).max())
    if n == p:   # exact gradient and Hessian are zero: absolute, in units of the terms they are the difference of
        gs, hs = np.abs(ref.AX).max(), np.abs(tc.spmm(r["rowptr"], r["col"], r["val"], r["eta"])).max()
        e["grad"] = float(np.abs(out["grad"].astype(LD) - r["grad"]).max() / gs)
        e["hess"] = float(np.abs(out["hess"].astype(LD) - r["hess"]).max() / hs)
    else:
        e["grad"], e["hess"] = tc.field_err(out["grad"], r["grad"]), tc.field_err(out["hess"], r["hess"])
    bars = dict(gram=TOL_G, project=TOL_G, skew=1e-13, retract=TOL_G, orth=TOL_G, grad=TOL_G, hess=TOL_H)
    if "spmm" in out:
        d, sc = np.abs(out["spmm"].astype(LD) - r["spmm"]), r["spmm_scale"]
        e["spmm"] = float((d[sc > 0] / sc[sc > 0]).max(initial=0))
        zero = r["spmm"] == 0
        assert zero[np.diff(r["rowptr"]) == 0].all()
        assert np.all(out["spmm"][zero] == 0), f"{label}: an exact zero of A V is not zero"
        e["f"] = float(abs(LD(out["f"]) - r["f"]) / r["f_scale"])
        e["precon"] = tc.field_err(out["precon"], r["precon"])
        bars.update(spmm=TOL_G, f=TOL_G, precon=TOL_G)
    if "kappa" in out:
        k, _, ee = r["dots"]
        e["kappa"] = float(abs(LD(out["kappa"]) - k) / k)
        e["rv"] = float(abs(LD(out["alpha"]) * LD(out["kappa"]) - ee) / ee)
        bars.update(kappa=TOL_H, rv=TOL_H)
    print(f"  {label}: " + ", ".join(f"{k} {v:.1e}" for k, v in e.items()))
    bad = {k: v for k, v in e.items() if not v <= bars[k]}
    assert not bad, f"{label}: beyond the bar: {bad}"
    return e


# ---- (a) ragged sizes, both matrix forms ----
@pytest.mark.parametrize("n", (0,) + tc.RAGGED_N)
@pytest.mark.parametrize("p", tc.TALL_P)
def test_tall_ragged_sizes_both_matrix_forms_vs_longdouble(ctx, p, n):
    """Gram (asymmetric operands), projection (and tangency), retraction at 0.3 P_X(Z), sparse product (and its exact
    zeros), objective, gradient, Hessian, preconditioner and the fused dots at n = p, 16, 17, 63, 64, 65, 241, 255, 256,
    257, 1025 on the general-valued matrix (plain entries) and the three-valued one (packed copy)."""
    n = n or p
    for form in ("general", "few"):
        r = tc.reference_values(n, p, form)
        check_ops(run_ops(ctx, r), r, f"n = {n}, p = {p}, {form}")


# ---- (b) grid stride ----
@pytest.mark.parametrize("n", tc.STRIDE_N)
@pytest.mark.parametrize("grid", (1, 2, 3))
def test_tall_small_grids_take_several_strides_vs_longdouble(grid, n):
    """MAX_GRID = 1, 2, 3 at n = 1025 (65 tiles, 17 slices) and 600 (38 tiles, 10 slices): a workgroup step is 16 tiles,
    so the tile loops take up to five strides with a partial last one and every workgroup owns a run of several slices.
    The order of summation follows the grid: each grid is held against longdouble, not against another grid."""
    from optimization_amd import capi
    c = capi.Context(0)
    try:
        c.set_option("MAX_GRID", grid)
        for p in tc.TALL_P:
            for form in ("general", "few"):
                r = tc.reference_values(n, p, form)
                check_ops(run_ops(c, r), r, f"grid {grid}, n = {n}, p = {p}, {form}")
    finally:
        c.close()


@pytest.mark.parametrize("p", (9, 16))
def test_tall_255_workgroups_partial_second_stride_vs_longdouble(ctx, p):
    """n = 66 000 on a banded matrix: 258 workgroup steps for the 255 workgroups tall_grid allows (MAX_GRID at its
    default of 512), so workgroups 0, 1, 2 take a second stride and the others do not.  Gram, projection, retraction,
    gradient, Hessian."""
    n = tc.LARGE_N
    assert (n + 255) // 256 > 255
    r = tc.reference_values(n, p, "banded", True)
    check_ops(run_ops(ctx, r, large=True), r, f"n = {n}, p = {p}, banded")


# ---- (c) the consumers' prologue reduction ----
@pytest.fixture(scope="module")
def both_modes():
    """(default context, MI355OPT_TALL_PROLOGUE=1 context)"""
    from optimization_amd import capi
    made = []
    try:
        for on in ("0", "1"):
            with pytest.MonkeyPatch.context() as mp:
                mp.setenv("MI355OPT_TALL_PROLOGUE", on)
                made.append(capi.Context(0))
        yield tuple(made)
    finally:
        for c in made:
            c.close()


def _prologue_ops(c, r, h, Delta):
    n, p = r["n"], r["p"]
    out = run_ops(c, r)
    A = make_csr(c, r)
    prob = c.stiefel_rq(A, n, p)
    X = c.upload(r["X"])
    g, H = prob.model(X)
    s = c.stpcg(g, H, None, Delta=Delta, max_iterations=8, kappa_fgr=1e-30, theta=1.0)
    out["step"], out["step_info"] = s["s"].numpy().copy(), (s["iterations"], s["exit_reason"])
    g, H = prob.model(X)
    Xt, t = prob.trial(X, c.upload(h), g)
    out["trial"], out["trial_scalars"] = Xt.numpy().reshape(n, p).copy(), np.array([t[k] for k in ("f", "hh", "gh", "hHh", "grad_sqnorm")])
    return out


@pytest.mark.parametrize("count", tc.PROLOGUE_COUNTS)
def test_tall_prologue_reduction_has_the_bits_of_the_reduce_kernel(both_modes, count):
    """n = 256 count - 100: the producers leave 1, 7, 8, 9, 17 Gram rows (below, at and past the 8-way unrolled body of
    tall_row_sum, with and without its tail).  Projection, retraction, gradient, Hessian, preconditioner, the fused trial
    step and an 8-pass STPCG step: the same bits with the rows summed in the consumers' prologue as with the reduce kernel
    between, and each within the bars against longdouble.  The STPCG step is held to TOL_H or 3 x the distance of the
    float64 run of the restated solve from its longdouble run (conftest.floor_or's rule).  H is indefinite at a random
    point of a matrix with normal weights: the solve is asked for 8 passes and leaves through the boundary rule at its
    first non-positive curvature, after one or two of them, in the restatement and on the device alike."""
    n = 256 * count - 100
    for p in tc.TALL_P:
        r = tc.reference_values(n, p, "general")
        ref = r["ref"]
        h = (LD(0.05) * r["eta"].astype(LD)).astype(np.float64)
        Delta = 10.0
        plain, prologue = (_prologue_ops(c, r, h, Delta) for c in both_modes)
        for k in plain:
            assert np.array_equal(bits(plain[k]), bits(prologue[k])), f"n = {n}, p = {p}: {k} differs between the two modes"
        check_ops(prologue, r, f"prologue, {count} rows, p = {p}")
        # the trial step: retraction along h, the objective there, <h,h>, <g,h>, <h,Hh>
        Ut = ref.retract(h)
        at = tc.TallRef(r["rowptr"], r["col"], r["val"], Ut)
        hl, gl = h.astype(LD), r["grad"]
        f, hh, gh, hHh = (LD(v) for v in prologue["trial_scalars"][:4])
        e = dict(trial=tc.field_err(prologue["trial"], Ut), f=float(abs(f - at.f()) / at.f_scale()),
                 hh=float(abs(hh - (hl * hl).sum()) / (hl * hl).sum()),
                 gh=float(abs(gh - (gl * hl).sum()) / (np.abs(gl) * np.abs(hl)).sum()),
                 hHh=float(abs(hHh - (hl * ref.hess(hl)).sum()) / (hl * ref.hess(hl)).sum()))
        # the 8-pass solve
        s_ld, k_ld, why = tc.stpcg(ref.hess, r["grad"], Delta, 8)
        s_64, _, _ = tc.stpcg(ref.hess, r["grad"], Delta, 8, dtype=np.float64)
        floor = tc.field_err(s_64, s_ld)
        e["step"] = tc.field_err(prologue["step"].reshape(n, p), s_ld)
        print(f"  prologue, {count} rows, p = {p}: " + ", ".join(f"{k} {v:.1e}" for k, v in e.items()) +
              f" (restated solve: {k_ld} passes, {why}, float64 floor {floor:.1e})")
        assert e["trial"] <= TOL_G and e["f"] <= TOL_G and max(e["hh"], e["gh"], e["hHh"]) <= TOL_H
        assert e["step"] <= max(TOL_H, 3 * floor)


# ---- (d) hard retractions ----
@pytest.mark.parametrize("name", tc.HARD_CASES)
def test_tall_retraction_at_large_condition_numbers_vs_jacobi_polar(ctx, name):
    """k_tall_polar at cond(Y'Y) = 1e2, 1e4, 1e6 against the Jacobi polar factor: distance, orthonormality and symmetry
    of U'Y within 8 x floor + TOL_G (the module's header).

    This test caught a loss of accuracy in tall_invsqrt_wave.  With the coupled Newton-Schulz iteration alone the distance
    met the bar (2.5 ... 9.3 x floor), but three cases missed it in the other two quantities: p9_n17_cond1e6
    (orthonormality 5.59e-11, bar 4.48e-11), p9_n300_cond1e6 (symmetry 5.23e-11, bar 3.41e-11) and p16_n17_cond1e4
    (orthonormality 8.28e-13, bar 6.51e-13); the float64 re-enactment of the iteration missed it by the same factors.
    One corrective step M <- M + M (I - M G M) / 2 with the residual accumulated in double-double was added behind the
    iteration.  Measured with it on an MI355X: distance 1.4 ... 5.6 x floor (at most 0.42 of the bar), orthonormality at
    most 0.74 and symmetry at most 0.77 of the bar, all 18 cases."""
    h = tc.hard_retraction(name)
    n, p = h["n"], h["p"]
    U = ctx.stiefel_retract(n, p, ctx.upload(h["X"]), ctx.upload(h["V"])).numpy().reshape(n, p).astype(LD)
    Y = h["X"].astype(LD) + h["V"].astype(LD)
    bar = 8 * h["floor"] + TOL_G
    dist = tc.field_err(U, h["U"])
    orth = float(np.abs(U.T @ U - np.eye(p, dtype=LD)).max())
    M = U.T @ Y
    symm = float(np.abs(M - M.T).max() / np.abs(Y).max())
    print(f"  {name}: cond(Y'Y) {h['cond']:.3e}, floor {h['floor']:.2e}, bar {bar:.2e}; distance {dist:.2e}, "
          f"orthonormality {orth:.2e}, symmetry of U'Y {symm:.2e}")
    assert dist <= bar and orth <= bar and symm <= bar


@pytest.mark.parametrize("p", tc.HARD_P)
@pytest.mark.parametrize("n", tc.HARD_N)
def test_tall_retraction_of_the_zero_step_returns_the_point(ctx, p, n):
    n = n or p
    X = tc.stiefel_point(n, p, seed=5000 + 13 * n + p)
    Y = ctx.stiefel_retract(n, p, ctx.upload(X), ctx.upload(np.zeros((n, p)))).numpy().reshape(n, p)
    e = tc.field_err(Y, X)
    print(f"  V = 0, n = {n}, p = {p}: {e:.2e}")
    assert e <= TOL_G
