"""Pose-graph translations on the device (optimization_amd/csrc/pgo_trans.hip, mi_pgo_trans_*; Optimization/MI355/PoseGraph.h)
against the restatements of tests/pgo_trans_cases.py, which share no code with the kernels.

Bars.  Right-hand side and residuals: the project's bar for pieces, so3_cases.TOL_G = 1e-13 relative to the longdouble
restatement, widened only by the float64 numpy restatement's own distance from the longdouble figures (logged).  Operator:
TOL_H = 1e-12.  Solve (tol = 1e-12): 1e-10 relative in the iterate against the dense solve refined in longdouble.  A float64
numpy Jacobi-PCG with the same stopping rule stays within 2.3e-12 of the refined dense solution on these graphs (35-55
iterations at Jacobi-scaled condition numbers 7 - 5e3; path_300: 299 iterations at 2.6e5) -- almost two decades under the
bar; the solve test logs those figures again.

Where tau cuts components off the anchor (every 7th tau zero on path_300: 43 pieces; a zero-degree anchor: the whole graph)
L_a is singular and has no dense solve: the reference is then the refined dense least-squares solution with the
degree-weighted mean removed on each such component, which is what Jacobi-PCG from t = 0 converges to
(pgo_trans_cases.dense_solve_refined).  The bar is the same."""
import numpy as np
import pytest

import pgo_trans_cases as pc
from so3_cases import LD, TOL_G, TOL_H

pytestmark = pytest.mark.gpu
NAMES = tuple(pc.CASES)
SOLVE_BAR = 1e-10


def make(ctx, name, kind, anchor):
    from optimization_amd import capi
    N, ei, ej, tt, tau, R = pc.problem(name, kind)
    return capi.PgoTranslations(ctx, N, ei, ej, tt, tau, anchor), ctx.upload(R.ravel())


def field(N, seed):
    return np.random.Generator(np.random.PCG64(seed)).normal(size=3 * N)


def rel_scalar(a, ref):
    """|a - ref| / |ref| with the difference in longdouble (ref = 0, every tau zero: |a|)"""
    d = abs(LD(a) - LD(ref))
    return float(d / abs(LD(ref))) if ref != 0 else float(d)


def residual_rounding(N, ei, ej, tau, t, b):
    """the 2-norm of (row entries + 2) eps (|L| |t| + |b|): what a float64 evaluation of L t - b may be off by"""
    a = np.abs(np.asarray(t, dtype=np.float64)).reshape(N, 3)
    s = pc.weighted_degree(N, ei, ej, tau)[:, None] * a + np.abs(np.asarray(b, dtype=np.float64)).reshape(N, 3)
    np.add.at(s, ei, tau[:, None] * a[ej])
    np.add.at(s, ej, tau[:, None] * a[ei])
    rows = np.bincount(np.concatenate([ei, ej]).astype(np.int64), minlength=N) + 3
    return float(np.linalg.norm(rows[:, None] * np.finfo(float).eps * s))


@pytest.mark.parametrize("kind", pc.TAU_KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_rhs_and_residuals_against_longdouble(ctx, name, kind):
    N, ei, ej, tt, tau, R = pc.problem(name, kind)
    E = ei.size
    t = field(N, 3)
    r_ld, f_ld, m_ld = pc.residual_ref(N, ei, ej, tt, tau, R, t)
    r_64, f_64, m_64 = pc.residual_ref(N, ei, ej, tt, tau, R, t, np.float64)
    for anchor in pc.anchors(name, kind):
        T, Rd = make(ctx, name, kind, anchor)
        unit = np.repeat(pc.unit_rows(N, ei, ej, tau, anchor), 3)
        b_ld = pc.rhs_ref(N, ei, ej, tt, tau, R, anchor)
        floor = pc.rel_ld(pc.rhs_ref(N, ei, ej, tt, tau, R, anchor, np.float64), b_ld)
        b1, b2 = T.rhs(Rd).numpy(), T.rhs(Rd).numpy()
        err = pc.rel_ld(b1, b_ld) if np.any(b_ld != 0) else float(np.abs(b1).max(initial=0.0))
        print(f"{name} {kind} anchor {anchor}: rhs {err:.2e} (float64 restatement {floor:.2e})")
        assert err <= TOL_G + floor
        assert np.array_equal(b1.view(np.uint64), b2.view(np.uint64)), "two launches of the right-hand side differ"
        assert np.all(b1[unit] == 0), "b is not exactly 0 at the anchor / on a zero-degree node"
        # residuals: the per-edge vector, the objective and the largest residual; the same numbers without the vector
        td = ctx.upload(t)
        r1, f1, m1 = T.residual(Rd, td)
        _, f2, m2 = T.residual(Rd, td)
        _, f3, m3 = T.residual(Rd, td, with_vector=False)
        assert (f1, m1) == (f2, m2) == (f3, m3), "the residual pass is not bit-reproducible / depends on r_out"
        if E:
            rfloor = pc.rel_ld(r_64, r_ld)
            ffloor, mfloor = rel_scalar(f_64, f_ld), rel_scalar(m_64, m_ld)
            rerr = pc.rel_ld(r1.numpy(), r_ld)
            ferr, merr = rel_scalar(f1, f_ld), rel_scalar(m1, m_ld)
            print(f"    residuals {rerr:.2e} ({rfloor:.2e}), f {ferr:.2e} ({ffloor:.2e}), max {merr:.2e} ({mfloor:.2e})")
            assert rerr <= TOL_G + rfloor and ferr <= TOL_G + ffloor and merr <= TOL_G + mfloor
        else:
            assert f1 == 0 and m1 == 0


@pytest.mark.parametrize("name", NAMES)
def test_operator_against_the_restatement_and_through_stpcg(ctx, name):
    kind = "every_7th_zero"
    N, ei, ej, tt, tau, R = pc.problem(name, kind)
    anchor = pc.anchors(name, kind)[-1]
    T, Rd = make(ctx, name, kind, anchor)
    L, P = T.operator()
    for seed in (1, 2):
        x = field(N, seed)
        ref = pc.laplacian_apply_ref(N, ei, ej, tau, anchor, x)
        got = L.apply(ctx.upload(x)).numpy()
        err = pc.rel_ld(got, ref)
        print(f"{name} anchor {anchor}: L x {err:.2e}")
        assert err <= TOL_H
    _, _, _, dinv, _ = pc.laplacian_csr(N, ei, ej, tau, anchor)
    assert np.array_equal(P.apply(ctx.upload(np.ones(3 * N))).numpy(), dinv)
    # the borrowed pair through the caller's own mi_stpcg: one fused solve, the iterate of mi_pgo_trans_solve bit for bit
    b = T.rhs(Rd)
    ctx.fusion_counters(reset=True)
    r = ctx.stpcg(b.scaled(-1.0), L, P, Delta=1e150, max_iterations=1000, kappa_fgr=1e-12, theta=0.0)
    fc = ctx.fusion_counters()
    assert fc["fused_stpcg_solves"] == 1 and fc["generic_stpcg_solves"] == 0 and fc["generic_inner_products"] == 0, fc
    t, info = T.solve(Rd, tol=1e-12)
    assert np.array_equal(r["s"].numpy().view(np.uint64), t.numpy().view(np.uint64))
    assert r["iterations"] == info["iterations"] and r["exit_reason"] == 0 and info["exit_reason"] == "RESIDUAL"


@pytest.mark.parametrize("kind", pc.TAU_KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_solve_against_the_refined_dense_solution(ctx, name, kind):
    N, ei, ej, tt, tau, R = pc.problem(name, kind)
    for n_anchor, anchor in enumerate(pc.anchors(name, kind)):
        T, Rd = make(ctx, name, kind, anchor)
        unit = np.repeat(pc.unit_rows(N, ei, ej, tau, anchor), 3)
        b_ld = pc.rhs_ref(N, ei, ej, tt, tau, R, anchor)
        t_ref = pc.dense_solve_refined(N, ei, ej, tau, anchor, b_ld).ravel()
        if n_anchor == 0:
            # the reference alone: the float64 restatement of the iteration, and the Jacobi-scaled condition number
            A = pc.dense_laplacian(N, ei, ej, tau, anchor)
            _, _, _, dinv, _ = pc.laplacian_csr(N, ei, ej, tau, anchor)
            t_pcg, its = pc.pcg_f64(A, dinv, b_ld.astype(np.float64), 1e-12, 1000)
            s = np.sqrt(dinv[::3])
            ev = np.linalg.eigvalsh(s[:, None] * A * s[None, :])
            ev = ev[ev > 1e-12 * ev[-1]]    # (components that tau cuts off the anchor leave zero eigenvalues: not counted)
            print(f"{name} {kind} anchor {anchor}: float64 PCG restatement {its} iterations, "
                  f"{pc.rel_ld(t_pcg, t_ref) if np.any(t_ref != 0) else 0.0:.2e} from the refined dense solution, "
                  f"Jacobi-scaled condition number {ev[-1] / ev[0]:.1e}")
        t, info = T.solve(Rd, tol=1e-12)
        th = t.numpy()
        err = pc.rel_ld(th, t_ref) if np.any(t_ref != 0) else float(np.abs(th).max(initial=0.0))
        print(f"{name} {kind} anchor {anchor}: {info['iterations']} iterations, exit {info['exit_reason']}, iterate {err:.2e}, "
              f"|L t - b| / |b| = {info['relative_residual']:.2e}")
        assert info["exit_reason"] == "RESIDUAL"
        assert err <= SOLVE_BAR
        assert np.all(th[unit] == 0), "t is not exactly 0 at the anchor / on a zero-degree node"
        # info against what the test recomputes from t_out
        bn = np.sqrt((b_ld * b_ld).sum())
        res = np.sqrt(((pc.laplacian_apply_ref(N, ei, ej, tau, anchor, th) - b_ld) ** 2).sum())
        want = float(res / bn) if bn > 0 else float(res)
        # the device forms L t - b in float64: row i carries at most (entries + 2) eps (|L| |t| + |b|)_i of rounding, which is
        # what the two figures may differ by (the norms themselves add 1e-12 relative)
        slack = residual_rounding(N, ei, ej, tau, th, b_ld) / (float(bn) if bn > 0 else 1.0)
        print(f"    relative residual recomputed in longdouble {want:.3e}, rounding allowance {slack:.1e}")
        assert abs(info["relative_residual"] - want) <= slack + 1e-12 * want, (info["relative_residual"], want)
        # f_tau and max |r_e| at the solution are differences of positions: float64 forms r_e to delta_e = 8 eps (|t_j| + |t_i| +
        # |tt_e|), hence f_tau to sum tau (|r_e| delta_e + delta_e^2) (+ 1e-13 f_tau for the sum) and the maximum to max delta_e
        r_ld, f_ld, m_ld = pc.residual_ref(N, ei, ej, tt, tau, R, th)
        if ei.size:
            tn = np.linalg.norm(th.reshape(N, 3), axis=1)
            delta = 8 * np.finfo(float).eps * (tn[ei] + tn[ej] + np.linalg.norm(tt, axis=1))
            rn = np.linalg.norm(r_ld.reshape(-1, 3).astype(np.float64), axis=1)
            assert abs(LD(info["objective"]) - f_ld) <= float((tau * (rn * delta + delta * delta)).sum()) + 1e-13 * float(f_ld)
            assert abs(LD(info["max_residual"]) - m_ld) <= float(delta.max())
        _, f2, m2 = T.residual(Rd, t, with_vector=False)
        assert (info["objective"], info["max_residual"]) == (f2, m2)


@pytest.mark.parametrize("name", ("ring_chords_1025", "hub_last", "multigraph_linspace", "path_300"))
def test_noise_free_measurements_give_the_true_positions(ctx, name):
    from optimization_amd import capi
    N, ei, ej, _, tau, R = pc.problem(name, "linspace")
    anchor = pc.anchors(name, "linspace")[-1]
    t_true = np.random.Generator(np.random.PCG64(77)).normal(size=(N, 3)) * 3
    Rm = R.reshape(N, 3, 3)
    tt = np.einsum("eba,eb->ea", Rm[ei], t_true[ej] - t_true[ei])    # R_i' (t_j - t_i)
    T = capi.PgoTranslations(ctx, N, ei, ej, tt, tau, anchor)
    t, info = T.solve(ctx.upload(R.ravel()), tol=1e-12)
    want = (t_true - t_true[anchor]).ravel()
    err = pc.rel_ld(t.numpy(), want)
    scale = float((tau * (tt * tt).sum(axis=1)).sum())
    print(f"{name}: positions {err:.2e}, f_tau / sum tau |tt|^2 = {info['objective'] / scale:.2e}, {info['iterations']} iterations")
    assert info["exit_reason"] == "RESIDUAL" and err <= SOLVE_BAR
    # what the iterate's bar leaves for f_tau: every |r_e| <= 2 x 1e-10 |t| when the iterate is within 1e-10 |t| of the truth
    assert info["objective"] <= 0.5 * tau.sum() * (2 * SOLVE_BAR * np.linalg.norm(want)) ** 2
    assert info["objective"] <= 1e-16 * scale, "f_tau is not at rounding level relative to sum tau |tt|^2"


def test_refusals_reach_the_c_abi(ctx):
    from optimization_amd import capi
    N, ei, ej, tt, tau, R = pc.problem("ring_chords_1023", "linspace")
    with pytest.raises(capi.MiError, match=r"anchor 1023 is outside \[0, N\)"):
        capi.PgoTranslations(ctx, N, ei, ej, tt, tau, N)
    bw = tau.copy()
    bw[5] = -1.0
    with pytest.raises(capi.MiError, match="edge 5 has a negative or non-finite weight"):
        capi.PgoTranslations(ctx, N, ei, ej, tt, bw, 0)
    T = capi.PgoTranslations(ctx, N, ei, ej, tt, tau, 0)
    with pytest.raises(capi.MiError, match="R must hold N row-major 3x3 blocks"):
        T.rhs(ctx.upload(np.zeros(9 * N + 9)))
    with pytest.raises(capi.MiError, match="tolerance"):
        T.solve(ctx.upload(R.ravel()), tol=1.0)


@pytest.mark.parametrize("name", ("ring_chords_1025", "hub_first", "isolated_1500"))
def test_header_layer_matches_the_c_abi_bit_for_bit(ctx, name):
    from harness_pgo_trans_py import PgoTransHarness
    kind = "every_7th_zero"
    N, ei, ej, tt, tau, R = pc.problem(name, kind)
    anchor = pc.anchors(name, kind)[-1]
    h = PgoTransHarness().run(N, ei, ej, tt, tau, anchor, R.ravel(), tol=1e-12)
    assert h["rc"] == 0, h["err"]
    assert (h["solve_fused"], h["solve_generic"], h["solve_inner_products"]) == (1, 0, 0), h
    assert (h["client_fused"], h["client_generic"], h["client_inner_products"]) == (1, 0, 0), h
    T, Rd = make(ctx, name, kind, anchor)
    t, info = T.solve(Rd, tol=1e-12)
    bits = t.numpy().view(np.uint64)
    assert np.array_equal(h["t_solve"].view(np.uint64), bits), "TranslationRecovery::solve differs from mi_pgo_trans_solve"
    assert np.array_equal(h["t_client"].view(np.uint64), bits), "the client's own STPCG call differs from mi_pgo_trans_solve"
    assert h["iterations"] == h["client_iterations"] == info["iterations"] and h["exit_reason"] == 0
    assert (h["objective"], h["relative_residual"], h["max_residual"]) == \
        (info["objective"], info["relative_residual"], info["max_residual"])
    assert np.array_equal(h["b"].view(np.uint64), T.rhs(Rd).numpy().view(np.uint64))
    r, f, m = T.residual(Rd, t)
    assert np.array_equal(h["r"].view(np.uint64), r.numpy().view(np.uint64)) and (h["residuals_objective"], h["residuals_max"]) == (f, m)
