"""GPU parity tests of the tall-row kernel family (stiefel_tall.hip): Stiefel St(n, p) for rows of 9 ... 16 doubles --
the sparse product, the manifold operations, the Rayleigh-quotient model and STPCG on its two-pass Hessian (curvature
dots fused into the finish pass) against the CPU oracle, the fused trial steps against the separate calls, and the
refusals of what the family does not do."""
import ctypes as C

import numpy as np
import pytest

from conftest import rel_err
from optimization_amd import workloads as wl
from test_gpu_stiefel import _random_csr

pytestmark = pytest.mark.gpu

TALL_P = [9, 12, 13, 16]   # the first tall width, an even one, an odd one with unaligned rows, the full tile


def _oracle_spmm(oracle, n, p, rowptr, col, val, V):
    Wo = np.zeros((n, p))
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    Vc = np.ascontiguousarray(V)
    oracle.lib.orc_csr_spmm(n, p, rowptr.ctypes.data_as(ip), col.ctypes.data_as(ip), val.ctypes.data_as(dp),
                            Vc.ctypes.data_as(dp), Wo.ctypes.data_as(dp))
    return Wo


@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 257, 5000])
def test_tall_spmm_ragged_packed_and_plain_vs_oracle(oracle, monkeypatch, n):
    """mi_csr_spmm for every tall width on a ragged random matrix with empty rows, at sizes with a partial 16-row tile, a
    partial 64-row slice and a partial last workgroup: general values (plain 12-byte entries) against the oracle, and
    values from a small set, so that the value-indexed packed copy is what the kernel reads, packed and plain
    (MI355OPT_NO_PACKED=1) against the oracle and each other.  The product is summed entry by entry in storage order
    with products and sums rounded separately, as the oracle's loop does: equal bits."""
    from optimization_amd import capi
    empty = 5 if n > 4 else 0
    rowptr, col, val = _random_csr(n, seed=100 * n + 7, empty_every=empty)
    val_few = np.random.default_rng(n).choice(np.array([-1.0, .5, 2.0, -0.0]), size=val.size)
    out = {}
    for mode in ("packed", "plain"):
        monkeypatch.setenv("MI355OPT_NO_PACKED", "1" if mode == "plain" else "0")
        c = capi.Context(0)
        try:
            A, Af = c.csr(n, rowptr, col, val), c.csr(n, rowptr, col, val_few)
            for p in TALL_P:
                V = np.random.default_rng(p).normal(size=(n, p))
                Vd = c.upload(V)
                out[mode, p, "general"] = A.spmm(p, Vd).numpy().reshape(n, p).copy()
                out[mode, p, "few"] = Af.spmm(p, Vd).numpy().reshape(n, p).copy()
        finally:
            c.close()
    for p in TALL_P:
        V = np.random.default_rng(p).normal(size=(n, p))
        Wo, Wf = _oracle_spmm(oracle, n, p, rowptr, col, val, V), _oracle_spmm(oracle, n, p, rowptr, col, val_few, V)
        for mode in ("packed", "plain"):
            assert np.allclose(out[mode, p, "general"], Wo, rtol=1e-13, atol=1e-13), (mode, p)
            assert np.array_equal(out[mode, p, "few"], Wf), (mode, p)
        assert np.array_equal(out["packed", p, "few"], out["plain", p, "few"]), p


@pytest.mark.parametrize("p", TALL_P)
def test_tall_rows_manifold_operations_vs_oracle(ctx, oracle, p):
    """Gram, tangent projection, polar retraction, objective, gradient and Hessian of the Rayleigh-quotient problem for
    rows of 9 ... 16 doubles against the oracle, with the properties and the bars of the p = 5 ... 8 test
    (test_wide_rows_manifold_operations_vs_oracle): 1e-13 for the operations."""
    nx, ny, nz = 13, 11, 9
    n = nx * ny * nz
    rowptr, col, val = wl.laplacian_3d(nx, ny, nz)
    X0 = wl.random_stiefel(n, p, seed=3 + p)
    A = ctx.csr(n, rowptr, col, val)
    prob = ctx.stiefel_rq(A, n, p)
    oprob = oracle.stiefel_rq(n, p, rowptr, col, val)
    rng = np.random.default_rng(p)
    Z = rng.normal(size=(n, p))
    X, Zd = ctx.upload(X0), ctx.upload(Z)
    assert np.allclose(ctx.stiefel_gram(n, p, X, Zd), X0.T @ Z, rtol=1e-12, atol=1e-13)
    Pz = ctx.stiefel_project(n, p, X, Zd).numpy().reshape(n, p)
    M = X0.T @ Z
    e = np.abs(Pz - (Z - X0 @ (0.5 * (M + M.T)))).max()
    print(f"p = {p}: projection {e:.2e}")
    assert np.allclose(Pz, Z - X0 @ (0.5 * (M + M.T)), atol=1e-13)
    Sk = X0.T @ Pz
    print(f"p = {p}: skew {np.abs(Sk + Sk.T).max():.2e}")
    assert np.abs(Sk + Sk.T).max() < 1e-13
    V = 0.3 * Pz
    Y = ctx.stiefel_retract(n, p, X, ctx.upload(V)).numpy().reshape(n, p)
    Yo = oracle.eval_retract(oprob, X0.ravel(), V.ravel()).reshape(n, p)
    print(f"p = {p}: retraction {rel_err(Y, Yo):.2e}, orthonormality {np.abs(Y.T @ Y - np.eye(p)).max():.2e}")
    assert rel_err(Y, Yo) < 1e-13 and np.abs(Y.T @ Y - np.eye(p)).max() < 1e-13
    f, fo = prob.objective(X), oracle.eval_f(oprob, X0.ravel())
    print(f"p = {p}: objective {abs(f - fo) / abs(fo):.2e}")
    assert abs(f - fo) <= 1e-13 * abs(fo)
    g, H = prob.model(X)
    go = oracle.eval_grad(oprob, X0.ravel())
    print(f"p = {p}: gradient {rel_err(g.numpy(), go):.2e}")
    assert rel_err(g.numpy(), go) < 1e-13
    Vt = ctx.stiefel_project(n, p, X, ctx.upload(rng.normal(size=(n, p))))
    Hv = H.apply(Vt)
    eh = rel_err(Hv.numpy(), oracle.eval_hess(oprob, X0.ravel(), Vt.numpy()))
    print(f"p = {p}: Hessian {eh:.2e}")
    assert eh < 1e-13
    U = ctx.stiefel_project(n, p, X, ctx.upload(rng.normal(size=(n, p))))
    a, b = U.dot(Hv), Vt.dot(H.apply(U))
    assert abs(a - b) <= 1e-12 * max(abs(a), abs(b))
    # finite differences along the retraction: f(R(tV)) = f + t <g,V> + t^2/2 <V,HV> + O(t^3)
    vn = np.linalg.norm(Vt.numpy())
    Vu = Vt.numpy() / vn
    t = 1e-4
    fp = prob.objective(ctx.stiefel_retract(n, p, X, ctx.upload(t * Vu)))
    fm = prob.objective(ctx.stiefel_retract(n, p, X, ctx.upload(-t * Vu)))
    gV, VHV = g.dot(Vt) / vn, Vt.dot(Hv) / vn ** 2
    assert abs((fp - fm) / (2 * t) - gV) <= 1e-6 * max(1.0, abs(gV))
    assert abs((fp - 2 * f + fm) / (t * t) - VHV) <= 1e-4 * max(1.0, abs(VHV))
    oracle.free(oprob)


@pytest.mark.parametrize("p", TALL_P)
def test_tall_rows_stpcg_two_pass_with_fused_dots_vs_oracle(oracle, p):
    """STPCG on rows of 9 ... 16 doubles: the two-pass Hessian through mi_op::apply_dots (the one-pass form does not exist
    for these widths: stiefel_hess_fused is never launched, the finish pass with the three dots is) against the oracle --
    counts, exit reason, alpha / beta traces, the step to 1e-10, interior and boundary exits -- with the settings of
    test_wide_rows_one_pass_hessian_matches_two_pass_and_oracle."""
    from optimization_amd import capi
    nx, ny, nz = 19, 14, 11          # 2926 rows: 46 slices, ragged last one
    n = nx * ny * nz
    rowptr, col, val = wl.laplacian_3d(nx, ny, nz)
    Xb, _ = wl.stiefel_bench_iterate(nx, ny, nz, p, eps=1e-2, seed=11 + p)
    oprob = oracle.stiefel_rq(n, p, rowptr, col, val)
    go = oracle.eval_grad(oprob, Xb.ravel())
    o = oracle.stpcg_problem(oprob, Xb.ravel(), go, 1e3, max_iterations=40, kappa_fgr=1e-8, theta=1.0, trace_cap=64)
    ob = oracle.stpcg_problem(oprob, Xb.ravel(), go, 1e-3, max_iterations=40, kappa_fgr=1e-8, theta=1.0)  # boundary exit
    oracle.free(oprob)
    c = capi.Context(0)
    try:
        A = c.csr(n, rowptr, col, val)
        prob = c.stiefel_rq(A, n, p)
        g, H = prob.model(c.upload(Xb))
        names = ("stiefel_hess_fused", "stiefel_finish_dots")
        for k in names:
            c.ktime_enable(k, True)
        c.ktime_reset()
        r = c.stpcg(g, H, Delta=1e3, max_iterations=40, kappa_fgr=1e-8, theta=1.0, trace_cap=64)
        launches = {k: c.ktime_read(k)[0] for k in names}
        rb = c.stpcg(g, H, Delta=1e-3, max_iterations=40, kappa_fgr=1e-8, theta=1.0)
        s, sb = r["s"].numpy().copy(), rb["s"].numpy().copy()
    finally:
        c.close()
    assert launches["stiefel_hess_fused"] == 0 and launches["stiefel_finish_dots"] >= 1, launches
    assert r["iterations"] == o["iterations"] and r["exit_reason"] == o["exit_reason"]
    assert np.allclose(r["trace"]["alpha"], o["trace"]["alpha"], rtol=1e-9)
    assert np.allclose(r["trace"]["beta"], o["trace"]["beta"], rtol=1e-8)
    print(f"p = {p}: step {rel_err(s, o['s']):.2e}, boundary step {rel_err(sb, ob['s']):.2e}")
    assert rel_err(s, o["s"]) < 1e-10
    assert (rb["iterations"], rb["exit_reason"]) == (ob["iterations"], ob["exit_reason"])
    assert rel_err(sb, ob["s"]) < 1e-10 and abs(rb["M_norm"] - ob["M_norm"]) <= 1e-12 * ob["M_norm"]


def test_tall_rows_preconditioned_stpcg_vs_oracle(ctx, oracle):
    """The problem's own tangent-space preconditioner P_X(D^-1 r) at p = 12 (row-scaled Gram pass + finish pass of the
    tall family) against the oracle's preconditioned solve, as test_wide_rows_preconditioned_and_sharded_slot_forms
    does for p = 6, 8."""
    nx, ny, nz, p = 12, 11, 10, 12
    n = nx * ny * nz
    rowptr, col, val = wl.laplacian_3d(nx, ny, nz)
    Xb, _ = wl.stiefel_bench_iterate(nx, ny, nz, p, eps=1e-2, seed=5)
    A = ctx.csr(n, rowptr, col, val)
    prob = ctx.stiefel_rq(A, n, p)
    diag = np.array([val[rowptr[i]:rowptr[i + 1]][col[rowptr[i]:rowptr[i + 1]] == i][0] for i in range(n)])
    dinv = 1.0 / (diag * np.linspace(0.5, 2.0, n))
    oprob = oracle.stiefel_rq(n, p, rowptr, col, val, dinv=dinv)
    go = oracle.eval_grad(oprob, Xb.ravel())
    Xd = ctx.upload(Xb)
    g, H = prob.model(Xd)
    P = prob.precon(Xd, ctx.upload(dinv))
    assert rel_err(P.apply(g).numpy(), oracle.eval_precon(oprob, Xb.ravel(), go)) < 1e-12
    rp = ctx.stpcg(g, H, P, Delta=1e3, max_iterations=40, kappa_fgr=1e-4, trace_cap=64)
    op = oracle.stpcg_problem(oprob, Xb.ravel(), go, 1e3, max_iterations=40, kappa_fgr=1e-4, trace_cap=64)
    oracle.free(oprob)
    assert rp["iterations"] == op["iterations"] and rp["exit_reason"] == op["exit_reason"]
    assert np.allclose(rp["trace"]["alpha"], op["trace"]["alpha"], rtol=1e-9)
    assert rel_err(rp["s"].numpy(), op["s"]) < 1e-9


@pytest.mark.parametrize("p", [9, 16])
def test_tall_rows_fused_trial_steps_have_the_bits_of_the_separate_calls(ctx, p):
    """mi_stiefel_rq_trial and mi_stiefel_rq_armijo_trial at p = 9 and 16 against the separate calls they replace, bit
    for bit (test_fused_trial_step_has_the_bits_of_the_separate_calls), each with one read-back."""
    from optimization_amd import capi
    nx, ny, nz = 20, 17, 13
    n = nx * ny * nz
    rowptr, col, val = wl.laplacian_3d(nx, ny, nz)
    A = ctx.csr(n, rowptr, col, val)
    prob = ctx.stiefel_rq(A, n, p)
    X = ctx.upload(wl.random_stiefel(n, p, seed=3))
    g, H = prob.model(X)
    h = ctx.stiefel_project(n, p, X, ctx.upload(np.random.default_rng(4).normal(size=(n, p)) * 1e-2))
    Hh = H.apply(h)
    hh, gh, hHh = ctx.dot_batch([h, g, h], [h, h, Hh])
    Xt_ref = ctx.stiefel_retract(n, p, X, h)
    f_ref = prob.objective(Xt_ref)
    syncs = ctx.sync_count()
    Xt, t = prob.trial(X, h, g)
    assert ctx.sync_count() - syncs == 1
    assert np.array_equal(Xt.numpy(), Xt_ref.numpy())
    assert (t["f"], t["hh"], t["gh"], t["hHh"]) == (f_ref, hh, gh, hHh)
    g2, H2 = prob.model(Xt)          # takes A X+, S+ and the gradient from the trial call
    prob2 = ctx.stiefel_rq(A, n, p)
    g2_ref, H2_ref = prob2.model(Xt_ref)
    assert np.array_equal(g2.numpy(), g2_ref.numpy())
    assert t["grad_sqnorm"] == g2_ref.dot(g2_ref)
    v = ctx.upload(np.random.default_rng(5).normal(size=(n, p)))
    assert np.array_equal(H2.apply(v).numpy(), H2_ref.apply(v).numpy())
    r1 = ctx.stpcg(g2, H2, Delta=10.0, max_iterations=8, kappa_fgr=1e-10, theta=1.0)
    r2 = ctx.stpcg(g2_ref, H2_ref, Delta=10.0, max_iterations=8, kappa_fgr=1e-10, theta=1.0)
    assert np.array_equal(r1["s"].numpy(), r2["s"].numpy())
    # the Armijo trial along -g at the same point: h = -t g, retraction, objective, gradient norm at the trial point
    g, H = prob.model(X)
    step = 1e-3
    hs = ctx.upload(-step * g.numpy())
    Xa_ref = ctx.stiefel_retract(n, p, X, hs)
    fa_ref = prob2.objective(Xa_ref)
    ga_ref, _ = prob2.model(Xa_ref)
    h_out, Xa, out = capi.Vec(ctx, n * p), capi.Vec(ctx, n * p), np.zeros(2)
    syncs = ctx.sync_count()
    capi.check(ctx.L.mi_stiefel_rq_armijo_trial(prob.h, X.h, g.h, C.c_double(step), h_out.h, Xa.h,
                                                 out.ctypes.data_as(C.POINTER(C.c_double))))
    assert ctx.sync_count() - syncs == 1
    assert np.array_equal(h_out.numpy(), hs.numpy())
    assert np.array_equal(Xa.numpy(), Xa_ref.numpy())
    assert (out[0], out[1]) == (fa_ref, ga_ref.dot(ga_ref))


def test_tall_rows_refusals(monkeypatch):
    """p = 17 and p = 0 are refused with a message that names the range; p = 12 on the multi-GPU code path of one rank
    (MI355OPT_FORCE_SLOT_PATH=1) with the one-context message: error codes, no launch."""
    from optimization_amd import capi
    nx, ny, nz = 6, 5, 4
    n = nx * ny * nz
    rowptr, col, val = wl.laplacian_3d(nx, ny, nz)
    c = capi.Context(0)
    try:
        A = c.csr(n, rowptr, col, val)
        for p in (17, 0):
            for call in (lambda: c.stiefel_rq(A, n, p), lambda: A.spmm(p, c.upload(np.zeros(n * max(p, 1)))),
                         lambda: c.stiefel_gram(n, p, c.upload(np.zeros(n * max(p, 1))), c.upload(np.zeros(n * max(p, 1))))):
                with pytest.raises(Exception, match=r"p must be in \[1,16\]"):
                    call()
    finally:
        c.close()
    monkeypatch.setenv("MI355OPT_FORCE_SLOT_PATH", "1")
    c = capi.Context(0)
    try:
        A = c.csr(n, rowptr, col, val)
        p = 12
        X = c.upload(wl.random_stiefel(n, p, seed=1))
        for call in (lambda: c.stiefel_rq(A, n, p), lambda: A.spmm(p, X), lambda: c.stiefel_gram(n, p, X, X),
                     lambda: c.stiefel_project(n, p, X, X), lambda: c.stiefel_retract(n, p, X, X)):
            with pytest.raises(Exception, match=r"rows of 9 \.\.\. 16 doubles run on one context"):
                call()
        assert c.stiefel_rq(A, n, 8) is not None   # (rows of up to 8 doubles run there as before)
    finally:
        c.close()
