"""The LDS-window form of the sparse kernels (sparse.hip build_window, spmm_core.h sell_window) beyond the 7-point
stencil: the matrix families of window_cases.py, each of which takes another branch of what the host decides at
creation -- a window of 2 and of 4 chunks, 8 entries per row, far columns that are loaded because the far structure is
not pure (with both far entries on one side of the row), 0.0 appended behind the value table, the table sizes at which
the 16-bit words and the window itself stop -- through every kernel that consumes the form:

  (a) k_st_hess_fused in its window form, p = 1, 2, 3        test_window_hessian_*
  (b) k_st_hess_widewin, p = 4 ... 7 (8 on request)           test_wide_window_hessian_*
  (c) k_spmm_colmajor_win and k_spmm_colmajor_sweep           test_panel_product_*
  (d) the row-major product on the images the above start from   test_row_major_product_*

Every test first asserts that the matrix got the form its family is named for (mi_debug_csr_window_info,
mi_debug_csr_format_info against the family's `expect`) and names the kernel form the solve's plan selects
(mi_debug_stiefel_hess_form on those facts): none passes by quietly taking the streaming form.  References: the CPU
oracle for the solves, a longdouble row-by-row product for the products."""
import numpy as np
import pytest

import window_cases as wcs
from conftest import rel_err
from optimization_amd import workloads as wl

pytestmark = pytest.mark.gpu

PLAIN, WINDOW, WIDEWIN, WIDE, WIDEQ = range(5)   # stiefel.hip StHessForm
SWITCHES = ("MI355OPT_NO_WINDOW", "MI355OPT_NO_WIN_BOUNDS", "MI355OPT_NO_FAR_COMPUTED", "MI355OPT_WORDS16",
            "MI355OPT_NO_DIRGRAM", "MI355OPT_WIDE_WINDOW")
MODES = {"default": {}, "stream": {"MI355OPT_NO_WINDOW": "1"}, "equal-runs": {"MI355OPT_NO_WIN_BOUNDS": "1"},
         "loaded-far": {"MI355OPT_NO_FAR_COMPUTED": "1"}, "words16": {"MI355OPT_WORDS16": "1"},
         "two-pass": {"MI355OPT_NO_DIRGRAM": "1"}}
NUM_CU = 256


def _record(**kw):
    print("  ".join(f"{k}={v:.2e}" if isinstance(v, float) else f"{k}={v}" for k, v in kw.items()))


def _assert_format(A, e):
    """the library decided what the family's expect says (and so did the restatement in test_cpu_window_cases.py)"""
    info, fmt = A.window_info(), A.format_info()
    assert fmt["packed"] == e.packed
    if not e.packed:
        assert info[0] == 0 and not fmt["wk16"]
        return info, fmt
    assert fmt["ntable"] == e.ntable and fmt["zidx"] == e.zidx and fmt["wk16"] == e.wk16
    assert info[0] == e.wc and info[3] == 0
    if e.wc:
        assert info[1] == e.head and info[2] == e.pure_D and fmt["far_stride"] == e.far_stride
    return info, fmt


def _plan(capi, p, e, env):
    """the launch plan of the one-pass Hessian on a matrix with these facts under these switches: (form, HW, FAR)"""
    T = (int(e.packed), int(e.wc > 0), int(e.wk16), e.wc, e.head, e.pure_D, e.far_stride, 0, 0)
    S = (int(env.get("MI355OPT_NO_WINDOW", "0")), int(env.get("MI355OPT_NO_FAR_COMPUTED", "0")),
         int(env.get("MI355OPT_WORDS16", "0")), -1, int(env.get("MI355OPT_WIDE_WINDOW", "-1")),
         int(env.get("MI355OPT_NO_WIN_BOUNDS", "0")), 0, 0, 0)
    out = capi.stiefel_hess_form(p, -1, T, S)
    assert out is not None
    return out[0], out[5], out[6]


def _same_runs(capi, n, e):
    """the planned runs (cut to the far stride) are the equal runs, for every workgroup budget a window kernel asks with"""
    ntiles = ((n + 63) // 64 + 3) // 4
    return all(np.array_equal(capi.window_runs(ntiles, w, NUM_CU, e.far_stride), capi.window_runs(ntiles, w, NUM_CU, 0))
               for w in (NUM_CU, 2 * NUM_CU, 3 * NUM_CU, 4 * NUM_CU))


def _solves(oracle, monkeypatch, name, p, extra_env=None):
    """STPCG (unpreconditioned: the one-pass Hessian in its recurrence form) under every switch of MODES, a fresh context
    each, the oracle's gradient as the solve's input: from a random point of St(n, p) with Delta = 0.5, 1 and 6
    iterations -- there the Hessian is indefinite and the oracle leaves for the boundary in iteration 0 or 1, so the
    Hessian pass decides a branch but hardly enters the step -- and ("deep") from a point next to the minimiser with
    Delta = 1e6, where the oracle completes 6 iterations and every one of the 7 Hessian products shapes the step.
    Every mode against the oracle here; the caller compares the modes."""
    from optimization_amd import capi
    n, rowptr, col, val, e = wcs.case(name)
    X0 = wl.random_stiefel(n, p, seed=n + p)
    oprob = oracle.stiefel_rq(n, p, rowptr, col, val)
    go = oracle.eval_grad(oprob, X0.ravel())
    ref = {m: oracle.stpcg_problem(oprob, X0.ravel(), go, 0.5, max_iterations=m, trace_cap=8) for m in (1, 6)}
    X1 = wcs.near_minimiser(name, p)
    go1 = oracle.eval_grad(oprob, X1.ravel())
    deep = oracle.stpcg_problem(oprob, X1.ravel(), go1, 1e6, max_iterations=6, kappa_fgr=1e-10, theta=1.0, trace_cap=8)
    assert deep["iterations"] == 6   # (the point is what it is meant to be)
    oracle.free(oprob)
    res, worst = {}, 0.0
    for mode, env in MODES.items():
        env = dict(env, **(extra_env or {}))
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        c = capi.Context(0)
        try:
            A = c.csr(n, rowptr, col, val)
            _assert_format(A, e)
            prob = c.stiefel_rq(A, n, p)
            g, H = prob.model(c.upload(X0))
            assert rel_err(g.numpy(), go) < 1e-11
            c.ktime_enable("stiefel_hess_fused", True)
            c.ktime_reset()
            out = {"plan": _plan(capi, p, e, env)}
            for maxit, o in ref.items():
                r = c.stpcg(c.upload(go), H, Delta=0.5, max_iterations=maxit, trace_cap=8)
                s = r["s"].numpy().copy()
                assert (r["iterations"], r["exit_reason"]) == (o["iterations"], o["exit_reason"]), (mode, maxit)
                err = rel_err(s, o["s"])
                worst = max(worst, err)
                assert err < 1e-10, (mode, maxit, err)   # BASELINE.json: iterate match within 1e-10 relative
                out[maxit] = (s, r["iterations"], r["exit_reason"], r["M_norm"])
            g1, H1 = prob.model(c.upload(X1))
            r = c.stpcg(c.upload(go1), H1, Delta=1e6, max_iterations=6, kappa_fgr=1e-10, theta=1.0, trace_cap=8)
            s = r["s"].numpy().copy()
            assert (r["iterations"], r["exit_reason"]) == (deep["iterations"], deep["exit_reason"]), (mode, "deep")
            assert np.allclose(r["trace"]["alpha"], deep["trace"]["alpha"], rtol=1e-9), (mode, "deep")
            err = rel_err(s, deep["s"])
            worst = max(worst, err)
            assert err < 1e-10, (mode, "deep", err)
            out["deep"] = (s, r["iterations"], r["exit_reason"], r["M_norm"])
            out["launches"] = c.ktime_read("stiefel_hess_fused")[0]
            res[mode] = out
        finally:
            c.close()
    # the one-pass kernel ran wherever it was not switched off
    assert all((r["launches"] > 0) == (mode != "two-pass") for mode, r in res.items())
    return n, e, res, worst


def _compare_modes(capi, name, p, n, e, res, worst):
    d, st = res["default"], res["stream"]
    gap = 0.0
    for maxit in (1, 6, "deep"):
        scale = np.abs(st[maxit][0]).max()
        for mode in ("default", "equal-runs", "loaded-far", "words16", "two-pass"):
            gap = max(gap, np.abs(res[mode][maxit][0] - st[maxit][0]).max() / scale)
            # every output row is formed by the same products and sums in the same order; the forms partition the rows
            # into per-workgroup partial sums differently: the replicated scalars agree to rounding
            assert np.abs(res[mode][maxit][0] - st[maxit][0]).max() <= 1e-11 * scale, (mode, maxit)
        # far columns computed or loaded, 16-bit or 32-bit words: the same kernel otherwise and the same row partition
        # (the runs are cut by win_far_stride, which neither switch touches)
        for mode in ("loaded-far", "words16"):
            assert np.array_equal(d[maxit][0], res[mode][maxit][0]) and d[maxit][1:] == res[mode][maxit][1:], (mode, maxit)
        if e.far_stride == 0 or _same_runs(capi, n, e):
            assert np.array_equal(d[maxit][0], res["equal-runs"][maxit][0]), maxit
    _record(test="hessian", family=name, p=p, default_form=str(d["plan"]), words16_form=str(res["words16"]["plan"]),
            loaded_far_form=str(res["loaded-far"]["plan"]), stream_form=str(st["plan"]), vs_oracle=float(worst),
            vs_stream=float(gap), bars="1e-10 / 1e-11")


@pytest.mark.parametrize("p", [1, 2, 3])
@pytest.mark.parametrize("name", wcs.WINDOWED)
def test_window_hessian_p_le_3_vs_oracle_and_streaming_form(oracle, monkeypatch, name, p):
    """(a) k_st_hess_fused<P, ., ., ., ., HW, FAR> in its window form: HW = 7 and 8, rings of 10, 12 and 16 chunks (wc =
    1, 2, 4), far columns computed (FAR = 1; with 16-bit words FAR = 2) on the pure families and loaded (FAR = 0) on
    the others, 0.0 at its place in the table or appended behind it."""
    from optimization_amd import capi
    n, e, res, worst = _solves(oracle, monkeypatch, name, p)
    hw, pure = 7 if e.head <= 7 else 8, e.pure_D > 0
    assert res["default"]["plan"] == (WINDOW, hw, 1 if pure else 0)
    assert res["equal-runs"]["plan"] == res["default"]["plan"]
    assert res["loaded-far"]["plan"] == (WINDOW, hw, 0)
    # 16-bit words: only where the far columns are computed and the words exist (<= 32 table entries); elsewhere the
    # switch must leave the 32-bit words' kernel -- and, below, its bits
    assert res["words16"]["plan"] == (WINDOW, hw, 2 if pure and e.wk16 else 1 if pure else 0)
    assert res["stream"]["plan"] == (PLAIN, 0, 0)
    _compare_modes(capi, name, p, n, e, res, worst)


@pytest.mark.parametrize("name", ["third_far", "circ_full_256", "circ_full_257"])
def test_window_hessian_matrices_without_a_window_keep_the_streaming_form(oracle, monkeypatch, name):
    """a third far entry in one row, a full value table without 0.0, a matrix that is not packed at all: no window form,
    the switches change nothing, not a bit"""
    from optimization_amd import capi
    n, e, res, worst = _solves(oracle, monkeypatch, name, 3)
    assert e.wc == 0 and all(r["plan"] == (PLAIN, 0, 0) for r in res.values())
    for maxit in (1, 6, "deep"):
        for mode in ("stream", "equal-runs", "loaded-far", "words16"):
            assert np.array_equal(res["default"][maxit][0], res[mode][maxit][0]), (mode, maxit)
    _compare_modes(capi, name, 3, n, e, res, worst)


B_FAMILIES = ["band_wc2", "matchings", "stencil_head8", "band_wc4", "two_offset_pure", "band_wc2_pure",
              "band_wc2_pure_head8"]


@pytest.mark.parametrize("p", [4, 5, 7])
@pytest.mark.parametrize("name", B_FAMILIES)
def test_wide_window_hessian_vs_oracle_and_streaming_form(oracle, monkeypatch, name, p):
    """(b) k_st_hess_widewin<P, HW, FARD>: rings of 10 and 12 chunks with padded rows, far rows gathered (loaded columns)
    or read as coalesced images at slice +- D (computed: D a multiple of 64 on the stencil, 300 and 1000 elsewhere).  A
    window of four chunks has no wide form: band_wc4 must fall back and the window switch change nothing."""
    from optimization_amd import capi
    n, e, res, worst = _solves(oracle, monkeypatch, name, p)
    hw, pure = 7 if e.head <= 7 else 8, e.pure_D > 0
    if e.wc <= 2:
        assert res["default"]["plan"] == (WIDEWIN, hw, 1 if pure else 0)
        assert res["loaded-far"]["plan"] == (WIDEWIN, hw, 0)
        assert res["words16"]["plan"] == res["equal-runs"]["plan"] == res["default"]["plan"]
        assert res["stream"]["plan"][0] in ((PLAIN,) if p == 4 else (WIDE, WIDEQ))
    else:
        assert res["default"]["plan"] == res["stream"]["plan"] and res["default"]["plan"][0] in (PLAIN, WIDE, WIDEQ)
        for maxit in (1, 6, "deep"):
            assert np.array_equal(res["default"][maxit][0], res["stream"][maxit][0]), maxit
    _compare_modes(capi, name, p, n, e, res, worst)


def test_wide_window_hessian_p8_on_request(oracle, monkeypatch):
    """p = 8 takes the window form only with MI355OPT_WIDE_WINDOW=1 (rows padded to 9 doubles in the ring); here with 8
    entries per row"""
    from optimization_amd import capi
    n, e, res, worst = _solves(oracle, monkeypatch, "stencil_head8", 8, {"MI355OPT_WIDE_WINDOW": "1"})
    assert res["default"]["plan"] == (WIDEWIN, 8, 1) and res["loaded-far"]["plan"] == (WIDEWIN, 8, 0)
    assert res["stream"]["plan"][0] in (WIDE, WIDEQ)
    _compare_modes(capi, "stencil_head8", 8, n, e, res, worst)


# ------------------------------------------------------------------------------------------------------------------
# products against a longdouble reference
# ------------------------------------------------------------------------------------------------------------------
_PANELS = {}


def _panel(name):
    """24 columns and their longdouble product, once per family"""
    if name not in _PANELS:
        n, rowptr, col, val, e = wcs.case(name)
        X = np.random.default_rng(n + 24).normal(size=(n, 24))
        ref, absref = wcs.spmm_ld(rowptr, col, val, X)
        theta = np.random.default_rng(n).uniform(0.5, 2.0, size=24)
        for a in (X, ref, absref, theta):
            a.setflags(write=False)
        _PANELS[name] = (X, ref, absref, theta)
    return _PANELS[name]


def _margin(Y, ref, bound):
    """max over the elements of |Y - ref| / bound (elements whose bound is 0 must be exact)"""
    err = np.abs(Y.astype(wcs.LD) - ref).astype(np.float64)
    assert (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max())


@pytest.mark.parametrize("k", [3, 8, 9, 24])
@pytest.mark.parametrize("name", wcs.ALL)
def test_panel_product_window_gather_and_loaded_far_vs_longdouble(ctx, name, k):
    """(c) mi_csr_spmm_colmajor and its fused residual form on every family: k_spmm_colmajor_win<8, HW, WC, FARD, RES>
    where the matrix has a window of one or two chunks -- which instantiation is recorded -- against the gather form
    (NO_SPMM_WIN=1) and the loaded far columns (NO_FAR_COMPUTED=1) bit for bit, and against the longdouble product
    within the bound of a sum of <= head rounded products.  Panels of 3, 8, 9 and 24 columns: less than a pass of 8
    columns, one, one and a column, three."""
    n, rowptr, col, val, e = wcs.case(name)
    X24, ref24, abs24, theta24 = _panel(name)
    X, ref, absref, theta = X24[:, :k], ref24[:, :k], abs24[:, :k], theta24[:k]
    A = ctx.csr(n, rowptr, col, val)
    _assert_format(A, e)
    Xd = ctx.upload(np.asfortranarray(X).ravel(order="F"))
    mat = lambda v: np.array(v.numpy(), copy=True).reshape(k, n).T   # noqa: E731
    out = {}
    ctx.ktime_enable("csr_spmm", True)
    try:
        for mode, opts in (("window", {}), ("loaded-far", {"NO_FAR_COMPUTED": 1}), ("gather", {"NO_SPMM_WIN": 1})):
            ctx.set_option("NO_FAR_COMPUTED", 0).set_option("NO_SPMM_WIN", 0).set_option("NO_SPMM_SWEEP", 1)
            for o, v in opts.items():
                ctx.set_option(o, v)
            ctx.ktime_reset()
            Y = mat(A.spmm_colmajor(k, Xd))
            AX, R, rn, xn = A.spmm_colmajor_residual(k, Xd, theta)
            out[mode] = (Y, mat(AX), mat(R), np.array(rn, copy=True), np.array(xn, copy=True))
            assert ctx.ktime_read("csr_spmm")[0] >= 2
    finally:
        ctx.set_option("NO_FAR_COMPUTED", 0).set_option("NO_SPMM_WIN", 0).set_option("NO_SPMM_SWEEP", 1)
        ctx.ktime_enable("csr_spmm", False)
    Y, AX, R, rn, xn = out["window"]
    for mode in ("loaded-far", "gather"):
        for a, b in zip(out["window"][:3], out[mode][:3]):
            assert np.array_equal(a, b), mode
        # the column sums are grouped by workgroup: to rounding between the forms (the bar of the existing panel tests)
        assert np.allclose(rn, out[mode][3], rtol=1e-13) and np.allclose(xn, out[mode][4], rtol=1e-13), mode
    assert np.array_equal(Y, AX)
    head = int(np.diff(rowptr).max())
    m_y = _margin(Y, ref, wcs.sum_bound(head, absref))
    assert m_y <= 1.0
    # R = AX - X diag(theta) from the device's own AX: one rounding of the product (none if fused), one of the difference
    xt = X.astype(wcs.LD) * theta.astype(wcs.LD)
    r_ref = AX.astype(wcs.LD) - xt
    m_r = _margin(R, r_ref, (2.0 ** -53 * (1 + 2.0 ** -50) * (np.abs(xt) + np.abs(r_ref))).astype(np.float64))
    assert m_r <= 1.0
    assert np.allclose(rn, np.linalg.norm(R, axis=0), rtol=1e-12) and np.allclose(xn, np.linalg.norm(X, axis=0), rtol=1e-12)
    inst = "gather"
    if 0 < e.wc <= 2:
        hw = 7 if e.head <= 7 else 8
        inst = (f"win<8,{hw},{e.wc},{'T' if e.pure_D else 'F'},F/T> (default), win<8,{hw},{e.wc},F,F/T> (loaded far)")
    _record(test="panel", family=name, k=k, kernels=inst, product_over_bound=m_y, residual_over_bound=m_r)


@pytest.mark.parametrize("k", [3, 8, 9, 24])
def test_panel_product_plane_sweep_on_eight_entries_per_row(ctx, k):
    """(c) the opt-in plane-sweep form (NO_SPMM_SWEEP=0, k_spmm_colmajor_sweep<8, 8, RES>) on stencil_head8 -- pure far
    stride 1600 >= 2 * 512 rows, 8 entries per row -- bit for bit against the window form and within the bound of the
    longdouble product.  (The per-kernel timer counts the product, whichever form runs: that the sweep applies follows
    from the facts asserted first -- packed, a window of <= 2 chunks, head <= 8, pure D >= 1024 -- which are
    spmm_sweep_ok's conditions.)"""
    name = "stencil_head8"
    n, rowptr, col, val, e = wcs.case(name)
    X24, ref24, abs24, theta24 = _panel(name)
    X, ref, absref, theta = X24[:, :k], ref24[:, :k], abs24[:, :k], theta24[:k]
    A = ctx.csr(n, rowptr, col, val)
    info, fmt = _assert_format(A, e)
    assert fmt["packed"] and 0 < info[0] <= 2 and info[1] <= 8 and info[2] >= 2 * 512
    Xd = ctx.upload(np.asfortranarray(X).ravel(order="F"))
    mat = lambda v: np.array(v.numpy(), copy=True).reshape(k, n).T   # noqa: E731
    out = {}
    ctx.ktime_enable("csr_spmm", True)
    try:
        for mode, off in (("window", 1), ("sweep", 0)):
            ctx.set_option("NO_SPMM_SWEEP", off)
            ctx.ktime_reset()
            Y = mat(A.spmm_colmajor(k, Xd))
            AX, R, rn, xn = A.spmm_colmajor_residual(k, Xd, theta)
            out[mode] = (Y, mat(AX), mat(R), np.array(rn, copy=True), np.array(xn, copy=True))
            assert ctx.ktime_read("csr_spmm")[0] >= 2
    finally:
        ctx.set_option("NO_SPMM_SWEEP", 1)
        ctx.ktime_enable("csr_spmm", False)
    for a, b in zip(out["window"][:3], out["sweep"][:3]):
        assert np.array_equal(a, b)
    assert np.allclose(out["window"][3], out["sweep"][3], rtol=1e-13)
    assert np.allclose(out["window"][4], out["sweep"][4], rtol=1e-13)
    m_y = _margin(out["sweep"][0], ref, wcs.sum_bound(8, absref))
    assert m_y <= 1.0
    _record(test="sweep", family=name, k=k, product_over_bound=m_y)


def test_panel_product_short_far_stride_does_not_take_the_plane_sweep(ctx):
    """two_offset_pure (D = 300 < 2 * 512 rows): the sweep's tiles would overlap their own far rows; the switch must leave
    the window form -- the same bits, column sums included (the same kernel groups them the same way)"""
    n, rowptr, col, val, e = wcs.case("two_offset_pure")
    X24, ref24, abs24, theta24 = _panel("two_offset_pure")
    A = ctx.csr(n, rowptr, col, val)
    _assert_format(A, e)
    assert 0 < e.pure_D < 2 * 512
    Xd = ctx.upload(np.asfortranarray(X24[:, :9]).ravel(order="F"))
    out = {}
    try:
        for off in (1, 0):
            ctx.set_option("NO_SPMM_SWEEP", off)
            AX, R, rn, xn = A.spmm_colmajor_residual(9, Xd, theta24[:9])
            out[off] = (AX.numpy().copy(), R.numpy().copy(), np.array(rn, copy=True), np.array(xn, copy=True))
    finally:
        ctx.set_option("NO_SPMM_SWEEP", 1)
    assert all(np.array_equal(a, b) for a, b in zip(out[0], out[1]))
    m = _margin(out[0][0].reshape(9, n).T, ref24[:, :9], wcs.sum_bound(e.head, abs24[:, :9]))
    assert m <= 1.0


@pytest.mark.parametrize("p", [1, 3, 8])
@pytest.mark.parametrize("name", ["circ_full", "third_far"])
def test_row_major_product_vs_longdouble(ctx, name, p):
    """(d) mi_csr_spmm (sell_stream on the packed copy) on the image without any padding (circ_full: 90 full slices of
    one width, no 0.0 in the table) and on the matrix that was refused a window, against the longdouble product"""
    n, rowptr, col, val, e = wcs.case(name)
    X24, ref24, abs24, _ = _panel(name)
    A = ctx.csr(n, rowptr, col, val)
    _assert_format(A, e)
    W = A.spmm(p, ctx.upload(np.ascontiguousarray(X24[:, :p]))).numpy().reshape(n, p)
    m = _margin(W, ref24[:, :p], wcs.sum_bound(int(np.diff(rowptr).max()), abs24[:, :p]))
    assert m <= 1.0
    _record(test="row-major", family=name, p=p, product_over_bound=m)
