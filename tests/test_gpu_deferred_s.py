"""The deferred-s form of the fused STPCG (stpcg.hip k_cg_pupdate_ds, switch DEFER_S): the single-context solve with the
flat direction kernel adds the step up every SECOND iteration, s = (s + alpha_k p_k) + alpha_k+1 p_k+1, from two
alternating direction buffers -- the same expressions in the same order as s += alpha p every iteration, so EVERY BIT of
the step, the scalars, the count, the exit and the traces must equal those of DEFER_S=0 (k_cg_pupdate every iteration),
compared here inside one process on one context.

Every way out of a solve has to add the pending term first, and which kernel does it depends on the parity of the
iteration the solve ends in: the test places the boundary exit, the negative-curvature exit, the kernel-of-H exit and the
residual exit each at an even and at an odd iteration (thresholds chosen between consecutive values of a host run of the
same recurrences), and FAILS if the set of (exit, parity) the device actually produced is not the full cross product."""
import numpy as np
import pytest

from optimization_amd import capi, workloads as wl

pytestmark = pytest.mark.gpu

RESIDUAL, MAXIT, KERNEL, BOUNDARY = 0, 1, 2, 3


def _solve_both(c, make, launches=None, **kw):
    """the same solve with DEFER_S = 0 and 1 on one context; every result bit must agree.  make(c) -> (g, H, P)"""
    out = []
    for defer_s in (0, 1):
        c.set_option("DEFER_S", defer_s)
        g, H, P = make(c)
        c.ktime_reset()
        c.ktime_enable("cg_pupdate", True)
        r = c.stpcg(g, H, P, trace_cap=64, **kw)
        nl = c.ktime_read("cg_pupdate")[0]
        c.ktime_enable("cg_pupdate", False)
        out.append((r, r["s"].numpy().copy(), nl))
    (a, sa, la), (b, sb, lb) = out
    assert a["iterations"] == b["iterations"] and a["exit_reason"] == b["exit_reason"], (a, b)
    assert a["M_norm"] == b["M_norm"] and a["rv_final"] == b["rv_final"], (a, b)
    for key in ("alpha", "beta", "kappa", "rv"):
        assert np.array_equal(a["trace"][key], b["trace"][key]), key
    assert np.array_equal(sa, sb), "s differs in %d of %d elements" % (int((sa != sb).sum()), sa.size)
    assert np.isfinite(sa).all()
    # the direction kernel is launched once per enqueued iteration in either form.  The host stops enqueuing when it SEES
    # the exit, so only a solve that runs to its iteration limit has a count that does not depend on timing
    if a["exit_reason"] == MAXIT:
        assert la == lb == a["iterations"], (la, lb, a["iterations"])
    else:
        assert min(la, lb) >= a["iterations"] + (0 if a["exit_reason"] == RESIDUAL else 1), (la, lb, a["iterations"])
    if launches is not None:
        assert la == lb == launches
    return a, sa


# ----------------------------------------------------------------------------------------------
# host run of the recurrences for a diagonal operator: where the exits are, so that thresholds can be put BETWEEN the values
# of consecutive iterations (the device's roundings differ in the last bits; every threshold below keeps a wide margin)
# ----------------------------------------------------------------------------------------------
def _host_cg(g, D, iters):
    """unconstrained CG on diag(D), no preconditioner: per iteration k the curvature kappa_k relative to |p|^2, the ratio
    |Hp| / |p| of the kernel test, |s_k+1|^2 and <r_k+1, r_k+1>"""
    r, s = g.copy(), np.zeros_like(g)
    p, rv = -r, float(g @ g)
    rows = []
    for _ in range(iters):
        Hp = D * p
        kappa, pp = float(p @ Hp), float(p @ p)
        ratio = float(np.sqrt(Hp @ Hp) / np.sqrt(pp))
        if kappa <= 0:
            rows.append(dict(kappa=kappa / pp, ratio=ratio, s2=None, rv=None))
            break
        alpha = rv / kappa
        s = s + alpha * p
        r = r + alpha * Hp
        rv_new = float(r @ r)
        rows.append(dict(kappa=kappa / pp, ratio=ratio, s2=float(s @ s), rv=rv_new))
        p = -r + (rv_new / rv) * p
        rv = rv_new
    return rows


def _between(lo, hi):
    assert 0 < lo < hi and hi / lo > 1.0001, (lo, hi)  # room of 5e-5 on either side: the roundings differ by ~1e-15
    return float(np.sqrt(lo * hi))


N_DIAG = 20_001  # odd: the last element is the leader thread's


def _spd(seed=11, n=N_DIAG):
    rng = np.random.default_rng(seed)
    return rng.normal(size=n), rng.uniform(0.5, 4.0, size=n)


def _diag_make(g, D):
    return lambda c: (c.upload(g), c.op_diag(c.upload(D)), None)


@pytest.fixture(scope="module")
def dctx():
    c = capi.Context(0)
    yield c
    c.close()


def test_every_exit_at_an_even_and_at_an_odd_iteration(dctx):
    seen = set()

    def record(kind, r, k_exit):
        seen.add((kind, k_exit & 1))
        print(f"{kind}: exit in iteration {k_exit}, {r['iterations']} iterations counted, reason {r['exit_reason']}")

    g, D = _spd()
    rows = _host_cg(g, D, 12)
    # boundary exit (:347, |s_k+1|^2 > Delta^2) in iteration k: Delta between |s_k| and |s_k+1|
    for k in (1, 2, 3, 4):
        Delta = np.sqrt(_between(rows[k - 1]["s2"], rows[k]["s2"]))
        r, s = _solve_both(dctx, _diag_make(g, D), Delta=Delta, max_iterations=100, kappa_fgr=1e-12, theta=1.0)
        assert r["exit_reason"] == BOUNDARY and r["iterations"] == k and r["M_norm"] == Delta
        assert abs(np.linalg.norm(s) - Delta) < 1e-9 * Delta
        record("boundary", r, k)
    # residual exit (:290) decided by the B-step of iteration k: theta = 0 makes the target kappa_fgr |r_0|
    rv0 = float(g @ g)
    for k in (1, 2, 3, 4):
        kf = np.sqrt(_between(rows[k]["rv"], rows[k - 1]["rv"]) / rv0)
        r, s = _solve_both(dctx, _diag_make(g, D), Delta=1e9, max_iterations=100, kappa_fgr=kf, theta=0.0)
        assert r["exit_reason"] == RESIDUAL and r["iterations"] == k + 1
        record("residual", r, k)
    # negative curvature (:347, kappa <= 0): a few negative eigenvalues, found by CG after some iterations.  Candidates are
    # scanned on the host; one is used only if the sign of every curvature up to the exit is far from rounding
    found = {}
    for nneg in (1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597):
        for scale in (0.02, 0.1, 0.5, 2.0):
            D2 = D.copy()
            D2[:nneg] = -scale * D2[:nneg]
            rows2 = _host_cg(g, D2, 40)
            k = len(rows2) - 1
            if rows2[k]["s2"] is not None or k < 1 or k & 1 in found:
                continue
            if rows2[k]["kappa"] < -1e-3 and all(x["kappa"] > 1e-3 for x in rows2[:k]):
                found[k & 1] = (D2, k)
    assert set(found) == {0, 1}, "no negative-curvature exit at both parities among the candidates: %r" % sorted(found)
    for D2, k in found.values():
        r, s = _solve_both(dctx, _diag_make(g, D2), Delta=1e9, max_iterations=100, kappa_fgr=1e-12, theta=1.0)
        assert r["exit_reason"] == BOUNDARY and r["iterations"] == k and r["M_norm"] == 1e9
        record("negative_curvature", r, k)
    # kernel of H (:305): a null space that g reaches into keeps |p| up while |Hp| falls with the residual of the range;
    # a raised epsilon between the ratios of iterations k - 1 and k ends the solve in iteration k
    D0 = 0.05 * D  # (every ratio below 1: epsilon has to be)
    D0[::3] = 0.0
    rows0 = _host_cg(g, D0, 12)
    for k in (1, 2, 3, 4):
        eps = _between(rows0[k]["ratio"], min(x["ratio"] for x in rows0[:k]))
        assert eps < 1
        r, s = _solve_both(dctx, _diag_make(g, D0), Delta=1e9, max_iterations=100, kappa_fgr=1e-12, theta=1.0, epsilon=eps)
        assert r["exit_reason"] == KERNEL and r["iterations"] == k and r["M_norm"] == 1e9
        record("kernel", r, k)
    # exits before any direction kernel, and in the very first iteration
    r, _ = _solve_both(dctx, _diag_make(g, np.zeros_like(g)), Delta=7.0, max_iterations=10)
    assert r["exit_reason"] == KERNEL and r["iterations"] == 0
    record("kernel", r, 0)
    r, _ = _solve_both(dctx, _diag_make(g, D), Delta=1e-3, max_iterations=10)
    assert r["exit_reason"] == BOUNDARY and r["iterations"] == 0
    record("boundary", r, 0)
    r, s = _solve_both(dctx, _diag_make(g, D), Delta=1.0, max_iterations=0)
    assert r["iterations"] == 0 and not s.any()
    want = {(kind, par) for kind in ("boundary", "negative_curvature", "kernel", "residual") for par in (0, 1)}
    assert seen == want, "cases not reached: %r" % sorted(want - seen)


def _stiefel_make(nx, ny, nz, p):
    n = nx * ny * nz
    rowptr, col, val = wl.laplacian_3d(nx, ny, nz)
    Xb, _ = wl.stiefel_bench_iterate(nx, ny, nz, p, eps=1e-3, seed=7)
    state = {}

    def make(c):
        if state.get("ctx") is not c:  # (matrix, problem and model once per context: the option acts per solve)
            A = c.csr(n, rowptr, col, val)
            prob = c.stiefel_rq(A, n, p)
            g, H = prob.model(c.upload(Xb))
            state.update(ctx=c, keep=(A, prob), g=g, H=H)
        return state["g"], state["H"], None
    return make


LIMITS = (1, 2, 3, 4, 5, 24, 25, 26, 50, 51)  # both parities of the last iteration; a re-anchor at k = 25 on either side


@pytest.mark.parametrize("grid", [(24, 20, 16), (100, 100, 100)])
def test_bench_problem_at_every_iteration_limit(dctx, grid):
    """bench.py's solve (Stiefel(n,3) Rayleigh quotient on a 3-D Laplacian, Delta 1e3, kappa_fgr 1e-12, theta 1) at a
    reduced size and at N = 3e6"""
    make = _stiefel_make(*grid, 3)
    par = set()
    for limit in LIMITS:
        r, _ = _solve_both(dctx, make, launches=limit, Delta=1e3, max_iterations=limit, kappa_fgr=1e-12, theta=1.0)
        assert r["exit_reason"] == MAXIT and r["iterations"] == limit
        par.add((limit - 1) & 1)
    assert par == {0, 1}


@pytest.mark.parametrize("p", [1, 3, 4, 6, 8])
def test_stiefel_widths(dctx, p):
    make = _stiefel_make(24, 20, 16, p)
    for limit in (6, 7, 27, 28):
        r, _ = _solve_both(dctx, make, launches=limit, Delta=1e3, max_iterations=limit, kappa_fgr=1e-12, theta=1.0)
        assert r["exit_reason"] == MAXIT and r["iterations"] == limit
    # a boundary exit: the trust region a tenth of the unconstrained step of four iterations, whichever iteration that is
    r4, s4 = _solve_both(dctx, make, Delta=1e3, max_iterations=4, kappa_fgr=1e-12, theta=1.0)
    r, _ = _solve_both(dctx, make, Delta=0.1 * r4["M_norm"], max_iterations=40, kappa_fgr=1e-12, theta=1.0)
    assert r["exit_reason"] == BOUNDARY


@pytest.mark.parametrize("precon", ["none", "diag", "block3", "callback"])
@pytest.mark.parametrize("n", [30_000, 30_003])
def test_preconditioners_and_run_ahead(dctx, precon, n):
    rng = np.random.default_rng(n)
    g = rng.uniform(-1, 1, size=n)
    D = rng.uniform(1.0, 400.0, size=n)
    M = D * rng.uniform(0.5, 2.0, size=n)
    Minv = 1.0 / M
    blocks = rng.normal(size=(n // 3, 3, 3))
    Binv = np.linalg.inv(blocks @ np.transpose(blocks, (0, 2, 1)) + 3 * np.eye(3)[None]).reshape(-1)
    keep = []

    def make(c):
        G, H = c.upload(g), c.op_diag(c.upload(D))
        P = None
        if precon == "diag":
            P = c.precon_diag(c.upload(Minv))
        elif precon == "block3":
            P = c.precon_block3(c.upload(Binv))
        elif precon == "callback":
            dop = c.op_diag(c.upload(Minv))
            keep.append(dop)
            P = c.precon_callback(n, lambda r, v: dop.apply(r, v))
        return G, H, P

    for ra in (1, 3, 8):
        for limit in (4, 5, 30, 31):
            r, _ = _solve_both(dctx, make, launches=limit, Delta=1e9, max_iterations=limit, kappa_fgr=0.0, theta=1.0,
                               run_ahead=ra)
            assert r["exit_reason"] == MAXIT and r["iterations"] == limit
        # a residual exit and a boundary exit somewhere along the solve
        r, _ = _solve_both(dctx, make, Delta=1e9, max_iterations=3000, kappa_fgr=1e-3, theta=1.0, run_ahead=ra)
        assert r["exit_reason"] == RESIDUAL and r["iterations"] > 2
        rb, _ = _solve_both(dctx, make, Delta=0.5 * r["M_norm"], max_iterations=3000, kappa_fgr=1e-3, theta=1.0, run_ahead=ra)
        assert rb["exit_reason"] == BOUNDARY


def test_deferred_result_solve_then_read_of_the_step(dctx):
    """defer=True: the call returns without waiting; s_out is valid in stream order, the scalars come from stpcg_collect"""
    g, D = _spd(seed=4)
    out = []
    for limit in (6, 7):
        for defer_s in (0, 1):
            dctx.set_option("DEFER_S", defer_s)
            G, H = dctx.upload(g), dctx.op_diag(dctx.upload(D))
            r = dctx.stpcg(G, H, Delta=1e9, max_iterations=limit, kappa_fgr=1e-14, theta=1.0, defer=True)
            res = dctx.stpcg_collect()
            out.append((res["iterations"], res["exit_reason"], res["M_norm"], res["rv_final"], r["s"].numpy().copy()))
        a, b = out[-2:]
        assert a[:4] == b[:4] and a[0] == limit
        assert np.array_equal(a[4], b[4])
