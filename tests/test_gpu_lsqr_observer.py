"""The reference's LSQR user function (IterativeSolvers.h:450-456, called at :845-851) on the fused solve: mi_lsqr_observed
through the C ABI (capi.Context.lsqr(observer=)) and through LinearAlgebra::LSQR on MI355::DeviceVector
(tests/cpp/harness_lsqr_observer.cpp).  Shapes: n = 1, n = 2*1024*3 + 1 (odd tail of the double2 walk, several
workgroups) and n = 20 000; a built-in CSR operator (fused-SpMV kernel forms) and a callback operator (k_lsqr_u /
k_lsqr_v); plain, damped and trust-region-bounded solves."""
import numpy as np
import pytest

import lsqr_observer_py as lo

pytestmark = pytest.mark.gpu

SIZES = (1, 2 * 1024 * 3 + 1, 20_000)
KINDS = ("plain", "damped", "bounded")


def _kind(kind, n):
    """solver arguments of a kind at size n.  bounded: a radius that the QR-based |x| estimate of lsqr_observer_py's
    problem (0.253, 0.269, 0.270.. x sqrt(n) after passes 0, 1, 2..) crosses in pass 1 or 2 -- at least one observed pass,
    then the shortened step of :785-793 and the S4 exit"""
    return {"plain": dict(), "damped": dict(lam=0.3), "bounded": dict(Delta=0.2699 * float(np.sqrt(n)))}[kind]
RESULT = ("xnorm", "iterations", "exit_reason", "rbar_norm", "Arnorm", "Anorm", "Acond")
EXIT_USER = 6


@pytest.fixture(scope="module")
def ctx():
    from optimization_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def problems(ctx):
    """n -> (b on the device, {"csr": (A, At), "callback": (A, At)}), made once"""
    out = {}
    for n in SIZES:
        lo_, di, up, b = lo.tridiagonal(n)
        mats = [ctx.csr(n, *lo.tridiagonal_csr(lo_, di, up, t)) for t in (False, True)]
        cb = [ctx.op_callback(n, (lambda M: lambda vin, vout: M.spmm(1, vin, vout))(M)) for M in mats]
        for op in cb:
            op.n_in = n
        out[n] = (ctx.upload(b), {"csr": [ctx.op_csr(M, 1) for M in mats], "callback": cb})
    return out


def _recorder(stop_at=None):
    rec = []

    def observer(k, x, xnorm, rbar_norm, Arnorm, Anorm, Acond):
        rec.append((k, xnorm, rbar_norm, Arnorm, Anorm, Acond))
        return stop_at is not None and k == stop_at
    return rec, observer


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("op", ["csr", "callback"])
@pytest.mark.parametrize("n", SIZES)
def test_an_observer_that_never_stops_changes_nothing(ctx, problems, n, op, kind):
    b, ops = problems[n]
    A, At = ops[op]
    for extra in (dict(), dict(max_iterations=5)):
        kw = dict(_kind(kind, n), **extra)
        ref = ctx.lsqr(A, At, b, **kw)
        rec, observer = _recorder()
        obs = ctx.lsqr(A, At, b, observer=observer, **kw)
        assert np.array_equal(obs["x"].numpy(), ref["x"].numpy())
        for f in RESULT:
            assert obs[f] == ref[f], (f, obs[f], ref[f])
        # called once per pass that no stopping rule S1-S4 ended, with the loop index of the pass
        assert [r[0] for r in rec] == list(range(ref["iterations"])), (ref["iterations"], ref["exit_reason"])
        # operator_applications is exact for the observed solve (mi_lsqr's includes its run-ahead): A'b at the start and
        # two per enqueued pass -- the pass that a stopping rule ended was enqueued, num_iterations does not count it
        passes = {0: ref["iterations"], 5: None}.get(ref["exit_reason"], ref["iterations"] + 1)
        if passes is None:  # A'b = 0: over before the loop; the one pass the host may have enqueued by then does nothing
            assert obs["operator_applications"] in (1, 3)
        else:
            assert obs["operator_applications"] == 1 + 2 * passes, (obs["operator_applications"], passes)
        assert ref["operator_applications"] >= obs["operator_applications"] or ref["exit_reason"] == 5
        if ref["exit_reason"] == 0 and rec:  # MAXIT: the last call saw the final state
            assert rec[-1][1:] == tuple(ref[f] for f in ("xnorm", "rbar_norm", "Arnorm", "Anorm", "Acond"))
    if n > 1 and kind != "bounded":
        assert ref["exit_reason"] == 0 and len(rec) == 5
    if n > 1 and kind == "bounded":
        assert ref["exit_reason"] == 4 and len(rec) >= 1


@pytest.mark.parametrize("op", ["csr", "callback"])
@pytest.mark.parametrize("n", SIZES[1:])
def test_an_observer_that_stops_at_k(ctx, problems, n, op):
    b, ops = problems[n]
    A, At = ops[op]
    kw = dict(btol=1e-12, Atol=1e-12)
    free = ctx.lsqr(A, At, b, **kw)
    assert free["iterations"] > 8, free            # no stopping rule fires in the passes used below
    syncs = {}
    for k in (3, 5):
        ref = ctx.lsqr(A, At, b, max_iterations=k + 1, **kw)
        rec, observer = _recorder(stop_at=k)
        s0 = ctx.sync_count()
        r = ctx.lsqr(A, At, b, observer=observer, **kw)
        syncs[k] = ctx.sync_count() - s0
        assert np.array_equal(r["x"].numpy(), ref["x"].numpy())
        assert (r["iterations"], r["exit_reason"]) == (k, EXIT_USER)
        assert r["operator_applications"] == 1 + 2 * (k + 1)
        assert [q[0] for q in rec] == list(range(k + 1))
        assert r["xnorm"] == ref["xnorm"] == rec[-1][1]
        # ... and in the last pass allowed: still a break, the loop index is not advanced
        rec, observer = _recorder(stop_at=k)
        r = ctx.lsqr(A, At, b, observer=observer, max_iterations=k + 1, **kw)
        assert np.array_equal(r["x"].numpy(), ref["x"].numpy())
        assert (r["iterations"], r["exit_reason"]) == (k, EXIT_USER)
    print("host synchronisations of a solve stopped at k = 3, 5:", syncs)
    assert syncs[5] - syncs[3] == 2               # one per pass
    assert syncs[3] == 4 + 1                      # ... and the read-back of the result


def test_an_observer_that_raises(ctx, problems):
    b, ops = problems[SIZES[1]]
    A, At = ops["csr"]
    ref = ctx.lsqr(A, At, b)

    def observer(k, *_):
        if k == 2:
            raise KeyError("from the observer")
        return False
    with pytest.raises(KeyError):
        ctx.lsqr(A, At, b, observer=observer)
    again = ctx.lsqr(A, At, b)
    assert np.array_equal(again["x"].numpy(), ref["x"].numpy()) and again["iterations"] == ref["iterations"]


def test_the_observed_solve_declines_where_it_must():
    from optimization_amd import capi
    lo_, di, up, b = lo.tridiagonal(64)
    for option, word in (("NO_FUSED_LSQR_OBSERVER", "NO_FUSED_LSQR_OBSERVER"), ("FORCE_LOCKSTEP", "FORCE_LOCKSTEP")):
        c = capi.Context(0)
        try:
            assert c.lsqr_observer_available() == (True, "")
            c.set_option(option, 1)
            ok, why = c.lsqr_observer_available()
            assert not ok and word in why, why
            A, At = (c.op_csr(c.csr(64, *lo.tridiagonal_csr(lo_, di, up, t)), 1) for t in (False, True))
            before = c.fusion_counters()
            with pytest.raises(capi.MiError) as e:
                c.lsqr(A, At, c.upload(b), observer=lambda *a: False)
            assert e.value.status == 7 and c.fusion_counters() == before       # MI_DECLINED: nothing done or counted
        finally:
            c.close()


# ---- the template layer ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness():
    return lo.LsqrObserverHarness()


@pytest.mark.parametrize("pack", [0, 1], ids=["no_pack", "pack"])
@pytest.mark.parametrize("kind", KINDS)
def test_template_lsqr_with_a_user_function_is_fused(harness, kind, pack):
    """LA::LSQR<DeviceVector, ...> with a user function against the same template on the host vector (the reference's
    statement sequence): same calls, same k sequence, iterate to 1e-9; with NO_FUSED_LSQR_OBSERVER the generic loop gives
    the same counts"""
    n = SIZES[1]
    lo_, di, up, b = lo.tridiagonal(n)
    kw = dict(lam=_kind(kind, n).get("lam", 0.0), Delta=_kind(kind, n).get("Delta"))
    h = harness.tridiag(0, pack, lo_, di, up, b, **kw)
    d = harness.tridiag(1, pack, lo_, di, up, b, **kw)
    g = harness.tridiag(1, pack, lo_, di, up, b, no_fused=True, **kw)
    assert h["rc"] == 0 and d["rc"] == 0 and g["rc"] == 0, (h["err"], d["err"], g["err"])
    print(kind, "pack", pack, "calls", h["calls"], d["calls"], g["calls"], "syncs fused", d["syncs"], "generic", g["syncs"])
    assert (d["fused_lsqr_solves"], d["generic_lsqr_solves"]) == (1, 0)
    assert (g["fused_lsqr_solves"], g["generic_lsqr_solves"]) == (0, 1)
    for r in (d, g):
        assert (r["iterations"], r["calls"]) == (h["iterations"], h["calls"])
        assert np.array_equal(r["rec"][:, 0], h["rec"][:, 0])
        assert r["counter"] == (h["calls"] if pack else 0) == h["counter"]
        assert np.abs(r["x"] - h["x"]).max() <= 1e-9 * max(1.0, np.abs(h["x"]).max())
        assert np.allclose(r["rec"][:, 1:], h["rec"][:, 1:], rtol=1e-9, atol=0)
    if h["calls"] > 3:
        hs = harness.tridiag(0, pack, lo_, di, up, b, stop_at=2, **kw)
        ds = harness.tridiag(1, pack, lo_, di, up, b, stop_at=2, **kw)
        assert (ds["iterations"], ds["calls"], ds["counter"]) == (hs["iterations"], hs["calls"], hs["counter"])
        assert hs["iterations"] == 2 and hs["calls"] == 3
        assert np.abs(ds["x"] - hs["x"]).max() <= 1e-9 * max(1.0, np.abs(hs["x"]).max())


def test_template_user_function_that_throws(harness):
    n = SIZES[1]
    lo_, di, up, b = lo.tridiagonal(n)
    ref = harness.tridiag(1, 1, lo_, di, up, b)
    thr = harness.tridiag(1, 1, lo_, di, up, b, throw_at=2)
    assert thr["rc"] == -3, (thr["rc"], thr["err"])             # the exception reached the caller of LSQR
    # ... and the same solve on the same context afterwards gives its usual bits
    assert np.array_equal(thr["x"], ref["x"]) and (thr["iterations"], thr["calls"]) == (ref["iterations"], ref["calls"])
    assert thr["fused_lsqr_solves"] == 1
