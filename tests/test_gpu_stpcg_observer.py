"""The observed fused STPCG (mi_stpcg_observed; stpcg.hip k_cg_peek / k_cg_user_stop): the reference's STPCGUserFunction
(IterativeSolvers.h:50-59, called at :365-369) on the kernels of mi_stpcg.

Device against device, bit for bit (capi, one context): an observer that never stops changes nothing; a stop at k leaves
what the un-observed solve with max_iterations = k leaves; the views are the solve's own vectors; every exit of the
solve is taken as without an observer and the observer is not called in the exiting pass.

Against the reference's arithmetic (tests/cpp/harness_observer.cpp): ONE templated driver on the host vector (generic
loop, bit-identical to the reference) and on MI355::DeviceVector (the fused observed path) records what the user
function sees; the records agree to 1e-10.  The tolerances asked of the inner solve's depth there: kappa_fgr is chosen
where the HOST loop's own record moves by less than 1e-11 when its input moves by one ulp
(tests/test_cpu_observer_resources.py measures that on the CPU) -- 1e-3 without the preconditioner (25 passes), 0.5 with
the fixture's diagonal preconditioner (6 passes: from pass ~12 on that problem amplifies a last-bit change tenfold per
pass, the stagnation the existing fixture test speaks of)."""
import numpy as np
import pytest

from conftest import rel_err
from optimization_amd import capi, workloads as wl
from test_gpu_deferred_s import _between, _diag_make, _host_cg, _spd

pytestmark = pytest.mark.gpu

RESIDUAL, MAXIT, KERNEL, BOUNDARY, USER = 0, 1, 2, 3, 4
from observer_py import KAPPA_PLAIN, KAPPA_PRECON  # kappa_fgr of the host-against-device records (module docstring)


@pytest.fixture(scope="module")
def octx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def obs():
    import observer_py
    return observer_py.ObserverHarness()


def _bits_equal(a, sa, b, sb, traces=True):
    assert a["iterations"] == b["iterations"] and a["exit_reason"] == b["exit_reason"], (a, b)
    assert a["M_norm"] == b["M_norm"] and a["rv_final"] == b["rv_final"], (a, b)
    if traces:
        for key in ("alpha", "beta", "kappa", "rv"):
            assert np.array_equal(a["trace"][key], b["trace"][key]), key
    assert np.array_equal(sa, sb), "s differs in %d of %d elements" % (int((sa != sb).sum()), sa.size)


def _observed(c, g, H, P, stop_at=None, at=None, **kw):
    """solve with an observer that records (k, alpha), stops at stop_at and runs at(k, s, r, v, p) if given"""
    calls = []

    def observer(k, s, r, v, p, alpha):
        calls.append((k, alpha))
        if at is not None:
            at(k, s, r, v, p)
        return k == stop_at
    n0 = c.sync_count()
    r = c.stpcg(g, H, P, observer=observer, **kw)
    syncs = c.sync_count() - n0
    return r, r["s"].numpy().copy(), calls, syncs


# ----------------------------------------------------------------------------------------------
# operators
# ----------------------------------------------------------------------------------------------
N_DIAG = 20_001  # odd, and divisible by 3


def _diag_case(precon):
    rng = np.random.default_rng(77)
    g = rng.normal(size=N_DIAG)
    D = rng.uniform(0.5, 40.0, size=N_DIAG)
    Minv = 1.0 / (D * rng.uniform(0.5, 2.0, size=N_DIAG))
    blocks = rng.normal(size=(N_DIAG // 3, 3, 3))
    Binv = np.linalg.inv(blocks @ np.transpose(blocks, (0, 2, 1)) + 3 * np.eye(3)[None]).reshape(-1)

    def make(c):
        P = None
        if precon == "diag":
            P = c.precon_diag(c.upload(Minv))
        elif precon == "block3":
            P = c.precon_block3(c.upload(Binv))
        return c.upload(g), c.op_diag(c.upload(D)), P

    def host_P(v):
        if precon == "diag":
            return Minv * v
        return np.einsum("bij,bj->bi", Binv.reshape(-1, 3, 3), v.reshape(-1, 3)).reshape(-1)

    def oracle_solve(oracle, k, kw):
        return oracle.stpcg(g, lambda v: D * v, P=None if precon == "none" else host_P,
                            inner=lambda a, b: float(a @ b), Delta=kw["Delta"], max_iterations=k,
                            kappa_fgr=kw["kappa_fgr"], theta=kw["theta"])
    return make, oracle_solve, dict(g=g, D=D, Minv=Minv)


def _stiefel_case(grid, p):
    nx, ny, nz = grid
    n = nx * ny * nz
    rowptr, col, val = wl.laplacian_3d(nx, ny, nz)
    Xb, _ = wl.stiefel_bench_iterate(nx, ny, nz, p, eps=1e-3, seed=7)
    state = {}

    def grad_bits(oracle):
        if "go" not in state:
            oprob = oracle.stiefel_rq(n, p, rowptr, col, val)
            state.update(oprob=oprob, go=oracle.eval_grad(oprob, Xb.ravel()))
        return state["go"]

    def make(c, oracle=None):
        if state.get("ctx") is not c:
            A = c.csr(n, rowptr, col, val)
            prob = c.stiefel_rq(A, n, p)
            g, H = prob.model(c.upload(Xb))
            if oracle is not None:  # identical inputs: the oracle's gradient bits are the device solve's input
                g = c.upload(grad_bits(oracle))
            state.update(ctx=c, keep=(A, prob), g=g, H=H)
        return state["g"], state["H"], None

    def oracle_solve(oracle, k, kw):
        go = grad_bits(oracle)
        return oracle.stpcg_problem(state["oprob"], Xb.ravel(), go, kw["Delta"], max_iterations=k,
                                    kappa_fgr=kw["kappa_fgr"], theta=kw["theta"])
    return make, oracle_solve


DIAG_KW = dict(Delta=1e9, kappa_fgr=1e-12, theta=1.0)
STIEFEL_KW = dict(Delta=1e3, kappa_fgr=1e-12, theta=1.0)
STIEFEL_2E4 = (32, 25, 25)  # 20000 rows

CASES = [("diag-" + pre, pre, None) for pre in ("none", "diag", "block3")] + \
        [("stiefel-p%d" % p, None, (STIEFEL_2E4, p)) for p in (1, 3, 4, 6, 8)] + \
        [("cfg2-full", None, ((100, 100, 100), 3))]


def _case(name, pre, st, oracle):
    if st is None:
        make, oracle_solve, _ = _diag_case(pre)
        return make, oracle_solve, DIAG_KW, 60
    make, oracle_solve = _stiefel_case(*st)
    return (lambda c: make(c, oracle)), oracle_solve, STIEFEL_KW, (20 if name == "cfg2-full" else 40)


@pytest.mark.parametrize("name,pre,st", CASES, ids=[c[0] for c in CASES])
def test_observer_that_never_stops_and_stops_at_k(octx, oracle, name, pre, st):
    c = octx
    make, oracle_solve, kw, limit = _case(name, pre, st, oracle)
    g, H, P = make(c)
    fc0 = c.fusion_counters()
    plain = c.stpcg(g, H, P, trace_cap=64, max_iterations=limit, **kw)
    s_plain = plain["s"].numpy().copy()
    # --- an observer that only counts: every bit of the un-observed solve
    r, s, calls, syncs = _observed(c, g, H, P, trace_cap=64, max_iterations=limit, **kw)
    _bits_equal(plain, s_plain, r, s)
    assert len(calls) == r["iterations"], (len(calls), r["iterations"])
    assert [k for k, _ in calls] == list(range(len(calls)))
    assert np.array_equal(np.array([a for _, a in calls]), r["trace"]["alpha"][:len(calls)])
    assert syncs <= len(calls) + 2, (syncs, len(calls))
    fc1 = c.fusion_counters()
    assert fc1["fused_stpcg_solves"] - fc0["fused_stpcg_solves"] == 2
    assert fc1["generic_inner_products"] == fc0["generic_inner_products"]
    print(f"{name}: {r['iterations']} iterations, exit {r['exit_reason']}, {syncs} syncs for {len(calls)} calls")
    # --- stop at k, both parities, each k below the pass in which the un-stopped solve leaves
    assert r["iterations"] > 8, "the un-stopped solve must outlast the largest stop"
    for k in (0, 1, 2, 7, 8):
        rk, sk, calls_k, syncs_k = _observed(c, g, H, P, stop_at=k, max_iterations=limit, **kw)
        assert rk["exit_reason"] == USER and rk["iterations"] == k and len(calls_k) == k + 1, (k, rk, len(calls_k))
        assert syncs_k <= len(calls_k) + 2
        ref = c.stpcg(g, H, P, max_iterations=k, **kw)  # the reference's break (:369) and its loop bound (:285) leave the same s_k
        s_ref = ref["s"].numpy()
        assert np.array_equal(sk, s_ref), (k, int((sk != s_ref).sum()))
        assert rk["M_norm"] == ref["M_norm"] and rk["rv_final"] == ref["rv_final"], (k, rk, ref)
        if k == 0:
            assert not sk.any() and rk["M_norm"] == 0.0
        else:
            o = oracle_solve(oracle, k, kw)
            assert o["iterations"] == k
            err = rel_err(sk, o["s"])
            print(f"{name}: stop at {k}: s against the oracle with max_iterations = {k}: {err:.2e}")
            assert err < 1e-10, (k, err)


@pytest.mark.parametrize("pre", ["none", "diag"])
def test_views_are_the_vectors_of_the_solve(octx, pre):
    c = octx
    make, _, data = _diag_case(pre)
    g, H, P = make(c)
    K = 5
    seen = {}

    def at(k, s, r, v, p):
        if k == K:
            seen.update(s=s.numpy(), r=r.numpy(), v=v.numpy(), p=p.numpy(), same=(v.h.value == r.h.value),
                        dot=r.dot(v))
    r, s_final, calls, _ = _observed(c, g, H, P, at=at, max_iterations=12, **DIAG_KW)
    assert r["iterations"] == 12 and seen
    ref = c.stpcg(g, H, P, max_iterations=K, trace_cap=16, **DIAG_KW)
    assert np.array_equal(seen["s"], ref["s"].numpy())
    if pre == "none":
        assert seen["same"] and np.array_equal(seen["v"], seen["r"])       # v IS r (:231)
    else:
        assert not seen["same"] and np.array_equal(seen["v"], data["Minv"] * seen["r"])
    model_r = data["g"] + data["D"] * seen["s"]
    assert rel_err(seen["r"], model_r) < 1e-10
    # a read-only library call on the views inside the observer (mi_vec_dot): <r,v> of pass K is the rv the trace has
    assert abs(seen["dot"] - ref["trace"]["rv"][K - 1]) <= 1e-12 * abs(seen["dot"])
    # ... and it did not disturb the solve
    plain = c.stpcg(g, H, P, max_iterations=12, **DIAG_KW)
    _bits_equal(plain, plain["s"].numpy(), r, s_final, traces=False)


@pytest.mark.parametrize("p", [3, 6])
def test_operator_applied_inside_the_observer_leaves_the_solve_alone(octx, p):
    """the natural use of the H an observer is handed: the model value <g,s> + <s,Hs>/2 per pass (mi_op_apply on the views,
    into a vector of the caller's).  The partial rows the pass's k_cg_update still has to reduce must survive it: every
    bit of the un-observed solve, on the one-pass Stiefel Hessian in its narrow (p = 3) and wide (p = 6) form"""
    c = octx
    make, _ = _stiefel_case(STIEFEL_2E4, p)
    g, H, P = make(c)
    plain = c.stpcg(g, H, P, trace_cap=64, max_iterations=30, **STIEFEL_KW)
    Hs, Hp, model = c.vec(g.n), c.vec(g.n), []

    def at(k, s, r, v, pp):
        H.apply(s, Hs)
        H.apply(pp, Hp)
        model.append(g.dot(s) + 0.5 * s.dot(Hs))
    r, s, calls, _ = _observed(c, g, H, P, at=at, trace_cap=64, max_iterations=30, **STIEFEL_KW)
    _bits_equal(plain, plain["s"].numpy(), r, s)
    assert len(model) == 30 and model[0] == 0.0 and all(b < a for a, b in zip(model, model[1:])), model[:5]


def test_every_exit_under_observation_at_both_parities(octx):
    c = octx
    seen = set()

    def both(make, k_exit, kind, **kw):
        g, H, P = make(c)
        plain = c.stpcg(g, H, P, trace_cap=64, **kw)
        r, s, calls, syncs = _observed(c, g, H, P, trace_cap=64, **kw)
        _bits_equal(plain, plain["s"].numpy(), r, s)
        ks = [k for k, _ in calls]
        # the observer runs in every pass before the exiting one and not in it (a residual exit is decided at the end
        # of pass k_exit, :290 at the top of the next one: that pass was observed)
        want = k_exit + 1 if kind == "residual" else k_exit
        assert ks == list(range(want)), (kind, k_exit, ks)
        assert syncs <= len(calls) + 2
        seen.add((kind, k_exit & 1))
        return r

    g, D = _spd()
    rows = _host_cg(g, D, 12)
    for k in (1, 2, 3, 4):
        Delta = np.sqrt(_between(rows[k - 1]["s2"], rows[k]["s2"]))
        r = both(_diag_make(g, D), k, "boundary", Delta=Delta, max_iterations=100, kappa_fgr=1e-12, theta=1.0)
        assert r["exit_reason"] == BOUNDARY and r["iterations"] == k and r["M_norm"] == Delta
    rv0 = float(g @ g)
    for k in (1, 2, 3, 4):
        kf = np.sqrt(_between(rows[k]["rv"], rows[k - 1]["rv"]) / rv0)
        r = both(_diag_make(g, D), k, "residual", Delta=1e9, max_iterations=100, kappa_fgr=kf, theta=0.0)
        assert r["exit_reason"] == RESIDUAL and r["iterations"] == k + 1
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
    assert set(found) == {0, 1}
    for D2, k in found.values():
        r = both(_diag_make(g, D2), k, "negative_curvature", Delta=1e9, max_iterations=100, kappa_fgr=1e-12, theta=1.0)
        assert r["exit_reason"] == BOUNDARY and r["iterations"] == k and r["M_norm"] == 1e9
    D0 = 0.05 * D
    D0[::3] = 0.0
    rows0 = _host_cg(g, D0, 12)
    for k in (1, 2, 3, 4):
        eps = _between(rows0[k]["ratio"], min(x["ratio"] for x in rows0[:k]))
        r = both(_diag_make(g, D0), k, "kernel", Delta=1e9, max_iterations=100, kappa_fgr=1e-12, theta=1.0, epsilon=eps)
        assert r["exit_reason"] == KERNEL and r["iterations"] == k and r["M_norm"] == 1e9
    # exits in the very first pass, and a solve that never enters the loop: no call at all
    for make, kw in ((_diag_make(g, np.zeros_like(g)), dict(Delta=7.0, max_iterations=10)),
                     (_diag_make(g, D), dict(Delta=1e-3, max_iterations=10)),
                     (_diag_make(g, D), dict(Delta=1.0, max_iterations=0))):
        gg, H, P = make(c)
        plain = c.stpcg(gg, H, P, **kw)
        r, s, calls, _ = _observed(c, gg, H, P, **kw)
        _bits_equal(plain, plain["s"].numpy(), r, s, traces=False)
        assert calls == []
    want = {(kind, par) for kind in ("boundary", "negative_curvature", "kernel", "residual") for par in (0, 1)}
    assert seen == want, sorted(want - seen)


def test_exception_in_the_observer_stops_the_solve_and_is_reraised(octx):
    c = octx
    make, _, _ = _diag_case("diag")
    g, H, P = make(c)

    class Boom(Exception):
        pass

    def observer(k, s, r, v, p, alpha):
        if k == 3:
            raise Boom("at 3")
        return False
    with pytest.raises(Boom):
        c.stpcg(g, H, P, observer=observer, max_iterations=20, **DIAG_KW)
    # the context is fit for the next solve
    plain = c.stpcg(g, H, P, max_iterations=20, trace_cap=32, **DIAG_KW)
    r, s, calls, _ = _observed(c, g, H, P, max_iterations=20, trace_cap=32, **DIAG_KW)
    _bits_equal(plain, plain["s"].numpy(), r, s)
    # a solve started from inside an observer is refused, not run
    inner = []

    def nested(k, s, r, v, p, alpha):
        try:
            c.stpcg(g, H, P, max_iterations=2, **DIAG_KW)
        except capi.MiError as e:
            inner.append(e.status)
        return True
    c.stpcg(g, H, P, observer=nested, max_iterations=5, **DIAG_KW)
    assert inner == [1]


@pytest.mark.parametrize("option", ["NO_FUSED_OBSERVER", "FORCE_LOCKSTEP", "FORCE_SLOT_PATH"])
def test_declined_calls_do_nothing(option):
    with capi.Context(0) as c:
        make, _, _ = _diag_case("none")
        g, H, P = make(c)
        c.set_option(option, 1)
        fc0, calls = c.fusion_counters(), []
        with pytest.raises(capi.MiError) as e:
            c.stpcg(g, H, P, observer=lambda *a: calls.append(a) or False, max_iterations=5, **DIAG_KW)
        assert e.value.status == 7 and calls == []           # MI_DECLINED: its own status
        assert c.fusion_counters() == fc0
        c.set_option(option, 0)
        r = c.stpcg(g, H, P, observer=lambda *a: calls.append(a) or False, max_iterations=5, **DIAG_KW)
        assert r["iterations"] == 5 and len(calls) == 5


def test_peek_kernel_is_timed_as_cg_scalar_a(octx):
    c = octx
    make, _, _ = _diag_case("none")
    g, H, P = make(c)
    c.ktime_reset()
    c.ktime_enable("cg_scalar_a", True)
    c.stpcg(g, H, P, max_iterations=9, **DIAG_KW)
    assert c.ktime_read("cg_scalar_a")[0] == 0            # the un-observed solve launches what it always launched
    r, _, calls, _ = _observed(c, g, H, P, max_iterations=9, **DIAG_KW)
    launches, ms = c.ktime_read("cg_scalar_a")
    c.ktime_enable("cg_scalar_a", False)
    assert launches == len(calls) == 9
    print(f"k_cg_peek: {1e3 * ms / launches:.1f} us per launch between events")


# ----------------------------------------------------------------------------------------------
# the template layer
# ----------------------------------------------------------------------------------------------
def test_user_function_keeps_the_fused_solver_counters_and_fixture(obs, golden):
    """tests/golden/stpcg_user_stop.json (the REAL reference), every case, through STPCG<DeviceVector> with tagged
    callables and a user function: the fixture's iteration and call counts, the tolerances of
    test_gpu_templates.py::test_stpcg_user_function_stop_on_device_vectors -- and the solve ran FUSED: one fused solve,
    no generic solve, no host-synchronising inner product.  With NO_FUSED_OBSERVER=1 the same call shows the opposite."""
    import oracle_py
    fx = golden("stpcg_user_stop.json")
    pr = oracle_py.stpcg_stop_problem(fx["n"], fx["seed"])
    for c in fx["cases"]:
        for off in (False, True):
            r = obs.diag(1, pr["g"], pr["D"], pr["Minv"] if c["precon"] else None, 1e6, 100, 1e-10, 1.0,
                         stop_at=c["stop_at"], record_dots=False, no_fused_observer=off)
            assert r["rc"] == 0, obs.err()
            assert (r["iterations"], r["calls"]) == (c["iterations"], c["calls"]), (c["stop_at"], off)
            tol = 1e-10 if c["iterations"] < 100 else 1e-5
            es = np.abs(r["s"] - np.array(c["s"])).max() / max(1e-300, np.abs(c["s"]).max())
            em = abs(r["M_norm"] - c["M_norm"]) / max(1e-300, c["M_norm"])
            print(f"precon {c['precon']} stop_at {c['stop_at']} {'generic' if off else 'fused'}: s {es:.2e} M_norm {em:.2e} "
                  f"syncs {r['syncs']}")
            assert es <= tol and (em <= tol or c["M_norm"] == 0.0)
            counters = (r["fused_stpcg_solves"], r["generic_stpcg_solves"], r["generic_inner_products"] > 0)
            assert counters == ((0, 1, True) if off else (1, 0, False)), (c["stop_at"], off, counters)
            if not off:
                assert r["syncs"] <= r["calls"] + 2


def _records_agree(host, dev, dev_rc=0):
    assert host["rc"] == 0 and dev["rc"] == dev_rc
    assert host["calls"] == dev["calls"] and host["iterations"] == dev["iterations"], (host["calls"], dev["calls"])
    assert np.array_equal(host["rec"][:, 0], dev["rec"][:, 0])
    e = np.abs(dev["rec"][:, 1:] - host["rec"][:, 1:]) / np.maximum(np.abs(host["rec"][:, 1:]), 1e-300)
    e[host["rec"][:, 1:] == dev["rec"][:, 1:]] = 0.0  # (<s,s> = <s,p> = 0 in pass 0)
    worst = e.max(axis=0)
    print("calls %d; worst relative deviation of alpha, <s,s>, <r,r>, <r,v>, <p,p>, <s,p>: %s"
          % (host["calls"], " ".join("%.1e" % w for w in worst)))
    assert worst.max() <= 1e-10, worst


@pytest.mark.parametrize("precon", [False, True])
def test_what_the_user_function_sees_host_loop_against_fused_solve(obs, precon):
    import oracle_py
    pr = oracle_py.stpcg_stop_problem()
    kappa = KAPPA_PRECON if precon else KAPPA_PLAIN
    args = (pr["g"], pr["D"], pr["Minv"] if precon else None, 1e6, 400, kappa, 1.0)
    host = obs.diag(0, *args)
    assert host["iterations"] < 100 and host["calls"] == host["iterations"]   # left by the residual test (:290)
    dev = obs.diag(1, *args)
    assert dev["rc"] == 0, obs.err()
    _records_agree(host, dev)
    assert dev["fused_stpcg_solves"] == 1 and dev["generic_stpcg_solves"] == 0
    assert dev["v_is_r"] == (0 if precon else 1) and dev["P_engaged"] == int(precon) and dev["At_engaged"] == 0
    assert rel_err(dev["s"], host["s"]) < 1e-10 and abs(dev["M_norm"] - host["M_norm"]) <= 1e-10 * host["M_norm"]


def test_projected_solve_under_observation(obs, golden):
    import oracle_py
    pr = oracle_py.projected_stpcg_problem("truncated")
    fx = golden("stpcg_projected.json")["truncated"]
    host, dev = obs.projected(0, pr), obs.projected(1, pr)
    assert dev["rc"] == 0, obs.err()
    assert host["iterations"] == dev["iterations"] == fx["iterations"]
    assert dev["P_engaged"] == 1 and dev["At_engaged"] == 1 and dev["v_is_r"] == 0
    assert dev["fused_stpcg_solves"] == 1 and dev["generic_stpcg_solves"] == 0
    _records_agree(host, dev)
    assert rel_err(dev["s"], np.array(fx["s"])) < 1e-10
    assert np.linalg.norm(pr["A"] @ dev["s"]) < 1e-6


def test_user_function_that_throws_reaches_the_caller(obs):
    import oracle_py
    pr = oracle_py.stpcg_stop_problem()
    args = (pr["g"], pr["D"], pr["Minv"], 1e6, 400, KAPPA_PRECON, 1.0)
    host = obs.diag(0, *args)
    dev = obs.diag(1, *args, throw_at=2)   # throws in pass 2, then the same solve again on the same context
    assert dev["rc"] == -3, (dev["rc"], obs.err())   # the exception reached the caller of STPCG
    _records_agree(host, dev, dev_rc=-3)              # ... and the solve behind it on the same context is correct
    assert dev["fused_stpcg_solves"] == 1
