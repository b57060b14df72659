"""GradientDescent on SO(3)^N (optimization_amd/csrc/so3.hip: k_so3_grad; mi_so3n_gradient,
mi_so3n_armijo_trial; MI355::RotationAveraging::gradient() and the `armijo` hook of its retraction()).

1. the gradient-only pass against the fp64 oracle and the longdouble restatement of tests/so3_cases.py at the bar
   tests/test_gpu_so3n_edges.py applies to the model's gradient (1e-13 norm-wise, the oracle within a third of it of the
   longdouble value), AND bit for bit against the gradient mi_so3n_model writes; f of the pass bit for bit against
   mi_so3n_objective -- on all four measurement x gather forms;
2. the Armijo chain bit for bit against the separate calls, with one host synchronisation;
3. the keys: which point's gradient / model the library believes it holds;
4. the template layer on the two cases of tests/golden/gd_so3n.json (the REAL reference's counts).

generic_inner_products of a fused run is asserted to be exactly 1, not 0: Riemannian/GradientDescent.h:217 forms
sqrt(metric(x0, g0, g0)) BEFORE the loop in every mode (mi_vec_dot, one host synchronisation), as the reference does;
the loop itself adds none (the statement sequence adds one per accepted iteration)."""
import contextlib
import functools

import numpy as np
import pytest

import so3_cases as sc
from conftest import floor_or, rel_err
from optimization_amd import workloads as wl

pytestmark = pytest.mark.gpu

FORMS = ("default", "no_quat", "no_rquat", "no_quat_no_rquat")


# ---------------------------------------------------------------------------------------------------------------------
# cases: the smallest graphs on which the pass can go wrong
# ---------------------------------------------------------------------------------------------------------------------
def _n65():
    """two slices, the second one ragged (one node), and that last node isolated"""
    ei, ej = wl.pose_graph(64, seed=5)[:2]
    return sc._build("n65_isolated_last", 65, ei, ej, 165, "linspace")


_CASES = {
    "tiny_1": lambda: sc.case("tiny_1"),                                  # N = 1, no edge
    "pose_40": lambda: sc.ring_chords(40, "linspace", seed=7),            # the graph of tests/golden/tnt_so3n_40.json
    "n65_isolated_last": _n65,
    "hub_300": lambda: sc.hub(False, "linspace", N=300),                  # degree N - 1 at node 0; 5 slices = 2 groups of 4
    "some_zero_130": lambda: sc.ring_chords(130, "some_zero"),
    "node_zero_130": lambda: sc.ring_chords(130, "node_zero"),
    "negative_130": lambda: sc.ring_chords(130, "negative"),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    return _CASES[name]()


@functools.lru_cache(maxsize=None)
def _reference(name):
    """longdouble f and gradient, once per case"""
    ref = sc.So3Ref(_case(name))
    return ref.f(), ref.grad()


_ORACLE = {}


def _oracle_values(oracle, name):
    """the fp64 oracle's gradient and its distance from the longdouble one (the floor), once per case"""
    if name not in _ORACLE:
        c = _case(name)
        op = oracle.so3n(c.N, c.ei, c.ej, c.Rt, c.w, precon_kind=0)
        try:
            go = oracle.eval_grad(op, c.R.ravel())
        finally:
            oracle.free(op)
        _ORACLE[name] = (go, sc.rel_err_ld(go, _reference(name)[1]))
    return _ORACLE[name]


@contextlib.contextmanager
def _form_ctx(form):
    from optimization_amd import capi
    c = capi.Context(0)
    try:
        for k, v in sc.FORMS[form].items():
            c.set_option(k, v)
        yield c
    finally:
        c.close()


def _bits(v):
    return v.numpy().view(np.uint64)


# ---------------------------------------------------------------------------------------------------------------------
# 1. gradient pass
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", list(_CASES))
def test_so3n_gradient_pass_vs_oracle_longdouble_and_the_model_pass(oracle, name, form):
    c = _case(name)
    go, floor = _oracle_values(oracle, name)
    gr = _reference(name)[1]
    assert floor_or(sc.TOL_G, floor) == sc.TOL_G, (name, floor)      # an oracle that drifts cannot widen the bar unseen
    with _form_ctx(form) as ctx:
        prob = ctx.so3n(c.N, c.ei, c.ej, c.Rt, c.w)
        info = prob.info()
        assert info["gather_quat"] == ("SO3_NO_RQUAT" not in sc.FORMS[form])
        assert info["sinc_quat"] == ("SO3_NO_QUAT" not in sc.FORMS[form])
        assert info["nslices"] == (c.N + 63) // 64 and info["nnzb"] == 2 * c.ei.size
        R = ctx.upload(c.R)
        ctx.ktime_enable("so3_grad")
        ctx.ktime_reset()
        g = prob.gradient(R)
        assert ctx.ktime_read("so3_grad")[0] == 1                    # the gradient-only kernel ran (once)
        e_orc, e_ref = rel_err(g.numpy(), go), sc.rel_err_ld(g.numpy(), gr)
        print(f"{name} {form}: grad vs oracle {e_orc:.2e} vs longdouble {e_ref:.2e} floor {floor:.2e}")
        assert e_orc <= sc.TOL_G and e_ref <= sc.TOL_G, (name, form, e_orc, e_ref)
        gm, H, P = prob.model(R)
        assert np.array_equal(_bits(g), _bits(gm)), (name, form, np.abs(g.numpy() - gm.numpy()).max())
        # f of the gradient pass (delivered by the Armijo chain) against mi_so3n_objective at the same point: a step of
        # length 0 leaves R where it is (R_i (I + 0) = R_i exactly)
        h, Rp, out = prob.armijo_trial(R, g, 0.0)
        assert np.array_equal(Rp.numpy(), c.R.ravel()) and not h.numpy().any()
        assert out["f"] == prob.objective(R) == prob.objective(Rp)
        assert np.array_equal(_bits(prob.gradient(Rp)), _bits(gm))
        assert out["grad_sqnorm"] == gm.dot(gm)


# ---------------------------------------------------------------------------------------------------------------------
# 2. Armijo chain = the separate calls
# ---------------------------------------------------------------------------------------------------------------------
def _placed_gradient(c, t):
    """a "gradient" whose step -t g has, node by node, the lengths of so3_cases.SWEEP (0, both sides of the retraction's
    series switch at 1e-4, 1, pi, 2 pi, 10) along random axes, and is exactly 0 on the nodes without an edge"""
    rng = np.random.Generator(np.random.PCG64(12))
    ax = rng.normal(size=(c.N, 3))
    ax /= np.linalg.norm(ax, axis=1)[:, None]
    ax[:3] = np.eye(3)
    mags = np.array([sc.SWEEP[i % len(sc.SWEEP)] for i in range(c.N)])
    g = ax * (mags / t)[:, None]
    g[sc.singular_nodes(c)] = 0.0
    return np.ascontiguousarray(g.ravel())


@pytest.mark.parametrize("form", ["default", "no_rquat", "no_quat"])
def test_so3n_armijo_chain_has_the_bits_of_the_separate_calls(form):
    c = sc.case("isolated_1500")
    t = 0.37
    gh = _placed_gradient(c, t)
    with _form_ctx(form) as ctx:
        prob = ctx.so3n(c.N, c.ei, c.ej, c.Rt, c.w)
        assert prob.info()["gather_quat"] == (form != "no_rquat")
        R, g = ctx.upload(c.R), ctx.upload(gh)
        # the statement sequence on fresh vectors
        h_ref = g.scaled(-t)
        Y_ref = prob.retract(R, h_ref)
        f_ref = prob.objective(Y_ref)
        g_ref = prob.gradient(Y_ref)
        n_ref = g_ref.dot(g_ref)
        hn = np.linalg.norm(h_ref.numpy().reshape(c.N, 3), axis=1)
        assert (hn == 0).sum() >= 60 and ((hn > 0) & (hn < 1e-4)).sum() >= 100 and ((hn > 1e-4) & (hn < 1.1e-4)).sum() >= 100
        assert (np.abs(hn - np.pi) < 1e-14).sum() >= 100 and (hn > 9).sum() >= 100
        # the chain, into vectors that exist already
        h, Rp = ctx.vec(3 * c.N), ctx.vec(9 * c.N)
        f0 = ctx.fusion_counters()
        s0 = ctx.sync_count()
        _, _, out = prob.armijo_trial(R, g, t, h=h, R_trial=Rp)
        assert ctx.sync_count() - s0 == 1
        assert ctx.fusion_counters()["fused_trial_steps"] - f0["fused_trial_steps"] == 1
        assert np.array_equal(_bits(h), _bits(h_ref))
        assert np.array_equal(_bits(Rp), _bits(Y_ref))
        assert out["f"] == f_ref and out["grad_sqnorm"] == n_ref
        assert np.array_equal(_bits(prob.gradient(Rp)), _bits(g_ref))          # the stored gradient
        # the next gather reads the quaternions the step kernel left: a second trial from R+ along its gradient
        g2 = prob.gradient(Rp)
        _, Rpp, out2 = prob.armijo_trial(Rp, g2, 1e-3)
        Ypp = prob.retract(Y_ref, g_ref.scaled(-1e-3))
        assert np.array_equal(_bits(Rpp), _bits(Ypp)) and out2["f"] == prob.objective(Ypp)
        assert np.array_equal(_bits(prob.gradient(Rpp)), _bits(prob.gradient(Ypp)))


# ---------------------------------------------------------------------------------------------------------------------
# 3. keys
# ---------------------------------------------------------------------------------------------------------------------
def _key_problem(ctx):
    c = _case("hub_300")
    prob = ctx.so3n(c.N, c.ei, c.ej, c.Rt, c.w)
    return c, prob, ctx.upload(c.R)


def test_so3n_model_after_an_armijo_trial_is_assembled_not_swapped_in(ctx):
    """(a) the point of an Armijo trial has a gradient and no model: mi_so3n_model there must assemble.  A trust-region
    trial first, so that the second set of arrays holds a (stale) model that a swap would bring in."""
    c, prob, R = _key_problem(ctx)
    g, H, P = prob.model(R)
    xi = ctx.upload(np.random.default_rng(3).normal(size=3 * c.N))
    prob.trial(R, g.scaled(-0.01), g)                        # fills Dinv_next / Bblk_next / Dsl_next at another point
    h, Rp, out = prob.armijo_trial(R, g, 0.02)
    gp, Hp, Pp = prob.model(Rp)
    prob2 = ctx.so3n(c.N, c.ei, c.ej, c.Rt, c.w)
    gq, Hq, Pq = prob2.model(Rp.copy())
    assert np.array_equal(_bits(gp), _bits(gq))
    assert np.array_equal(_bits(Hp.apply(xi)), _bits(Hq.apply(xi)))
    assert np.array_equal(_bits(Pp.apply(xi)), _bits(Pq.apply(xi)))
    assert out["grad_sqnorm"] == gq.dot(gq)
    # ... and the model call dropped the Armijo key: the next gradient there is assembled
    ctx.ktime_enable("so3_grad")
    ctx.ktime_reset()
    assert np.array_equal(_bits(prob.gradient(Rp)), _bits(gq))
    assert ctx.ktime_read("so3_grad")[0] == 1
    ctx.ktime_enable("so3_grad", False)


def test_so3n_gradient_at_the_armijo_point_is_a_copy_until_the_point_is_written(ctx):
    """(b) no assembly for the point the last Armijo trial evaluated; (c) an in-place write revives nothing"""
    c, prob, R = _key_problem(ctx)
    g = prob.gradient(R)
    h, Rp, out = prob.armijo_trial(R, g, 0.02)
    fresh = prob.gradient(Rp.copy())                          # (another handle: assembled)
    ctx.ktime_enable("so3_grad")
    ctx.ktime_reset()
    stored = prob.gradient(Rp)
    assert ctx.ktime_read("so3_grad")[0] == 0                 # (b)
    assert np.array_equal(_bits(stored), _bits(fresh))
    assert np.array_equal(_bits(prob.gradient(Rp)), _bits(fresh)) and ctx.ktime_read("so3_grad")[0] == 0   # not consumed
    Rp.scale(1.0)                                             # (c) an in-place write (of the same values): a new generation
    rewritten = prob.gradient(Rp)
    assert ctx.ktime_read("so3_grad")[0] == 1                 # assembled afresh
    assert np.array_equal(_bits(rewritten), _bits(fresh))
    ctx.ktime_enable("so3_grad", False)


def test_so3n_gradient_at_a_tnt_trial_point_leaves_the_speculative_model_in_place(ctx):
    """(d) mi_so3n_trial, mi_so3n_gradient(R_trial), mi_so3n_model(R_trial): the bits of the sequence without the
    gradient call, and the gradient call assembles nothing"""
    c = _case("hub_300")
    xi = ctx.upload(np.random.default_rng(4).normal(size=3 * c.N))
    res = []
    for with_gradient in (True, False):
        prob = ctx.so3n(c.N, c.ei, c.ej, c.Rt, c.w)
        R = ctx.upload(c.R)
        g, H, P = prob.model(R)
        Rt, t = prob.trial(R, g.scaled(-0.01), g)
        if with_gradient:
            ctx.ktime_enable("so3_grad")
            ctx.ktime_reset()
            gt = prob.gradient(Rt)
            assert ctx.ktime_read("so3_grad")[0] == 0
            ctx.ktime_enable("so3_grad", False)
        g2, H2, P2 = prob.model(Rt)
        if with_gradient:
            assert np.array_equal(_bits(gt), _bits(g2))
        res.append((t["f"], t["grad_sqnorm"], g2.numpy(), H2.apply(xi).numpy(), P2.apply(xi).numpy()))
    a, b = res
    assert a[0] == b[0] and a[1] == b[1]
    for u, v in zip(a[2:], b[2:]):
        assert np.array_equal(u.view(np.uint64), v.view(np.uint64))


def test_so3n_armijo_trial_and_gradient_refuse_bad_arguments(ctx):
    """(e) as mi_so3n_trial: an aliased trial point and wrong lengths are MI_ERR_INVALID_ARGUMENT with a message"""
    from optimization_amd import capi
    c, prob, R = _key_problem(ctx)
    g = prob.gradient(R)
    for kw in (dict(R_trial=R), dict(R_trial=ctx.vec(9 * c.N - 9)), dict(h=ctx.vec(3 * c.N + 3)), dict(h=g)):
        with pytest.raises(capi.MiError) as e:
            prob.armijo_trial(R, g, 0.1, **kw)
        assert e.value.status == 1 and str(e.value)
    with pytest.raises(capi.MiError) as e:
        prob.armijo_trial(R, ctx.vec(3 * c.N - 3), 0.1)
    assert e.value.status == 1
    for bad in (lambda: prob.gradient(ctx.vec(9 * c.N + 9)), lambda: prob.gradient(R, out=ctx.vec(3 * c.N + 1))):
        with pytest.raises(capi.MiError) as e:
            bad()
        assert e.value.status == 1 and str(e.value)


# ---------------------------------------------------------------------------------------------------------------------
# 4. template layer
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gd_harness():
    import harness_gd_so3n_py as hg
    return hg.GdSo3nHarness()


_RUNS = {}


def _run(gd_harness, golden, key, mode):
    if (key, mode) not in _RUNS:
        g = golden("gd_so3n.json")[key]
        ei, ej, Rt, w, _, Rinit = wl.pose_graph(g["N"], seed=g["seed"])
        r = gd_harness.gd(g["N"], ei, ej, Rt, w, Rinit, g["params"], mode)
        assert r["rc"] == 0, r["err"]
        _RUNS[(key, mode)] = r
    return _RUNS[(key, mode)]


def _same_counts(r, g):
    assert (r["status"], r["iterations"]) == (g["status"], g["iterations"])
    assert list(r["linesearch_iterations"]) == g["linesearch_iterations"]


@pytest.mark.parametrize("key", ["N40", "N150"])
def test_gd_so3n_fused_armijo_trial_vs_reference_fixture(gd_harness, golden, key):
    import harness_gd_so3n_py as hg
    g = golden("gd_so3n.json")[key]
    r = _run(gd_harness, golden, key, hg.FUSED)
    _same_counts(r, g)
    m = g["iterations"]
    trace = np.array(g["objective_values"] + [g["f"]])
    e_f = np.abs(r["objective_values"][:m + 1] - trace).max() / np.abs(trace).min()
    e_x = rel_err(r["x"], np.array(g["x"]))
    print(f"{key}: trace {e_f:.2e} x {e_x:.2e} syncs {r['counters']['syncs']}")
    assert np.allclose(r["objective_values"][:m + 1], trace, rtol=1e-10, atol=0)
    assert e_x <= 1e-10 and abs(r["f"] - g["f"]) <= 1e-10 * abs(g["f"])
    k = r["counters"]
    trials = int(np.sum(g["linesearch_iterations"]))
    assert k["fused_trial_steps"] == trials and k["generic_trial_steps"] == 0
    assert k["generic_inner_products"] == 1          # GradientDescent.h:217, before the loop (module docstring)
    assert k["syncs"] <= trials + 4                  # one read-back per trial; f(x0), |g0| and the final download


@pytest.mark.parametrize("key", ["N40", "N150"])
def test_gd_so3n_statement_sequence_has_the_bits_of_the_fused_run(gd_harness, golden, key):
    import harness_gd_so3n_py as hg
    g = golden("gd_so3n.json")[key]
    a, b = _run(gd_harness, golden, key, hg.FUSED), _run(gd_harness, golden, key, hg.PLAIN_RETRACTION)
    _same_counts(b, g)
    assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["objective_values"], b["objective_values"])
    assert a["f"] == b["f"] and a["gradfx_norm"] == b["gradfx_norm"]
    trials = int(np.sum(g["linesearch_iterations"]))
    kb = b["counters"]
    assert kb["fused_trial_steps"] == 0 and kb["generic_trial_steps"] == trials
    assert kb["generic_inner_products"] == g["iterations"] + 1
    assert kb["syncs"] >= a["counters"]["syncs"] + g["iterations"]


@pytest.mark.parametrize("key", ["N40", "N150"])
def test_gd_so3n_with_a_pack_keeps_the_fused_armijo_trial(gd_harness, golden, key):
    import harness_gd_so3n_py as hg
    a, b = _run(gd_harness, golden, key, hg.FUSED), _run(gd_harness, golden, key, hg.PACK)
    assert (a["status"], a["iterations"]) == (b["status"], b["iterations"])
    assert np.array_equal(a["linesearch_iterations"], b["linesearch_iterations"])
    assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["objective_values"], b["objective_values"])
    assert a["gradfx_norm"] == b["gradfx_norm"]
    for name in ("fused_trial_steps", "generic_trial_steps", "generic_inner_products", "syncs"):
        assert a["counters"][name] == b["counters"][name], name


def test_gd_so3n_with_a_wrapped_objective_runs_the_statement_sequence(gd_harness, golden):
    import harness_gd_so3n_py as hg
    g = golden("gd_so3n.json")["N40"]
    r = _run(gd_harness, golden, "N40", hg.WRAPPED_OBJECTIVE)
    k = r["counters"]
    assert r["status"] == 0 and k["fused_trial_steps"] == 0
    assert k["generic_trial_steps"] == int(np.sum(r["linesearch_iterations"])) > 0
    # f + 1: the same minimiser
    assert abs(r["f"] - 1.0 - g["f"]) <= 1e-9 * abs(g["f"])
