"""Robust loss by device-side edge reweighting (optimization_amd/csrc/so3.hip: k_so3_edge_weight, k_so3_inc_reweight;
mi_so3n_reweight / mi_so3n_weights) against the longdouble restatement of tests/so3n_robust_reference.py and against a
problem created afresh with the downloaded weights.

(a) the weights against the reference: |w_e - w_ref| <= 64 eps max(1, 1/c) |w0_e| (so3n_robust_reference.weight_tol);
(b) a reweighted problem is the problem with those weights: bit-equal objective, model gradient, Hessian products,
    block-Jacobi product, trial outputs, certificate info and product; residual, dF, dF*, gn_scaling to 4 eps of the largest
    entry of the edge (node) block;
(c) Huber, then L2 with R = NULL restores a never-reweighted problem;
(d) nothing stale: trial -> reweight -> model, armijo_trial -> reweight -> gradient, and a least-squares view / gn_scaling
    first asked for after a reweighting;
(e) the info sums; (f) host waits; (g) refusals."""
import numpy as np
import pytest

import so3_cases as sc
import so3n_robust_reference as rr
from so3_cases import LD

pytestmark = pytest.mark.gpu

EPS = rr.EPS
ROBUST = ("huber", "cauchy", "geman_mcclure")


@pytest.fixture(scope="module")
def ctx():
    from optimization_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def _problem(ctx, c, w=None):
    from optimization_amd import capi
    return capi.So3N(ctx, c.N, c.ei, c.ej, c.Rt, c.w if w is None else w)


def _outputs(ctx, prob, c, R_host, nls=True):
    """everything of (b): (exact: dict of arrays compared bit for bit, close: dict of (array, block width))"""
    R = ctx.upload(R_host)
    xis, v = sc.probes(c)
    exact, close = {}, {}
    exact["objective"] = np.array([prob.objective(R)])
    g, H, P = prob.model(R)
    exact["gradient"] = g.numpy()
    for k, xi in enumerate(xis):
        exact[f"hess{k}"] = H.apply(ctx.upload(xi)).numpy()
    exact["block_jacobi"] = P.apply(ctx.upload(v)).numpy()
    Rt, t = prob.trial(R, ctx.upload(0.01 * xis[0]), g)
    exact["trial"] = np.array([t[k] for k in ("f", "hh", "gh", "hHh", "grad_sqnorm", "precon_grad_sqnorm")])
    exact["trial_point"] = Rt.numpy()
    cert, info = prob.certificate(R)
    exact["cert_info"] = np.array([info[k] for k in ("f", "stationarity", "trace_C")])
    X = np.random.Generator(np.random.PCG64(5)).normal(size=3 * c.N * 4)
    exact["cert_apply"] = cert.apply(4, ctx.upload(X)).numpy()
    if nls and c.ei.size:
        close["residual"] = (prob.residual(R).numpy(), 9)
        dF, dFt = prob.jacobian(R)
        close["dF"] = (dF.apply(ctx.upload(xis[1])).numpy(), 9)
        Y = np.random.Generator(np.random.PCG64(6)).normal(size=9 * c.ei.size)
        close["dFt"] = (dFt.apply(ctx.upload(Y)).numpy(), 3)
        close["gn_scaling"] = (prob.gn_scaling().apply(ctx.upload(np.ones(3 * c.N))).numpy(), 3)
    return exact, close


def _compare(a, b, what, bitwise_close=False):
    ea, ca = a
    eb, cb = b
    for k in ea:
        assert np.array_equal(ea[k], eb[k], equal_nan=True), (what, k, float(np.nanmax(np.abs(ea[k] - eb[k]))))
    worst = {}
    for k in ca:
        (x, blk), (y, _) = ca[k], cb[k]
        if bitwise_close:
            assert np.array_equal(x, y), (what, k, float(np.abs(x - y).max()))
            continue
        scale = np.abs(y).reshape(-1, blk).max(axis=1)
        err = np.abs(x - y).reshape(-1, blk).max(axis=1)
        worst[k] = float((err / np.where(scale > 0, scale, 1.0)).max() / EPS) if err.size else 0.0
        assert np.all(err <= 4 * EPS * scale), (what, k, worst[k])
    return worst


@pytest.mark.parametrize("name", rr.VARIANTS)
def test_weights_and_info_against_the_reference(ctx, name):
    """(a) and (e), every kind and scale at the variant's point"""
    c = rr.variant(name)
    prob = _problem(ctx, c)
    R = ctx.upload(c.R.ravel())
    worst = 0.0
    for kind in rr.KINDS:
        for s in rr.SCALES:
            ref = rr.reference(name, kind, s)
            info = prob.reweight(R, kind, s)
            w = prob.weights()
            ratio = np.abs(w.astype(LD) - ref.w) / (rr.weight_tol(s) * np.abs(c.w.astype(LD)))
            worst = max(worst, float(ratio.max()))
            assert np.all(ratio <= 1), (name, kind, s, float(ratio.max()))
            for got, want in ((info["robust_cost"], ref.robust_cost), (info["weighted_cost"], ref.weighted_cost)):
                assert abs(LD(got) - want) <= 1e-10 * abs(want), (name, kind, s, got, float(want))
            assert info["outliers"] == ref.outliers, (name, kind, s)
            f = prob.objective(R)
            assert abs(info["weighted_cost"] - f) <= 1e-10 * abs(f), (name, kind, s, info["weighted_cost"], f)
    print(name, "largest |w - w_ref| / bound:", worst)


@pytest.mark.parametrize("kind,s", [("huber", 0.5), ("cauchy", 0.05), ("geman_mcclure", 3.0)])
@pytest.mark.parametrize("name", rr.VARIANTS)
def test_reweighted_problem_is_the_problem_with_those_weights(ctx, name, kind, s):
    """(b); the least-squares arrays exist BEFORE the reweighting (its edge pass writes sqrt(w))"""
    c = rr.variant(name)
    prob = _problem(ctx, c)
    R = ctx.upload(c.R.ravel())
    if c.ei.size:
        prob.jacobian(R)
        prob.gn_scaling()
    prob.reweight(R, kind, s, info=False)
    fresh = _problem(ctx, c, prob.weights())
    worst = _compare(_outputs(ctx, prob, c, c.R.ravel()), _outputs(ctx, fresh, c, c.R.ravel()), (name, kind, s))
    print(name, kind, s, "largest error in units of eps:", worst)


@pytest.mark.parametrize("name", ("ring_chords_1500:outliers", "nonrot_1025:outliers", "hub:random", "tiny_2:random"))
def test_l2_restores_the_creation_time_weights(ctx, name):
    """(c)"""
    c = rr.variant(name)
    prob, never = _problem(ctx, c), _problem(ctx, c)
    R = ctx.upload(c.R.ravel())
    prob.jacobian(R)
    prob.gn_scaling()
    prob.reweight(R, "huber", 0.05)
    assert not np.array_equal(prob.weights(), c.w)
    assert prob.reweight(None, "l2", 1.0, info=False) is None
    assert np.array_equal(prob.weights(), c.w)
    _compare(_outputs(ctx, prob, c, c.R.ravel()), _outputs(ctx, never, c, c.R.ravel()), name, bitwise_close=True)


@pytest.mark.parametrize("name", ("ring_chords_1500:outliers", "nonrot_1025:random", "multigraph:outliers"))
def test_no_stale_model_after_a_reweighting(ctx, name):
    """(d)"""
    c = rr.variant(name)
    xis, _ = sc.probes(c)
    prob = _problem(ctx, c)
    R = ctx.upload(c.R.ravel())
    g, H, P = prob.model(R)
    Rt, _ = prob.trial(R, ctx.upload(0.05 * xis[0]), g)
    prob.reweight(Rt, "cauchy", 0.5, info=False)
    w = prob.weights()
    fresh = _problem(ctx, c, w)
    Rt2 = ctx.upload(Rt.numpy())
    g1, H1, P1 = prob.model(Rt)
    g2, H2, P2 = fresh.model(Rt2)
    assert np.array_equal(g1.numpy(), g2.numpy())
    x = ctx.upload(xis[1])
    assert np.array_equal(H1.apply(x).numpy(), H2.apply(x).numpy())
    assert np.array_equal(P1.apply(x).numpy(), P2.apply(x).numpy())
    # the same through the Armijo chain
    prob.reweight(None, "l2", 1.0, info=False)
    ga = prob.gradient(R)
    _, Ra, _ = prob.armijo_trial(R, ga, 0.05)
    prob.reweight(Ra, "geman_mcclure", 0.5, info=False)
    fresh = _problem(ctx, c, prob.weights())
    assert np.array_equal(prob.gradient(Ra).numpy(), fresh.gradient(ctx.upload(Ra.numpy())).numpy())
    # a least-squares view and a scaling first asked for AFTER a reweighting
    Rh = Ra.numpy()
    a, b = _outputs(ctx, prob, c, Rh), _outputs(ctx, fresh, c, Rh)
    print(name, "first use after a reweighting, largest error in units of eps:", _compare(a, b, name))


def _first_use_problem():
    """N = 70: two slices, the second with 6 live lanes and 58 padding lanes; a ring over every node but one (isolated),
    60 chords, one zero-weight edge; noisy rotation measurements, weights in [0.5, 2]; a point off the truth"""
    from types import SimpleNamespace
    N, iso = 70, 33
    rng = np.random.Generator(np.random.PCG64(70))

    def rot(v):
        t = np.linalg.norm(v, axis=-1)[..., None, None]
        K = np.zeros(v.shape[:-1] + (3, 3))
        K[..., 0, 1], K[..., 0, 2], K[..., 1, 2] = -v[..., 2], v[..., 1], -v[..., 0]
        K = K - np.swapaxes(K, -1, -2)
        return np.eye(3) + np.sin(t) / t * K + (1 - np.cos(t)) / t ** 2 * (K @ K)

    nodes = np.array([i for i in range(N) if i != iso])
    a, b = rng.integers(0, N - 1, size=60), rng.integers(0, N - 1, size=60)
    b = np.where(a == b, (b + 1) % (N - 1), b)
    ei = np.concatenate([nodes, nodes[a]]).astype(np.int32)
    ej = np.concatenate([np.roll(nodes, -1), nodes[b]]).astype(np.int32)
    truth = rot(rng.normal(size=(N, 3)))
    Rt = np.swapaxes(truth[ei], 1, 2) @ truth[ej] @ rot(0.05 * rng.normal(size=(ei.size, 3)))
    w = rng.uniform(0.5, 2.0, size=ei.size)
    w[17] = 0.0
    R = truth @ rot(0.2 * rng.normal(size=(N, 3)))
    return SimpleNamespace(N=N, ei=ei, ej=ej, Rt=Rt.reshape(-1, 9), w=w, R=R)


def _views(ctx, prob, c, R):
    """(exact, close) as _compare takes them: f and the gradient of a fresh model; F, dF x, dF* y, the scaling of ones"""
    rng = np.random.Generator(np.random.PCG64(71))
    x, y = rng.normal(size=3 * c.N), rng.normal(size=9 * c.ei.size)
    close = {"residual": (prob.residual(R).numpy(), 9)}
    dF, dFt = prob.jacobian(R)
    close["dF"] = (dF.apply(ctx.upload(x)).numpy(), 9)
    close["dFt"] = (dFt.apply(ctx.upload(y)).numpy(), 3)
    close["gn_scaling"] = (prob.gn_scaling().apply(ctx.upload(np.ones(3 * c.N))).numpy(), 3)
    exact = {"objective": np.array([prob.objective(R)]), "gradient": prob.model(R)[0].numpy()}
    return exact, close


def test_first_use_order_does_not_change_a_reweighted_problem(ctx):
    """The rule behind (d): whichever of the least-squares views, the scaling and the reweighting is asked for first, the
    views are those of the weights in force.  A: reweight -> residual -> jacobian -> gn_scaling; B: gn_scaling -> jacobian
    -> residual -> reweight at the same point, then the views again; C: a fresh problem with A's weights.
    A against B bit for bit: both orders end in the same kernels on the same device weights (so it was before the
    first-use paths became one function per resource: the commit before gives equal bits in every quantity).  Against C
    the bar of (b): the host and the device sum degw in different orders.  The reweighting waits for the host as often in
    either order (never without info)."""
    c = _first_use_problem()
    R = ctx.upload(c.R.ravel())
    A = _problem(ctx, c)
    n0 = ctx.sync_count()
    A.reweight(R, "cauchy", 0.5, info=False)
    syncs_a = ctx.sync_count() - n0
    va = _views(ctx, A, c, R)
    B = _problem(ctx, c)
    B.gn_scaling()
    B.jacobian(R)
    B.residual(R)
    n0 = ctx.sync_count()
    B.reweight(R, "cauchy", 0.5, info=False)
    syncs_b = ctx.sync_count() - n0
    vb = _views(ctx, B, c, R)
    print("host waits of the reweighting call: first use", syncs_a, "everything there", syncs_b)
    assert syncs_a == 0 and syncs_b == 0
    w = A.weights()
    assert np.array_equal(w, B.weights()) and w[17] == 0.0 and not np.array_equal(w, c.w)
    _compare(va, vb, "A against B", bitwise_close=True)
    Cp = _problem(ctx, c, w)
    vc = _views(ctx, Cp, c, R)
    print("against a fresh problem, largest error in units of eps:", _compare(va, vc, "A against C"), _compare(vb, vc, "B against C"))
    info = A.info()
    assert info["nslices"] == 2 and info["nnzb"] == 2 * c.ei.size


def test_no_host_wait_without_info(ctx):
    """(f)"""
    c = rr.variant("ring_chords_1500:outliers")
    prob = _problem(ctx, c)
    R = ctx.upload(c.R.ravel())
    prob.reweight(R, "huber", 0.5, info=False)        # the first call uploads
    n0 = ctx.sync_count()
    prob.reweight(R, "cauchy", 0.5, info=False)
    prob.reweight(None, "l2", 1.0, info=False)
    assert ctx.sync_count() == n0
    prob.reweight(R, "geman_mcclure", 0.5, info=True)
    assert ctx.sync_count() == n0 + 1


def test_refused_calls_leave_the_weights_untouched(ctx):
    """(g)"""
    from optimization_amd import capi
    c = rr.variant("ring_chords_1500:outliers")
    prob = _problem(ctx, c)
    R = ctx.upload(c.R.ravel())
    prob.reweight(R, "huber", 0.5, info=False)
    w = prob.weights()
    other = capi.Context(0)
    try:
        bad = [(R, 4, 0.5), (R, -1, 0.5), (R, "huber", 0.0), (R, "cauchy", -1.0), (R, "geman_mcclure", float("nan")),
               (R, "huber", float("inf")), (ctx.upload(np.zeros(9 * c.N - 9)), "huber", 0.5),
               (other.upload(c.R.ravel()), "huber", 0.5), (None, "huber", 0.5)]
        for Rv, kind, s in bad:
            with pytest.raises(capi.MiError) as e:
                prob.reweight(Rv, kind, s)
            assert e.value.status == 1, (kind, s)
            assert np.array_equal(prob.weights(), w), (kind, s)
    finally:
        other.close()
    # a context with a communicator, as the least-squares view refuses it
    sharded = capi.Context(0)
    try:
        sharded.set_option("FORCE_UNIFORM_GRID", 1)
        sharded.comm_init(1, 0, sharded.comm_unique_id())
        p2 = _problem(sharded, c)
        R2 = sharded.upload(c.R.ravel())
        with pytest.raises(capi.MiError) as e:
            p2.reweight(R2, "huber", 0.5)
        assert e.value.status == 1 and "single-context" in str(e.value)
        assert np.array_equal(p2.weights(), c.w)
        del p2
        sharded.comm_finalize()
    finally:
        sharded.close()


def test_no_edges(ctx):
    c = sc.tiny(1)
    prob = _problem(ctx, c)
    info = prob.reweight(ctx.upload(c.R.ravel()), "huber", 0.5)
    assert info == dict(robust_cost=0.0, weighted_cost=0.0, outliers=0) and prob.weights().size == 0
