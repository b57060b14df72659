"""The joint pose-graph problem on the device (optimization_amd/csrc/pgo.hip, capi.Pgo) against the longdouble restatement of
tests/pgo_cases.py (held against finite differences by test_cpu_pgo_fd.py), against the existing stages, and form against
form.

Bars.  Objective, gradient, retraction and every written block: the project's bar for pieces, so3_cases.TOL_G = 1e-13 relative,
widened only by the restatement's own float64 distance from its longdouble figures where it has one (objective, gradient:
logged; its rotation term stays in longdouble, so the widening is that of the translation term alone).  H eta and the three
curvature dots: TOL_H = 1e-12, flat.  Inverse blocks times their blocks: the identity to 1e-12 where a block has an inverse."""
import numpy as np
import pytest

import pgo_cases as pc
from so3_cases import LD, TOL_G, TOL_H

pytestmark = pytest.mark.gpu


def make(ctx, name):
    from optimization_amd import capi
    p = pc.problem(name)
    return p, capi.Pgo(ctx, p["N"], p["ei"], p["ej"], p["Rt"], p["tt"], p["kappa"], p["tau"]), ctx.upload(p["x"])


def rel(a, ref):
    """relative to the reference, or absolute where the reference is exactly zero (no edges, a weight pattern of zeros)"""
    ref = np.asarray(ref, dtype=LD)
    return pc.rel_ld(a, ref) if np.any(ref != 0) else float(np.abs(np.asarray(a)).max(initial=0.0))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name", pc.GPU_CASES)
def test_passes_against_longdouble(ctx, name):
    p, P, x = make(ctx, name)
    N = p["N"]
    ref = pc.reference_values(name)
    floor = ref["floor"]
    lay = ref["lay"]
    info = P.info()
    assert (info["nslices"], info["nnzb"], info["padded"]) == (lay["nslices"], lay["nnzb"], lay["padded"])
    f = P.objective(x)
    g, H, M = P.model(x)
    gn = g.numpy()
    ferr, gerr = rel([f], [ref["f"]]), rel(gn, ref["grad"])
    print(f"{name}: f {ferr:.2e} ({floor['f']:.2e}), grad {gerr:.2e} ({floor['grad']:.2e})")
    assert ferr <= TOL_G + floor["f"] and gerr <= TOL_G + floor["grad"]
    # every written block
    B, G, Nsl, Minv, acted = ref["blocks"]
    got = {k: P.blocks(k) for k in ("Bblk", "Gblk", "Nsl", "Minv")}
    pad9 = 9 * lay["padded"]
    berr, gerr2, nerr = rel(got["Bblk"], B[:pad9]), rel(got["Gblk"], G[:pad9]), rel(got["Nsl"], Nsl)
    print(f"    blocks: kappa B {berr:.2e}, G {gerr2:.2e}, node blocks {nerr:.2e}")
    assert berr <= TOL_G and gerr2 <= TOL_G and nerr <= TOL_G
    assert np.all(got["Bblk"][B[:pad9] == 0] == 0) and np.all(got["Gblk"][G[:pad9] == 0] == 0), "a padding block is not zero"
    # the inverse blocks times their blocks, where the safeguard did not act; the identity where it did
    Mi = got["Minv"].reshape(N, 2, 3, 3)
    Hxx = np.zeros((N, 3, 3))
    degt = np.zeros(N)
    for l, node in enumerate(lay["perm"]):
        if node >= 0:
            s, lane = l // 64, l % 64
            Hxx[node] = got["Nsl"][(s * 19 + np.arange(9)) * 64 + lane].reshape(3, 3)
            degt[node] = got["Nsl"][(s * 19 + 18) * 64 + lane]
    act = acted.reshape(N, 2)
    eye = np.eye(3)
    assert np.all(Mi[act[:, 0], 0] == eye) and np.all(Mi[act[:, 1], 1] == eye)
    ok0, ok1 = ~act[:, 0], ~act[:, 1]
    if ok0.any():
        d = np.abs(Mi[ok0, 0].astype(LD) @ Hxx[ok0].astype(LD) - eye).max()
        print(f"    inverse blocks: max |M H - I| {float(d):.2e} (cond up to {np.linalg.cond(Hxx[ok0]).max():.1e})")
        assert d <= 1e-12
    if ok1.any():
        assert np.abs(Mi[ok1, 1] * degt[ok1, None, None] - eye).max() <= 1e-12
    # H eta; the three curvature dots of the fused pass k_pgo_hvp<true>, read back from its partial rows (hvp_dots); and two of
    # them once more as a solve sees them (one unpreconditioned STPCG pass from g = eta: p = -eta, kappa_0 = <eta, H eta>,
    # alpha_0 kappa_0 = <r, r> = <eta, eta>)
    for eta, href in zip(ref["etas"], ref["hess"]):
        e = ctx.upload(eta)
        h1, h2 = H.apply(e).numpy(), H.apply(e).numpy()
        herr = rel(h1, href)
        assert np.array_equal(bits(h1), bits(h2)), "two launches of the Hessian pass differ"
        want_k, want_rv, want_hh = (eta.astype(LD) * href).sum(), (eta.astype(LD) ** 2).sum(), (href * href).sum()
        hd, (d_eh, d_hh, d_ee) = P.hvp_dots(e)
        assert np.array_equal(bits(hd.numpy()), bits(h1)), "the pass with the dots writes another H eta"
        assert abs(LD(d_ee) - want_rv) <= TOL_H * want_rv
        if want_k == 0:    # (no edge: H = 0, no solve to take the dots from)
            assert np.all(h1 == 0)
            continue
        r = ctx.stpcg(e, H, None, Delta=1e150, max_iterations=1, kappa_fgr=1e-10, theta=1.0, trace_cap=4)
        kerr = float(abs(LD(r["trace"]["kappa"][0]) - want_k) / abs(want_k))
        rverr = float(abs(LD(r["trace"]["alpha"][0]) * LD(r["trace"]["kappa"][0]) - want_rv) / want_rv)
        derr = [float(abs(LD(a) - w) / abs(w)) for a, w in ((d_eh, want_k), (d_hh, want_hh), (d_ee, want_rv))]
        print(f"    H eta {herr:.2e}; dots <eta,h> {derr[0]:.2e}, <h,h> {derr[1]:.2e}, <eta,eta> {derr[2]:.2e}; "
              f"in a solve <eta, H eta> {kerr:.2e}, <eta, eta> {rverr:.2e}")
        assert herr <= TOL_H and max(derr) <= TOL_H and kerr <= TOL_H and rverr <= TOL_H
    # the retraction (a step of 0.3 rad / 0.3 length units per node)
    y = P.retract(x, ctx.upload(ref["etas"][0])).numpy()
    yerr = rel(y, ref["retract"])
    print(f"    retraction {yerr:.2e}")
    assert yerr <= TOL_G


def test_retraction_across_the_series_switch(ctx):
    """|xi_i| on both sides of and at 1e-4, 0, pi and a large angle, node by node"""
    import so3_cases as sc
    p, P, x = make(ctx, "ring65")
    N = p["N"]
    rng = np.random.Generator(np.random.PCG64(5))
    ax = rng.normal(size=(N, 3))
    ax /= np.linalg.norm(ax, axis=1)[:, None]
    eta = np.zeros((N, 6))
    eta[:, :3] = ax * np.resize(np.array(sc.SWEEP), N)[:, None]
    eta[:, 3:] = rng.normal(size=(N, 3))
    y = P.retract(x, ctx.upload(eta.ravel())).numpy()
    assert pc.rel_ld(y, pc.PgoRef(p).retract(eta.ravel())) <= TOL_G
    zero = np.flatnonzero(np.resize(np.array(sc.SWEEP), N) == 0.0)
    assert np.array_equal(y[:9 * N].reshape(N, 9)[zero], p["x"][:9 * N].reshape(N, 9)[zero]), "exp(0) is not the identity"


@pytest.mark.parametrize("name", ("ring300_tau0", "multigraph130_tau0"))
def test_without_translation_weights_it_is_rotation_averaging(ctx, name):
    from optimization_amd import capi
    p, P, x = make(ctx, name)
    N = p["N"]
    S = capi.So3N(ctx, N, p["ei"], p["ej"], p["Rt"], p["kappa"])
    R = x.view(0, 9 * N)
    gs, _, _ = S.model(R)
    fs = S.objective(R)
    g = P.gradient(x).numpy().reshape(N, 6)
    f = P.objective(x)
    print(f"{name}: f {abs(f - fs) / abs(fs):.2e}, grad {pc.rel_ld(g[:, :3], gs.numpy()):.2e}")
    assert abs(f - fs) <= TOL_G * abs(fs) and pc.rel_ld(g[:, :3], gs.numpy()) <= TOL_G
    assert np.all(g[:, 3:] == 0)


def test_without_rotation_weights_the_delta_rows_are_the_graph_laplacian(ctx):
    """kappa = 0 and xi = 0: the delta rows of H eta are the UNANCHORED tau-weighted Laplacian applied to delta (edge by edge
    in longdouble), and the same view of the point goes through mi_pgo_trans_residual without a copy"""
    from optimization_amd import capi
    p, P, x = make(ctx, "ring65_kappa0")
    N, ei, ej, tau = p["N"], p["ei"], p["ej"], p["tau"].astype(LD)
    _, H, _ = P.model(x)
    rng = np.random.Generator(np.random.PCG64(8))
    eta = np.zeros((N, 6))
    eta[:, 3:] = rng.normal(size=(N, 3))
    h = H.apply(ctx.upload(eta.ravel())).numpy().reshape(N, 6)
    d = tau[:, None] * (eta[ej, 3:].astype(LD) - eta[ei, 3:].astype(LD))
    want = np.zeros((N, 3), dtype=LD)
    np.add.at(want, ej, d)
    np.add.at(want, ei, -d)
    assert pc.rel_ld(h[:, 3:], want) <= TOL_H
    T = capi.PgoTranslations(ctx, N, ei, ej, p["tt"], p["tau"], 0)
    _, ft, _ = T.residual(x.view(0, 9 * N), x.view(9 * N, 3 * N), with_vector=False)
    f = P.objective(x)
    assert abs(f - ft) <= TOL_G * abs(ft)


@pytest.mark.parametrize("name", ("n1", "n2", "ring65", "ring300_tau7", "hub_last200", "hub_last1500", "isolated70"))
def test_forms_agree_bit_for_bit(ctx, name):
    p, P, x = make(ctx, name)
    ref = pc.reference_values(name)
    f1, f2 = P.objective(x), P.objective(x)
    g_model, H, M = P.model(x)
    g_grad, g_grad2 = P.gradient(x).numpy(), P.gradient(x).numpy()
    assert f1 == f2 and np.array_equal(bits(g_grad), bits(g_grad2)), "the same input twice gives other bits"
    assert np.array_equal(bits(g_model.numpy()), bits(g_grad)), "the gradient-only form differs from the model form"
    blocks1 = {k: P.blocks(k) for k in ("Bblk", "Gblk", "Nsl", "Minv")}
    g_again, _, _ = P.model(x)
    assert np.array_equal(bits(g_again.numpy()), bits(g_model.numpy()))
    for k, v in blocks1.items():
        assert np.array_equal(bits(P.blocks(k)), bits(v)), k
    # the trial chain against the separate calls
    h = ctx.upload(0.1 * ref["etas"][1])
    for with_precon in (True, False):
        xt, t = P.trial(x, h, g_model, with_precon=with_precon)
        Hh = H.apply(h)
        y = P.retract(x, h)
        assert np.array_equal(bits(xt.numpy()), bits(y.numpy()))
        gt = P.gradient(y)
        sep = dict(f=P.objective(y), hh=h.dot(h), gh=g_model.dot(h), hHh=h.dot(Hh), grad_sqnorm=gt.dot(gt))
        for k, v in sep.items():
            assert t[k] == v, (k, t[k], v)
        if with_precon:
            # M at the trial point: the model there (which rebinds the operator: it comes last)
            Mt_blocks = P.blocks("Minv_trial")
            gy, Hy, My = P.model(y)
            assert np.array_equal(bits(gy.numpy()), bits(gt.numpy()))
            assert np.array_equal(bits(P.blocks("Minv")), bits(Mt_blocks)), "the inverse blocks of the trial chain differ"
            Pg = My.apply(gy)
            assert t["precon_grad_sqnorm"] == Pg.dot(Pg)
            g_model, H, M = P.model(x)
        else:
            assert t["precon_grad_sqnorm"] == -1.0
    # the objective-only form gives the bits of the sum the trial chain takes from the gradient form
    assert f1 == P.objective(x)


def test_entry_points_refuse_what_they_must(ctx):
    from optimization_amd import capi
    p, P, x = make(ctx, "n2")
    g, H, M = P.model(x)
    h = ctx.upload(np.zeros(12))
    other = ctx.upload(p["x"])
    with pytest.raises(capi.MiError, match="not bound to this x"):
        P.trial(other, h, g)
    with pytest.raises(capi.MiError, match="12N doubles"):
        P.objective(ctx.upload(np.zeros(9 * p["N"])))
    with pytest.raises(capi.MiError, match="6N doubles"):
        P.retract(x, ctx.upload(np.zeros(3 * p["N"])))
    with pytest.raises(capi.MiError, match="negative or non-finite weight"):
        capi.Pgo(ctx, 2, p["ei"], p["ej"], p["Rt"], p["tt"], p["kappa"], -p["tau"] - 1)


def test_a_context_with_a_communicator_is_refused():
    """single-context only: a context that carries a communicator (hence the uniform grid) gets no joint problem"""
    from optimization_amd import capi
    p = pc.problem("n2")
    sharded = capi.Context(0)
    try:
        sharded.set_option("FORCE_UNIFORM_GRID", 1)
        sharded.comm_init(1, 0, sharded.comm_unique_id())
        with pytest.raises(capi.MiError) as e:
            capi.Pgo(sharded, p["N"], p["ei"], p["ej"], p["Rt"], p["tt"], p["kappa"], p["tau"])
        assert e.value.status == 1 and "single-context" in str(e.value)
        sharded.comm_finalize()
    finally:
        sharded.close()
