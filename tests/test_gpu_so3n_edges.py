"""GPU parity tests for the SO(3)^N kernels (optimization_amd/csrc/so3.hip) where tests/test_gpu_so3n.py does not
reach: irregular graphs in the SELL-64 incidence layout (a hub beyond the 1024-node window, empty slices, isolated first
and last nodes, N = 1, duplicate and two-way edges, degree 1, a power law), zero / negative / twelve-decade weights, the
rotations on which Shepperd's matrix -> quaternion branch changes sides or ties -- as gathered neighbours and as
measurements in both directions -- the 9-component measurement form, every creation-time switch, the retraction around
its series switch and at 0, pi, 2 pi, and the grid-stride walk of the model assembly.

Every piece is compared with the fp64 oracle AND with the longdouble reference of tests/so3_cases.py.  Bars: 1e-13
(objective, gradient, retraction) and 1e-12 (Hessian, preconditioner) norm-wise, plain.  Two comparisons run at
conftest.floor_or(bar, floor): the objective at N = 2.2e6 (floor: the oracle's sequential sum of 6.6e6 terms against the
longdouble edge loop) and the STPCG step (floor: the re-association floor of conftest.oracle_omp) -- never anything
measured on the device.  Measured: profiles/
so3n_edge_parity.md (SO3N_EDGE_PARITY_LOG=<file> makes the tests append their figures as JSON lines)."""
import contextlib
import json
import os

import numpy as np
import pytest

import so3_cases as sc
from conftest import floor_or, rel_err, trace_close
from optimization_amd import workloads as wl

pytestmark = pytest.mark.gpu

_LOG = os.environ.get("SO3N_EDGE_PARITY_LOG")
_FLOORS = {}


def _record(**kw):
    print("  ".join(f"{k}={v:.2e}" if isinstance(v, float) else f"{k}={v}" for k, v in kw.items()))
    if _LOG:
        with open(_LOG, "a") as f:
            f.write(json.dumps(kw) + "\n")


def _floors(oracle, name):
    if name not in _FLOORS:
        _FLOORS[name] = sc.oracle_vs_reference(oracle, name)
    return _FLOORS[name]


@contextlib.contextmanager
def _form_ctx(form):
    """a context of its own with the form's switches set before the problem is created"""
    from optimization_amd import capi
    c = capi.Context(0)
    try:
        for k, v in sc.FORMS[form].items():
            c.set_option(k, v)
        yield c
    finally:
        c.close()


def _check(case, form, quantity, dev, orc, ref, floor):
    """dev against the oracle's value and the longdouble reference's, both at the plain bar: on every case here the
    oracle is within a third of the bar of the longdouble reference (measured: 3e-15 at most), which is asserted, so that
    an oracle that drifts cannot widen a device bar unseen"""
    bar = sc.bar_of(quantity)
    assert floor_or(bar, floor) == bar, (case, quantity, floor)
    if np.ndim(dev) == 0:
        den = abs(float(ref)) or 1.0
        e_orc, e_ref = abs(dev - orc) / den, float(abs(np.longdouble(dev) - ref) / den)
    else:
        e_orc, e_ref = rel_err(dev, orc), sc.rel_err_ld(dev, ref)
    _record(case=case, form=form, quantity=quantity, dev_vs_oracle=float(e_orc), dev_vs_longdouble=float(e_ref),
            floor=float(floor), bar=float(bar))
    assert e_orc <= bar, (case, form, quantity, "vs oracle", e_orc, bar)
    assert e_ref <= bar, (case, form, quantity, "vs longdouble", e_ref, bar)


# (a) pieces against both references -----------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(sc.FORMS))
@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_so3n_edge_pieces_vs_oracle_and_longdouble(oracle, name, form):
    c, ref, fl = sc.case(name), sc.reference_values(name), _floors(oracle, name)
    x = c.R.ravel()
    sing = np.repeat(sc.singular_nodes(c), 3)
    op = oracle.so3n(c.N, c.ei, c.ej, c.Rt, c.w, precon_kind=1)
    try:
        with _form_ctx(form) as ctx:
            prob = ctx.so3n(c.N, c.ei, c.ej, c.Rt, c.w)
            info = prob.info()
            assert info["gather_quat"] == ("SO3_NO_RQUAT" not in sc.FORMS[form])
            # the 9-component measurement form: forced, or because one measurement is not a rotation
            assert info["sinc_quat"] == ("SO3_NO_QUAT" not in sc.FORMS[form] and name not in sc.NONROT_CASES)
            assert info["nnzb"] == 2 * c.ei.size and info["nslices"] == (c.N + 63) // 64
            R = ctx.upload(c.R)
            _check(name, form, "f", prob.objective(R), oracle.eval_f(op, x), ref["f"], fl["f"])
            g, H, P = prob.model(R)
            _check(name, form, "grad", g.numpy(), oracle.eval_grad(op, x), ref["grad"], fl["grad"])
            for xi, hr in zip(ref["xis"], ref["hess"]):
                hv = H.apply(ctx.upload(xi)).numpy()
                _check(name, form, "hess", hv, oracle.eval_hess(op, x, xi), hr, fl["hess"])
                assert np.all(hv[sing] == 0)       # a node without a (weighted) edge: its rows of H v are exactly 0
            pv = P.apply(ctx.upload(ref["v"])).numpy()
            with np.errstate(all="ignore"):
                po = oracle.eval_precon(op, x, ref["v"])
            assert np.array_equal(np.isfinite(pv), np.isfinite(po)) and np.array_equal(np.isfinite(po), ~sing)
            _check(name, form, "precon", pv[~sing], po[~sing], ref["precon"][~sing], fl["precon"])
            for m in sc.SWEEP:
                xi = ref["sweep"][m]
                Y = prob.retract(R, ctx.upload(xi)).numpy()
                q = f"retract_{m:.17g}"
                _check(name, form, q, Y, oracle.eval_retract(op, x, xi), ref["retract"][m], fl[q])
    finally:
        oracle.free(op)


# (b) Hessian structure ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["default", "no_quat_no_rquat"])
@pytest.mark.parametrize("name", sc.STRUCTURE_CASES)
def test_so3n_edge_hessian_and_preconditioner_are_self_adjoint(name, form):
    c = sc.case(name)
    rng = np.random.default_rng(11)
    with _form_ctx(form) as ctx:
        prob = ctx.so3n(c.N, c.ei, c.ej, c.Rt, c.w)
        g, H, P = prob.model(ctx.upload(c.R))
        u, v = ctx.upload(rng.normal(size=3 * c.N)), ctx.upload(rng.normal(size=3 * c.N))
        Hu, Hv = H.apply(u), H.apply(v)
        a, b = u.dot(Hv), v.dot(Hu)
        assert abs(a - b) <= 1e-11 * max(abs(a), abs(b)), (a, b)
        Pu, Pv = P.apply(u), P.apply(v)
        a, b = u.dot(Pv), v.dot(Pu)
        assert abs(a - b) <= 1e-11 * max(abs(a), abs(b)), (a, b)


# (c) quaternion bit contract ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_precon", [False, True])
def test_so3n_fused_trial_has_the_bits_of_the_separate_calls_on_every_quaternion_branch(ctx, with_precon):
    """test_gpu_so3n.py::test_so3n_fused_trial_step_has_the_bits_of_the_separate_calls at a step whose trial point lies on
    all four branches of mat_to_quat, on exact half turns, on trace 0 and on tied diagonal entries: the quaternion the
    retraction writes (k_so3_retract<true>) must be, bit for bit, the one the conversion pass (k_so3_quat) forms from the
    same matrix -- the contract the comment over mat_to_quat states."""
    c, hh_ = sc.bit_contract_point()
    N = c.N
    prob = ctx.so3n(N, c.ei, c.ej, c.Rt, c.w)
    assert prob.info()["gather_quat"] and prob.info()["sinc_quat"]
    R = ctx.upload(c.R)
    g, H, P = prob.model(R)
    h = ctx.upload(hh_)
    Hh = H.apply(h)
    hh, gh, hHh = ctx.dot_batch([h, g, h], [h, h, Hh])
    Rt_ref = prob.retract(R, h)
    Y = Rt_ref.numpy().reshape(N, 3, 3)
    branch = np.array([sc.device_branch(Yi) for Yi in Y])
    tr = Y[:, 0, 0] + Y[:, 1, 1] + Y[:, 2, 2]
    assert all((branch == b).sum() >= 40 for b in range(4)), np.bincount(branch)
    assert (tr == 0).sum() >= 1 and ((tr > 0) & (tr < 1e-14)).sum() >= 1 and ((tr < 0) & (tr > -1e-14)).sum() >= 1
    assert ((branch > 0) & (Y[:, 0, 0] == Y[:, 1, 1]) & (Y[:, 0, 0] >= Y[:, 2, 2])).sum() >= 1     # tied largest entries
    assert np.all(Y[10] == np.eye(3))
    f_ref = prob.objective(Rt_ref)
    Rtr, t = prob.trial(R, h, g, with_precon=with_precon)
    assert np.array_equal(Rtr.numpy(), Rt_ref.numpy())
    assert (t["f"], t["hh"], t["gh"], t["hHh"]) == (f_ref, hh, gh, hHh)
    g2, H2, P2 = prob.model(Rtr)      # swaps the speculative model in
    prob2 = ctx.so3n(N, c.ei, c.ej, c.Rt, c.w)
    g2_ref, H2_ref, P2_ref = prob2.model(Rt_ref)
    assert np.array_equal(g2.numpy(), g2_ref.numpy())
    assert t["grad_sqnorm"] == g2_ref.dot(g2_ref)
    if with_precon:
        Pg = P2_ref.apply(g2_ref)
        assert t["precon_grad_sqnorm"] == Pg.dot(Pg)
    else:
        assert t["precon_grad_sqnorm"] == -1.0
    v = ctx.upload(np.random.default_rng(5).normal(size=3 * N))
    assert np.array_equal(H2.apply(v).numpy(), H2_ref.apply(v).numpy())
    assert np.array_equal(P2.apply(v).numpy(), P2_ref.apply(v).numpy())
    # (without the preconditioner: this far from a minimiser the blocks D_i are indefinite, and a solve in their "norm"
    # is NaN on either model)
    r1 = ctx.stpcg(g2, H2, None, Delta=10.0, max_iterations=8, kappa_fgr=1e-10, theta=1.0)
    r2 = ctx.stpcg(g2_ref, H2_ref, None, Delta=10.0, max_iterations=8, kappa_fgr=1e-10, theta=1.0)
    assert np.isfinite(r1["s"].numpy()).all() and np.array_equal(r1["s"].numpy(), r2["s"].numpy())


# (d) fused STPCG on irregular graphs ----------------------------------------------------------------------------------
@pytest.mark.parametrize("precon", [False, True])
@pytest.mark.parametrize("name", ["hub_first_linspace", "multigraph_linspace"])
def test_so3n_edge_fused_stpcg_vs_oracle(ctx, oracle, oracle_omp, name, precon):
    c = sc.case(name)      # the point is the truth perturbed by 0.2, as in workloads.pose_graph
    x = c.R.ravel()
    prob = ctx.so3n(c.N, c.ei, c.ej, c.Rt, c.w)
    op = oracle.so3n(c.N, c.ei, c.ej, c.Rt, c.w, precon_kind=1 if precon else 0)
    mp = oracle_omp.so3n(c.N, c.ei, c.ej, c.Rt, c.w, precon_kind=1 if precon else 0) if oracle_omp is not None else None
    try:
        g, H, P = prob.model(ctx.upload(c.R))
        go = oracle.eval_grad(op, x)
        if mp is not None:
            oracle_omp.eval_grad(mp, x)      # (binds the model to the point; the floor solves take the oracle's g too)
        # a solve that ends inside the region (residual exit after 9 ... 19 iterations; on the multigraph without the
        # preconditioner a boundary exit after 16) and one that the region cuts short.  (Solved to 1e-8 these problems end
        # in the gauge directions of f -- global rotations, curvature 0 -- which no implementation determines: the
        # re-associated reference itself is then 1e-4 from the sequential one on the hub.)
        for Delta, kappa in ((1e3, 1e-3), (100.0 if precon else 12.0, 1e-5)):
            kw = dict(max_iterations=60, kappa_fgr=kappa, theta=.5, trace_cap=64)
            r = ctx.stpcg(g, H, P if precon else None, Delta=Delta, **kw)
            o = oracle.stpcg_problem(op, x, go, Delta, **kw)
            floors = []
            if mp is not None:
                for t in (2, 3, 4):
                    oracle_omp.set_threads(t)
                    floors.append(oracle_omp.stpcg_problem(mp, x, go, Delta, **kw))
            fl_s = max(rel_err(f["s"], o["s"]) for f in floors) if floors else 0.0
            es = rel_err(r["s"].numpy(), o["s"])
            _record(case=name, form="precon" if precon else "plain", quantity=f"stpcg_step_Delta={Delta:g}",
                    dev_vs_oracle=float(es), floor=float(fl_s), bar=float(floor_or(1e-10, fl_s)),
                    iterations=int(o["iterations"]), exit_reason=int(o["exit_reason"]))
            assert r["iterations"] == o["iterations"] and r["exit_reason"] == o["exit_reason"]
            for key in ("alpha", "beta"):
                assert len(r["trace"][key]) == len(o["trace"][key])
                if not len(o["trace"][key]):
                    continue
                ok, msg = trace_close(r["trace"][key], o["trace"][key],
                                      [f["trace"][key] for f in floors] if floors else None, 1e-9)
                assert ok, f"{name} Delta = {Delta} {key}: {msg}"
            assert es <= floor_or(1e-10, fl_s), (es, fl_s)
    finally:
        oracle.free(op)
        if mp is not None:
            oracle_omp.set_threads(4)
            oracle_omp.free(mp)


# (e) beyond the assembly's grid cap -----------------------------------------------------------------------------------
def test_so3n_model_assembly_beyond_its_grid_cap(ctx, oracle):
    """N = 2 200 000: more groups of 4 slices than the 8 x 1024 workgroups the model assembly launches at most, so every
    workgroup walks more than one group (the grid-stride loop of k_so3_model) and the objective partials fill all 8
    components.  The only test that does."""
    N = 2_200_000
    assert -(-N // 256) > 8 * 1024
    ei, ej, Rt, w, _, Rinit = wl.pose_graph(N, seed=11)
    w = np.linspace(0.5, 1.5, w.size)
    prob = ctx.so3n(N, ei, ej, Rt, w)
    info = prob.info()
    assert info["model_grid"] == 8 * 1024 < -(-info["nslices"] // 4)
    op = oracle.so3n(N, ei, ej, Rt, w, precon_kind=1)
    try:
        x = Rinit.ravel()
        R = ctx.upload(Rinit)
        f, fo = prob.objective(R), oracle.eval_f(op, x)
        # the floor of the objective: the oracle's sequential sum of 6.6e6 terms against the longdouble edge loop
        fr = sc.So3Ref(sc.Case("big", N, ei, ej, Rt, w, Rinit)).f()
        floor = float(abs(np.longdouble(fo) - fr) / fr)
        bar = floor_or(sc.TOL_F, floor)
        _record(case="pose_graph_2200000", form="default", quantity="f", dev_vs_oracle=abs(f - fo) / fo,
                dev_vs_longdouble=float(abs(np.longdouble(f) - fr) / fr), floor=floor, bar=bar)
        assert abs(f - fo) <= bar * fo and abs(np.longdouble(f) - fr) <= bar * fr
        g, H, P = prob.model(R)
        rng = np.random.default_rng(2)
        xi, v = rng.normal(size=3 * N), rng.normal(size=3 * N)
        for q, dev, orc, tol in (("grad", g.numpy(), oracle.eval_grad(op, x), sc.TOL_G),
                                 ("hess", H.apply(ctx.upload(xi)).numpy(), oracle.eval_hess(op, x, xi), sc.TOL_H),
                                 ("precon", P.apply(ctx.upload(v)).numpy(), oracle.eval_precon(op, x, v), sc.TOL_P)):
            e = rel_err(dev, orc)
            _record(case="pose_graph_2200000", form="default", quantity=q, dev_vs_oracle=float(e), floor=0.0, bar=tol)
            assert e < tol, (q, e)
        # the fused trial step's objective comes from the assembly's own pass over the trial point: the same walk
        h = ctx.upload(1e-2 * rng.normal(size=3 * N))
        f_sep = prob.objective(prob.retract(R, h))
        _, t = prob.trial(R, h, g)
        assert t["f"] == f_sep
    finally:
        oracle.free(op)
