"""Joint pose-graph refinement at the cfg3 graph (workloads.pose_graph, N = 5e5, E = 1.5e6 by default): the model assembly,
one joint Hessian-vector product, the fused inner iteration and one TNT outer iteration, and -- for scale, in the same
process, alternating with the joint product -- k_bsr3_spmv on the rotation half (mi_so3n's Hessian) and the p = 3 CSR
product on the translation half (mi_pgo_trans's Laplacian).  The joint product streams both matrices plus the coupling
blocks, so the sum of those two is the floor to read it against.

    python tools/bench_pgo.py [--n 500000] [--reps 200] [--rounds 5] [--out FILE.json]

Times of passes: event pairs around `reps` back-to-back launches (mi_timer_start / mi_timer_stop), `rounds` times, all
rounds reported (sorted).  Times of solves: a host clock around work that ends in a device synchronisation.  Bytes are
algorithmic, from the shapes (header comment of optimization_amd/csrc/pgo.hip), with the padded slot count of the layout.
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optimization_amd import capi, workloads as wl  # noqa: E402

HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500000)
    ap.add_argument("--reps", type=int, default=200)   # (event windows of 9 ms and more)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N = a.n
    ei, ej, Rt, _, R_true, _ = wl.pose_graph(N)
    ei64, ej64 = ei.astype(np.int64), ej.astype(np.int64)
    E = ei.size
    rng = np.random.Generator(np.random.PCG64(11))
    t_true = rng.normal(size=(N, 3)) * 10
    tt = np.einsum("eba,eb->ea", R_true.reshape(N, 3, 3)[ei64], t_true[ej64] - t_true[ei64]) + 0.02 * rng.normal(size=(E, 3))
    kappa, tau = np.ones(E), np.linspace(0.5, 2.0, E)
    # the point: the truth itself -- with noisy measurements (0.05 rad, 0.02 length units) a point near the optimum with a
    # gradient of the noise's size and a positive definite Hessian off the gauge, which is where TNT spends its inner iterations
    x0 = np.concatenate([R_true.ravel(), t_true.ravel()])
    ctx = capi.Context(0)
    L = ctx.L
    P = capi.Pgo(ctx, N, ei, ej, Rt, tt, kappa, tau)
    S = capi.So3N(ctx, N, ei, ej, Rt, kappa)
    T = capi.PgoTranslations(ctx, N, ei, ej, tt, tau, 0)
    x = ctx.upload(x0)
    info = P.info()
    padded = info["padded"]

    def events(fn, reps):
        fn()
        ctx.sync()
        ctx.timer_start()
        for _ in range(reps):
            fn()
        return ctx.timer_stop() * 1e3 / reps   # us per call

    def med(v):
        return sorted(v)[len(v) // 2]

    out = {"n": N, "edges": E, "padded_slots": padded, "device": ctx.device_name(), "reps": a.reps, "rounds": a.rounds}
    # the model assembly (into one gradient vector: no allocation inside the timed loop)
    g = ctx.vec(6 * N)
    hop, pc = capi.vp(), capi.vp()

    def model():
        capi.check(L.mi_pgo_model(P.h, x.h, g.h, C.byref(hop), C.byref(pc)))

    model_us = [events(model, a.reps) for _ in range(a.rounds)]
    model_bytes = 116 * padded + 144 * padded + 96 * 2 * E + N * (4 + 96 + 48 + 152 + 144)
    grad_us = [events(lambda: P.gradient(x, out=g), a.reps) for _ in range(a.rounds)]
    g, H, M = P.model(x)
    # the three products, alternating
    eta = ctx.upload(rng.normal(size=6 * N))
    h = ctx.vec(6 * N)
    _, Hs, _ = S.model(x.view(0, 9 * N))
    xi, hs = ctx.upload(rng.normal(size=3 * N)), ctx.vec(3 * N)
    Lt, _ = T.operator()
    de, ht = ctx.upload(rng.normal(size=3 * N)), ctx.vec(3 * N)
    prods = {"hvp_us": lambda: H.apply(eta, out=h), "bsr3_rotation_half_us": lambda: Hs.apply(xi, out=hs),
             "csr3_translation_half_us": lambda: Lt.apply(de, out=ht)}
    times = {k: [] for k in prods}
    for _ in range(a.rounds):
        for k, fn in prods.items():
            times[k].append(events(fn, a.reps))
    hvp_bytes = 160 * padded + 48 * 2 * E + N * (4 + 152 + 48 + 48)
    hvp_med = med(times["hvp_us"])
    out.update(model_us=sorted(model_us), model_bytes=model_bytes, model_GBps=model_bytes / (med(model_us) * 1e-6) / 1e9,
               gradient_only_us=sorted(grad_us), hvp_bytes=hvp_bytes, hvp_GBps=hvp_bytes / (hvp_med * 1e-6) / 1e9,
               hvp_fraction_of_8TBps=hvp_bytes / (hvp_med * 1e-6) / HBM_BYTES_PER_S,
               floor_sum_of_halves_us=med(times["bsr3_rotation_half_us"]) + med(times["csr3_translation_half_us"]))
    out.update({k: sorted(v) for k, v in times.items()})

    # the fused inner iteration: two iteration budgets that the stopping rule does not cut short, the difference per pass
    def solve(iters):
        ctx.sync()
        c0 = time.perf_counter()
        r = ctx.stpcg(g, H, M, Delta=1e150, max_iterations=iters, kappa_fgr=1e-14, theta=0.0)
        ctx.sync()
        return (time.perf_counter() - c0) * 1e6, r["iterations"]

    solve(10)
    per_it = []
    for _ in range(a.rounds):
        (ta, ka), (tb, kb) = solve(10), solve(40)
        if kb > ka:
            per_it.append((tb - ta) / (kb - ka))
    out.update(inner_iteration_us=sorted(per_it), inner_iteration_launches=3)

    # one TNT outer iteration at x with TNT's default inner control (kappa_fgr = 0.1, theta = 0.5) and a radius of 10 that the
    # step does not reach: the model, the inner solve, the trial chain
    def outer():
        ctx.sync()
        c0 = time.perf_counter()
        model()
        r = ctx.stpcg(g, H, M, Delta=10.0, max_iterations=1000, kappa_fgr=0.1, theta=0.5)
        _, t = P.trial(x, r["s"], g, with_precon=True)
        return (time.perf_counter() - c0) * 1e3, r["iterations"], t

    outer()
    outs = [outer() for _ in range(a.rounds)]
    out.update(outer_iteration_ms=sorted(o[0] for o in outs), outer_inner_iterations=int(outs[0][1]),
               outer_trial={k: float(v) for k, v in outs[0][2].items()}, inner_solve_iterations=[int(solve(10)[1]), int(solve(40)[1])])
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
