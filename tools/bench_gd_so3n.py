#!/usr/bin/env python3
"""GradientDescent on SO(3)^N at the cfg3 size (N = 5e5, the pose graph bench.py's cfg3 leg builds), through the C ABI:
the fused Armijo trial (mi_so3n_armijo_trial + mi_so3n_gradient) against the statement sequence a client had to write
before the gradient-only pass existed -- mi_vec_scale_to, mi_so3n_retract, mi_so3n_objective per trial, mi_so3n_model +
mi_vec_dot per accepted point -- alternating in one process.

An "accepted iteration" here is TRIALS Armijo trials (default 2: the mean of tests/golden/gd_so3n.json is 1.5 ... 2.2)
followed by the gradient and its norm at the accepted point.  Both forms do the same trials at the same points.

Also: the gradient-only pass by event pairs (mi_ktime), the pass's algorithmic bytes from
mi_debug_so3n_info and its share of 8 TB/s, and host synchronisations per trial from mi_ctx_sync_count.

Usage: python tools/bench_gd_so3n.py [--n 500000] [--rounds 12] [--iters 10] [--trials 2] [--out profiles/gd_so3n_ab]
Writes <out>.jsonl (one line per round and form, and a summary line) and prints the summary."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from optimization_amd import capi, workloads as wl  # noqa: E402

PEAK_BYTES_PER_S = 8e12


def grad_pass_bytes(info, N):
    """algorithmic bytes of one gradient-only pass: per padded incidence slot the neighbour index (4) and the weight (8);
    per incidence the measurement record (32 as a quaternion, 72 as a matrix) and the gathered neighbour record (32 /
    72); per node R_i in (72) and three doubles out (24)"""
    s = 32 if info["sinc_quat"] else 72
    q = 32 if info["gather_quat"] else 72
    return info["padded"] * 12 + info["nnzb"] * (s + q) + N * (72 + 24)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500_000)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--iters", type=int, default=10, help="accepted iterations per timed window")
    ap.add_argument("--trials", type=int, default=2, help="Armijo trials per accepted iteration")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N = a.n
    ei, ej, Rt, w, _, Rinit = wl.pose_graph(N, seed=7, init_sigma=0.02)
    ctx = capi.Context(0)
    prob = ctx.so3n(N, ei, ej, Rt, w)
    info = prob.info()
    deg = np.zeros(N)
    np.add.at(deg, ei, w)
    np.add.at(deg, ej, w)
    alpha = 1.0 / deg.max()
    R = ctx.upload(Rinit)
    g = prob.gradient(R)
    # work vectors of both forms exist before the clock starts (a DeviceVector client draws them from the pool)
    h, Y, gY = ctx.vec(3 * N), ctx.vec(9 * N), ctx.vec(3 * N)
    L = ctx.L

    def fused(iters):
        for _ in range(iters):
            t = alpha
            for _k in range(a.trials):
                prob.armijo_trial(R, g, t, h=h, R_trial=Y)
                t *= .5
            prob.gradient(Y, out=gY)          # the accepted point: a copy

    def parent_style(iters):
        for _ in range(iters):
            t = alpha
            for _k in range(a.trials):
                capi.check(L.mi_vec_scale_to(h.h, -t, g.h))
                capi.check(L.mi_so3n_retract(prob.h, R.h, h.h, Y.h))
                prob.objective(Y)
                t *= .5
            gm, _, _ = prob.model(Y, with_precon=False)       # the only way to a gradient: the full assembly
            gm.dot(gm)

    def window(fn):
        ctx.sync()
        s0 = ctx.sync_count()
        t0 = time.perf_counter()
        fn(a.iters)
        ctx.sync()
        dt = time.perf_counter() - t0
        return 1e6 * dt / a.iters, (ctx.sync_count() - s0 - 1) / (a.iters * a.trials)

    fused(2)
    parent_style(2)
    rows = []
    for r in range(a.rounds):
        for name, fn in (("fused", fused), ("parent_style", parent_style)) if r % 2 == 0 else \
                (("parent_style", parent_style), ("fused", fused)):
            us, syncs = window(fn)
            rows.append(dict(round=r, form=name, us_per_iteration=us, us_per_trial=us / a.trials, syncs_per_trial=syncs))
    # kernels by event pairs, in windows of their own
    ctx.ktime_enable("so3_grad")
    ctx.ktime_reset()
    fused(a.iters)
    n_g, ms_g = ctx.ktime_read("so3_grad")
    ctx.ktime_enable("so3_grad", False)
    # the full assembly for comparison: host clock around 20 calls, device drained (tools/time_so3_model.py)
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(20):
        prob.model(R, with_precon=False)
    ctx.sync()
    model_us = 1e6 * (time.perf_counter() - t0) / 20
    t0 = time.perf_counter()
    for _ in range(20):
        prob.gradient(R, out=gY)
    ctx.sync()
    grad_call_us = 1e6 * (time.perf_counter() - t0) / 20

    def stat(form, key):
        v = np.array([x[key] for x in rows if x["form"] == form])
        return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))

    gb = grad_pass_bytes(info, N)
    grad_us = 1e3 * ms_g / max(n_g, 1)
    summary = dict(
        summary=True, device=ctx.device_name(), N=N, edges=int(ei.size), info=info, trials_per_iteration=a.trials,
        iterations_per_window=a.iters, rounds=a.rounds,
        fused_us_per_iteration=stat("fused", "us_per_iteration"), fused_us_per_trial=stat("fused", "us_per_trial"),
        parent_style_us_per_iteration=stat("parent_style", "us_per_iteration"),
        parent_style_us_per_trial=stat("parent_style", "us_per_trial"),
        fused_syncs_per_trial=stat("fused", "syncs_per_trial")["median"],
        parent_style_syncs_per_trial=stat("parent_style", "syncs_per_trial")["median"],
        grad_pass_us=grad_us, grad_pass_launches=int(n_g), grad_pass_bytes=int(gb), grad_pass_bytes_per_s=gb / (grad_us * 1e-6) if n_g else None,
        grad_pass_share_of_8TBps=gb / (grad_us * 1e-6) / PEAK_BYTES_PER_S if n_g else None,
        model_call_us=model_us, gradient_call_us=grad_call_us)
    print(json.dumps(summary))
    if a.out:
        with open(a.out + ".jsonl", "w") as f:
            for x in rows:
                f.write(json.dumps(x) + "\n")
            f.write(json.dumps(summary) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
