"""Times mi_so3n_reweight at BASELINE cfg3's size (N = 5e5, E = 1.5e6) next to mi_so3n_residual in the same process (the
same gathers, 72 E more bytes written), and prints one JSON line with the times, the algorithmic bytes of the two new
passes and the GB/s they give.  Warm-up, then the median of `reps` batches of `inner` enqueued calls
between two host waits."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(ctx, fn, warmup, reps, inner):
    for _ in range(warmup):
        fn()
    ctx.sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        ctx.sync()
        ts.append((time.perf_counter() - t0) / inner)
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=500000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    from optimization_amd import capi, workloads as wl
    ei, ej, Rt, w, _, R0 = wl.pose_graph(a.N, seed=3)
    N, E = a.N, len(ei)
    ctx = capi.Context(0)
    prob = capi.So3N(ctx, N, ei, ej, Rt, w)
    R = ctx.upload(np.ascontiguousarray(R0).ravel())
    F = capi.Vec(ctx, 9 * E)
    prob.residual(R, out=F)                              # the least-squares arrays exist: the edge pass also writes sqrt(w)
    prob.gn_scaling()
    sq = prob.info()["sinc_quat"]
    meas = 32 if sq else 72
    edge_bytes = E * (8 + 8 + meas + 144 + 8 + 8)
    node_bytes = 2 * E * (4 + 4 + 8 + 8) + N * (4 + 24)
    res_bytes = E * (16 + meas + 144 + 72)
    out = dict(N=N, E=E, sinc_quat=sq, device=ctx.device_name(), reps=a.reps, inner=a.inner)
    for key, fn in (("reweight_no_info", lambda: prob.reweight(R, "geman_mcclure", 0.5, info=False)),
                    ("residual", lambda: prob.residual(R, out=F))):
        med, best = timed(ctx, fn, a.warmup, a.reps, a.inner)
        out[key + "_us"] = med * 1e6
        out[key + "_best_us"] = best * 1e6
    for _ in range(a.warmup):
        prob.reweight(R, "geman_mcclure", 0.5, info=True)
    ts = []
    for _ in range(a.reps * 4):
        t0 = time.perf_counter()
        prob.reweight(R, "geman_mcclure", 0.5, info=True)
        ts.append(time.perf_counter() - t0)
    out["reweight_with_info_us"] = float(np.median(ts)) * 1e6
    out["reweight_bytes"] = edge_bytes + node_bytes
    out["edge_pass_bytes"], out["node_pass_bytes"], out["residual_bytes"] = edge_bytes, node_bytes, res_bytes
    out["reweight_GBps"] = (edge_bytes + node_bytes) / out["reweight_no_info_us"] / 1e3
    out["residual_GBps"] = res_bytes / out["residual_us"] / 1e3
    print(json.dumps(out))


if __name__ == "__main__":
    main()
