"""Pose-graph translations at the cfg3 graph (workloads.pose_graph, N = 5e5 by default): the two passes that depend on R,
the solve, and the route a client had before mi_pgo_trans_* existed -- download R, assemble b on the host with numpy,
upload, the same mi_stpcg on a user-built mi_csr -- alternating with the device route in one process.

    python tools/bench_pgo_trans.py [--n 500000] [--reps 50] [--rounds 5] [--out FILE.json]

Times of passes: event pairs around `reps` back-to-back launches (mi_timer_start / mi_timer_stop).  Times of routes: a host
clock around work that ends in a device synchronisation.  Bytes are algorithmic, from the shapes (header comment of
optimization_amd/csrc/pgo_trans.hip).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from optimization_amd import capi, workloads as wl  # noqa: E402


def host_rhs(N, ei, ej, tt, tau, R, anchor):
    """b(R) with vectorised numpy (bincount per component: the fastest plain-numpy scatter)"""
    v = tau[:, None] * np.einsum("eab,eb->ea", R.reshape(N, 3, 3)[ei], tt)
    b = np.empty((N, 3))
    for c in range(3):
        b[:, c] = np.bincount(ej, weights=v[:, c], minlength=N) - np.bincount(ei, weights=v[:, c], minlength=N)
    b[anchor] = 0
    return b.ravel()


def host_laplacian(N, ei, ej, tau, anchor):
    """the anchored Laplacian as CSR, the way a numpy client builds it (sort + reduceat; every node has an edge here)"""
    keep = (ei != anchor) & (ej != anchor)
    r = np.concatenate([ei[keep], ej[keep], np.arange(N)])
    c = np.concatenate([ej[keep], ei[keep], np.arange(N)])
    deg = np.bincount(ei, weights=tau, minlength=N) + np.bincount(ej, weights=tau, minlength=N)
    deg[anchor] = 1.0
    v = np.concatenate([-tau[keep], -tau[keep], deg])
    key = r.astype(np.int64) * N + c
    order = np.argsort(key, kind="stable")
    key, v = key[order], v[order]
    first = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))
    val = np.add.reduceat(v, first)
    rows, cols = key[first] // N, key[first] % N
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=N))]).astype(np.int32)
    return rowptr, cols.astype(np.int32), val, np.repeat(1.0 / deg, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N = a.n
    ei, ej, _, _, R_true, _ = wl.pose_graph(N)
    ei64, ej64 = ei.astype(np.int64), ej.astype(np.int64)
    E = ei.size
    rng = np.random.Generator(np.random.PCG64(11))
    t_true = rng.normal(size=(N, 3)) * 10
    tt = np.einsum("eba,eb->ea", R_true.reshape(N, 3, 3)[ei64], t_true[ej64] - t_true[ei64]) + 0.02 * rng.normal(size=(E, 3))
    tau = np.linspace(0.5, 2.0, E)
    anchor = 0
    ctx = capi.Context(0)
    T = capi.PgoTranslations(ctx, N, ei, ej, tt, tau, anchor)
    Rd = ctx.upload(R_true.ravel())
    b = ctx.vec(3 * N)

    def events(fn, reps):
        fn()
        ctx.sync()
        ctx.timer_start()
        for _ in range(reps):
            fn()
        return ctx.timer_stop() * 1e3 / reps   # us per call

    out = {"n": N, "edges": E, "device": ctx.device_name(), "tol": a.tol}
    # the two passes
    rhs_us = sorted(events(lambda: T.rhs(Rd, out=b), a.reps) for _ in range(a.rounds))
    t0, info0 = T.solve(Rd, tol=a.tol)
    res_us = sorted(events(lambda: T.residual(Rd, t0, with_vector=False), a.reps) for _ in range(a.rounds))
    resw_us = sorted(events(lambda: T.residual(Rd, t0), 10) for _ in range(a.rounds))
    # algorithmic bytes (the padded slot count is not public: 2E incidences is the lower bound the layout pads by ~5 %)
    rhs_bytes = 40 * 2 * E + 72 * E + 100 * N
    res_bytes = 160 * E
    out.update(rhs_us=rhs_us, rhs_bytes=rhs_bytes, rhs_GBps=rhs_bytes / (rhs_us[len(rhs_us) // 2] * 1e-6) / 1e9,
               residual_us=res_us, residual_bytes=res_bytes,
               residual_GBps=res_bytes / (res_us[len(res_us) // 2] * 1e-6) / 1e9,
               residual_with_vector_us=resw_us, residual_with_vector_bytes=res_bytes + 24 * E)
    # the parent's route, built once (not timed, as mi_pgo_trans_create is not)
    rowptr, col, val, dinv = host_laplacian(N, ei64, ej64, tau, anchor)
    A = ctx.csr(N, rowptr, col, val)
    Lop, P = ctx.op_csr(A, 3), ctx.precon_diag(ctx.upload(dinv))
    Ld, Pd = T.operator()

    def device_route():
        t, info = T.solve(Rd, tol=a.tol)
        return t, info["iterations"]

    def device_pcg_only():
        T.rhs(Rd, out=b)
        r = ctx.stpcg(b.scaled(-1.0), Ld, Pd, Delta=1e150, max_iterations=1000, kappa_fgr=a.tol, theta=0.0)
        return r["s"], r["iterations"]

    def host_route():
        Rh = Rd.numpy()
        g = ctx.upload(-host_rhs(N, ei64, ej64, tt, tau, Rh, anchor))
        r = ctx.stpcg(g, Lop, P, Delta=1e150, max_iterations=1000, kappa_fgr=a.tol, theta=0.0)
        return r["s"], r["iterations"]

    def host_assembly_only():
        Rh = Rd.numpy()
        ctx.upload(-host_rhs(N, ei64, ej64, tt, tau, Rh, anchor))
        ctx.sync()

    routes = {"solve_ms": device_route, "rhs_plus_pcg_ms": device_pcg_only, "host_route_ms": host_route,
              "host_download_assembly_upload_ms": host_assembly_only}
    times = {k: [] for k in routes}
    its = {}
    for fn in routes.values():   # warm-up of every route
        fn()
    for _ in range(a.rounds):    # alternating
        for k, fn in routes.items():
            ctx.sync()
            c0 = time.perf_counter()
            r = fn()
            ctx.sync()
            times[k].append((time.perf_counter() - c0) * 1e3)
            if r is not None:
                its[k] = int(r[1])
    td, th = device_route()[0].numpy(), host_route()[0].numpy()
    out.update({k: sorted(v) for k, v in times.items()})
    out.update(iterations=its, solve_info={k: (v if isinstance(v, str) else float(v)) for k, v in info0.items()},
               routes_rel_diff=float(np.linalg.norm(td - th) / np.linalg.norm(th)),
               position_rms_error=float(np.sqrt(np.mean((td.reshape(N, 3) - (t_true - t_true[anchor])) ** 2))))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
