#!/usr/bin/env python3
"""Side benchmark of the tall-row kernel family (stiefel_tall.hip): St(1e6, p), p = 9, 12, 16, on the 100^3 Laplacian.

Per width, each in a child process of its own with a time limit (the parent starts nothing more after a child that
failed), it records
  * microseconds per STPCG inner iteration of the fused solve (two-pass Hessian, curvature dots in the finish pass),
    with the Gram rows reduced by the one-workgroup kernel ("reduce", the default) and re-reduced in the consumers'
    prologue ("prologue", MI355OPT_TALL_PROLOGUE=1);
  * microseconds of the sparse-product + Gram kernel, the reduce kernel and the finish kernel (event pairs);
  * the Hessian step's compulsory bytes and its fraction of 8 TB/s;
  * microseconds per iteration of the GENERIC loop a client has without the family: the same recurrence driven from the
    host, one kernel per vector statement, one synchronising inner product each, the operator mi_csr_spmm followed by
    mi_stiefel_project.
It writes profiles/tall_rows.jsonl and profiles/tall_rows.md.
Usage: python tools/bench_tall_rows.py [--nx 100] [--p 9 12 16] [--iters 50]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 8e12  # bytes / s


def child(nx, p, iters):
    import numpy as np
    from optimization_amd import capi, workloads as wl
    n = nx ** 3
    c = capi.Context(0)
    rowptr, col, val = wl.laplacian_3d(nx, nx, nx)
    A = c.csr(n, rowptr, col, val)
    prob = c.stiefel_rq(A, n, p)
    X = c.upload(wl.stiefel_bench_iterate(nx, nx, nx, p, eps=1e-3, seed=7)[0])
    g, H = prob.model(X)
    s = c.vec(n * p)
    kw = dict(Delta=1e3, max_iterations=iters, kappa_fgr=1e-12, theta=1.0, s_out=s)
    for _ in range(3):   # warm-up: clocks, code objects, pools
        c.stpcg(g, H, **kw)
    ts, its = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        r = c.stpcg(g, H, **kw)
        ts.append(time.perf_counter() - t0)
        its.append(r["iterations"])
    names = ("stiefel_spmm_gram", "stiefel_gram_reduce", "stiefel_finish_dots")
    for k in names:
        c.ktime_enable(k, True)
    c.ktime_reset()
    for _ in range(2):
        c.stpcg(g, H, **kw)
    kus = {}
    for k in names:
        cnt, ms = c.ktime_read(k)
        kus[k] = 1e3 * ms / cnt if cnt else 0.0
        c.ktime_enable(k, False)
    # the generic loop: CG recurrence from the host, a synchronising inner product each, operator from public pieces
    def op(v):
        return c.stiefel_project(n, p, X, A.spmm(p, v))
    def generic(k):
        r_ = g.copy()
        d = g.scaled(-1.0)
        sg = c.vec(n * p).fill(0.0)
        rr = r_.dot(r_)
        for _ in range(k):
            Hd = op(d)
            dHd = d.dot(Hd)
            alpha = rr / dHd
            sg.axpy(alpha, d)
            r_.axpy(alpha, Hd)
            rr_new = r_.dot(r_)
            d.axpby(-1.0, r_, rr_new / rr, d)
            rr = rr_new
        return sg.dot(sg)
    generic(5)
    gts = []
    for _ in range(3):
        t0 = time.perf_counter()
        generic(iters)
        gts.append(time.perf_counter() - t0)
    N = n * p
    stored = int(rowptr[-1])
    words = 4 if os.environ.get("MI355OPT_NO_PACKED", "0") in ("", "0") else 12
    hess_bytes = words * stored + 8 * 7 * N   # product: matrix, V, X in, Z out; finish: X, Z, V in, out
    hess_us = sum(kus.values())
    out = dict(p=p, n=n, iters=int(np.median(its)), mode="prologue" if os.environ.get("MI355OPT_TALL_PROLOGUE") == "1" else "reduce",
               us_per_iteration=1e6 * float(np.median(ts)) / float(np.median(its)),
               us_spmm_gram=kus["stiefel_spmm_gram"], us_reduce=kus["stiefel_gram_reduce"], us_finish=kus["stiefel_finish_dots"],
               hess_bytes=hess_bytes, hess_fraction_of_peak=hess_bytes / (hess_us * 1e-6) / PEAK if hess_us else 0.0,
               generic_us_per_iteration=1e6 * float(np.median(gts)) / iters)
    print("RESULT " + json.dumps(out), flush=True)
    c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=100)
    ap.add_argument("--p", type=int, nargs="*", default=[9, 12, 16])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--child", type=int, default=0)
    ap.add_argument("--limit", type=int, default=150, help="seconds per child")
    a = ap.parse_args()
    if a.child:
        return child(a.nx, a.child, a.iters)
    rows = []
    for p in a.p:
        for mode in ("reduce", "prologue"):
            env = dict(os.environ, MI355OPT_TALL_PROLOGUE="1" if mode == "prologue" else "0")
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(p), "--nx", str(a.nx),
                                    "--iters", str(a.iters)], env=env, capture_output=True, text=True, timeout=a.limit)
            except subprocess.TimeoutExpired:
                print(f"p = {p} ({mode}): no result within {a.limit} s; stopping", file=sys.stderr)
                return 2
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                print(f"p = {p} ({mode}): child failed ({r.returncode}); stopping\n{r.stderr[-2000:]}", file=sys.stderr)
                return 2
            rows.append(json.loads(line[0][7:]))
            print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "tall_rows.jsonl"), "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    with open(os.path.join(ROOT, "profiles", "tall_rows.md"), "w") as f:
        f.write(f"# Tall rows: St({a.nx}^3, p), p = 9 ... 16 (tools/bench_tall_rows.py)\n\n"
                f"{a.iters}-iteration STPCG solves on the {a.nx}^3 Laplacian (value-indexed matrix), median of 5 after 3 warm-up "
                "solves, host clock around the whole solve divided by its iterations; kernel times from event pairs in "
                "separate solves.  Hessian bytes: the compulsory traffic of one application -- 4 bytes per matrix entry, V, X "
                "in and Z out in the product pass, X, Z, V in and the result out in the finish pass (7 fields of 8 n p bytes) -- "
                "and its rate over the product, reduce and finish kernels as a fraction of 8 TB/s.  The neighbouring "
                "reference point is p = 8's one-pass Hessian at 0.56 of peak.  Gram rows: `reduce` = one-workgroup reduce "
                "kernel between producer and consumer (the default), `prologue` = every consumer workgroup re-reduces the "
                "rows (MI355OPT_TALL_PROLOGUE=1).  Generic loop: the CG recurrence driven from the host, one kernel per "
                "vector statement, one synchronising inner product each, operator = mi_csr_spmm + mi_stiefel_project "
                "(cheaper than the full Hessian: a lower bound of what a client's own loop costs).\n\n")
        f.write("| p | Gram rows | us / inner iteration | product + Gram us | reduce us | finish us | Hessian bytes | of 8 TB/s | "
                "generic loop us / iteration | generic / fused |\n|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['p']} | {r['mode']} | {r['us_per_iteration']:.1f} | {r['us_spmm_gram']:.1f} | {r['us_reduce']:.1f} | "
                    f"{r['us_finish']:.1f} | {r['hess_bytes'] / 1e6:.0f} MB | {r['hess_fraction_of_peak']:.2f} | "
                    f"{r['generic_us_per_iteration']:.1f} | {r['generic_us_per_iteration'] / r['us_per_iteration']:.1f} |\n")
        f.write("\n")
        for p in a.p:
            rr = {r["mode"]: r for r in rows if r["p"] == p}
            if len(rr) == 2:
                best = min(rr, key=lambda m: rr[m]["us_per_iteration"])
                f.write(f"p = {p}: `{best}` is the faster form ({rr['reduce']['us_per_iteration']:.1f} us with the reduce kernel, "
                        f"{rr['prologue']['us_per_iteration']:.1f} us with the prologue re-reduction).\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
