#!/usr/bin/env python3
"""The certificate panel product Z = S X at the cfg3 size (N = 5e5, the pose graph bench.py's cfg3 leg builds), through the
C ABI: k_so3_cert_panel (mi_so3n_cert_apply) against the SAME matrix S assembled as scalar CSR on the host and run through
mi_csr_spmm_colmajor -- the path that existed before -- at k = 8 and k = 24, alternating in one process after a warm-up,
each timed by an event pair around REPS back-to-back launches (the pair's own cost, measured around nothing, subtracted).

Algorithmic bytes of one block-kernel application, P = ceil(k / 8) passes over the matrix stream:
    P * (padded * 12 + nnzb * s + N * 52) + 48 k N      s = 32 (quaternion measurements) or 72
(per padded slot the weight (8) and the neighbour index (4); per incidence the measurement record; per node the six
diagonal-block entries (48) and its slot in perm (4); the panel read once and written once -- the 24 k nnzb bytes of
neighbour rows gathered from cache are not counted) and its share of 8 TB/s.  The CSR form: nnz * 12 + 48 k N.

Not measured here: LOBPCG iterations and time to a verdict at this size, and a block-Jacobi preconditioner (not built).

Usage: python tools/bench_certify.py [--n 500000] [--rounds 8] [--reps 20] [--out profiles/certify_so3n]
Writes <out>.jsonl (one line per round, form and width, and a summary line) and prints the summary."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np  # noqa: E402
from optimization_amd import capi, workloads as wl  # noqa: E402

PEAK_BYTES_PER_S = 8e12


def block_bytes(info, N, k):
    s = 32 if info["sinc_quat"] else 72
    return -(-k // 8) * (info["padded"] * 12 + info["nnzb"] * s + N * 52) + 48 * k * N


def csr_of_S(N, ei, ej, Rt, w, R):
    """S as scalar CSR (rowptr, col, val), from the float64 restatement of tests/so3n_certificate_reference.py"""
    import so3n_certificate_reference as cr
    ref = cr.CertRef(N, ei, ej, Rt, w, R)
    E = ref.degw()[:, None, None] * np.eye(3) - ref.C()
    M = np.asarray(Rt).reshape(-1, 3, 3)
    wv = np.asarray(w)[:, None, None]
    bi = np.concatenate([np.arange(N), ei, ej])
    bj = np.concatenate([np.arange(N), ej, ei])
    blk = np.concatenate([E, -wv * M, -wv * np.swapaxes(M, 1, 2)])
    rows = (3 * bi[:, None, None] + np.arange(3)[None, :, None] + 0 * np.arange(3)[None, None, :]).ravel()
    cols = (3 * bj[:, None, None] + 0 * np.arange(3)[None, :, None] + np.arange(3)[None, None, :]).ravel()
    vals = blk.ravel()
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    # duplicate edges: entries of the same (row, col) are added
    key = rows * (3 * N) + cols
    first = np.concatenate([[True], key[1:] != key[:-1]])
    start = np.flatnonzero(first)
    vals = np.add.reduceat(vals, start)
    rows, cols = rows[start], cols[start]
    rowptr = np.zeros(3 * N + 1, dtype=np.int64)
    np.add.at(rowptr, rows + 1, 1)
    return np.cumsum(rowptr).astype(np.int32), cols.astype(np.int32), vals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500_000)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="profiles/certify_so3n")
    a = ap.parse_args()
    if capi.device_count() == 0:
        sys.exit("bench_certify: no GPU (a measurement path does not fall back)")
    N = a.n
    ei, ej, Rt, w, _, R0 = wl.pose_graph(N)
    ctx = capi.Context(0)
    prob = ctx.so3n(N, ei, ej, Rt, w)
    info = prob.info()
    R = ctx.upload(R0.ravel())
    cert, cinfo = prob.certificate(R)
    rowptr, col, val = csr_of_S(N, ei, ej, Rt, w, R0)
    A = ctx.csr(3 * N, rowptr, col, val)
    m = 3 * N
    rng = np.random.Generator(np.random.PCG64(1))
    lines, summary = [], {"N": N, "E": int(len(ei)), "nnz": int(val.size), **info, "f": cinfo["f"]}
    for k in (8, 24):
        X = ctx.upload(rng.normal(size=m * k))
        Zb, Zc = ctx.vec(m * k), ctx.vec(m * k)
        forms = {"block": lambda: cert.apply(k, X, Zb), "csr": lambda: A.spmm_colmajor(k, X, Zc)}
        for fn in forms.values():                      # warm-up: code objects, pool
            for _ in range(3):
                fn()
        ctx.sync()
        diff = float(np.abs(Zb.numpy() - Zc.numpy()).max())
        ctx.timer_start()
        empty = ctx.timer_stop()
        per = {name: [] for name in forms}
        for r in range(a.rounds):
            for name, fn in (list(forms.items()) if r % 2 == 0 else list(forms.items())[::-1]):
                ctx.timer_start()
                for _ in range(a.reps):
                    fn()
                us = (ctx.timer_stop() - empty) * 1e3 / a.reps
                per[name].append(us)
                lines.append(dict(k=k, round=r, form=name, us_per_product=us))
        bb, cb = block_bytes(info, N, k), val.size * 12 + 48 * k * N
        for name, by in (("block", bb), ("csr", cb)):
            med = float(np.median(per[name]))
            summary[f"k{k}_{name}_us"] = med
            summary[f"k{k}_{name}_us_min_max"] = [float(min(per[name])), float(max(per[name]))]
            summary[f"k{k}_{name}_bytes"] = int(by)
            summary[f"k{k}_{name}_share_of_8TBs"] = by / (med * 1e-6) / PEAK_BYTES_PER_S
        summary[f"k{k}_max_abs_difference"] = diff
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out + ".jsonl", "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
        f.write(json.dumps(dict(summary=summary)) + "\n")
    print(json.dumps(summary, indent=1))
    ctx.close()


if __name__ == "__main__":
    main()
