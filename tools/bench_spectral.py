#!/usr/bin/env python3
"""Spectral initialisation at the cfg3 size (N = 5e5, the pose graph bench.py's cfg3 leg builds), through the template
layer (tests/cpp/harness_spectral_so3n.cpp): wall-clock time of MI355::RotationAveraging::spectral_initialization and its
LOBPCG iterations, with and without the Jacobi preconditioner, alternating in one process after a warm-up run, beside the
TNT run that follows from the spectral point (its time per outer iteration: one model assembly and one inner STPCG solve).
No bar: it records what is measured.

Usage: python tools/bench_spectral.py [--n 500000] [--rounds 2] [--tau 1e-6] [--out profiles/spectral_init.md]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from optimization_amd import capi, workloads as wl  # noqa: E402
from harness_spectral_so3n_py import SpectralSo3nHarness  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=500_000)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--tau", type=float, default=1e-6)
    ap.add_argument("--max-iterations", type=int, default=1000)
    ap.add_argument("--out", default="profiles/spectral_init.md")
    a = ap.parse_args()
    if capi.device_count() == 0:
        sys.exit("bench_spectral: no GPU (a measurement path does not fall back)")
    N = a.n
    ei, ej, Rt, w, _, _ = wl.pose_graph(N)
    h = SpectralSo3nHarness()
    sei, sej, sRt, sw, _, _ = wl.pose_graph(2000)
    h.run(2000, sei, sej, sRt, sw, run_tnt=True, cert_max_iterations=0)     # warm-up: code objects, pools
    rows = []
    for r in range(a.rounds):
        for pre in ((True, False) if r % 2 == 0 else (False, True)):
            out = h.run(N, ei, ej, Rt, w, tau=a.tau, max_iterations=a.max_iterations, precondition=pre, run_tnt=True,
                        cert_max_iterations=0)
            if out["rc"]:
                sys.exit("bench_spectral: " + out["err"])
            row = dict(round=r, precondition=pre, seconds_spectral=out["seconds_spectral"], iterations=out["iterations"],
                       converged=out["converged"], flipped=out["flipped"], degenerate=out["degenerate"],
                       min_separation=out["min_separation"], f_R0=out["f"], lower_bound=out["lower_bound"],
                       seconds_tnt=out["seconds_tnt"], tnt_outer_iterations=out["tnt_iterations"], f_final=out["f_final"],
                       tnt_gradnorm=out["tnt_gradnorm"])
            print(json.dumps(row), flush=True)
            rows.append(row)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write("# Spectral initialisation of rotation averaging: what was measured\n\n")
        f.write("`tools/bench_spectral.py --n %d --rounds %d --tau %g`: the pose graph of bench.py's cfg3 leg, N = %d, E = %d, "
                "on %s.  Wall clock around `spectral_initialization()` (Laplacian diagonal, LOBPCG with nev = 3 and nx = 6, "
                "rounding, one objective) and around the TNT call from the spectral point (gradient tolerance 1e-9; its time "
                "per outer iteration is one model assembly plus one inner solve).  Both forms in the same process, "
                "alternating; no bar.\n\n" % (N, a.rounds, a.tau, N, len(ei), capi.Context(0).device_name()))
        f.write("| round | preconditioner | init s | LOBPCG iterations | converged | f(R0) | lower bound | TNT s | TNT outer "
                "iterations | TNT s / outer iteration | f final |\n|---|---|---|---|---|---|---|---|---|---|---|\n")
        for x in rows:
            per = x["seconds_tnt"] / max(1, x["tnt_outer_iterations"])
            f.write("| %d | %s | %.3f | %d | %s | %.6e | %.6e | %.3f | %d | %.4f | %.6e |\n" % (
                x["round"], "Jacobi" if x["precondition"] else "none", x["seconds_spectral"], x["iterations"], x["converged"],
                x["f_R0"], x["lower_bound"], x["seconds_tnt"], x["tnt_outer_iterations"], per, x["f_final"]))
        f.write("\nRounding: flipped %s, degenerate blocks %s, smallest separation %s.\n" % (
            sorted({x["flipped"] for x in rows}), sorted({x["degenerate"] for x in rows}),
            "%.3f" % min(x["min_separation"] for x in rows)))


if __name__ == "__main__":
    main()
