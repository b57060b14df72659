#!/usr/bin/env python3
"""TNT on the cfg2-size Stiefel problem (Rayleigh quotient of the 3-D Laplacian, p = 3) with Args = {int, DeviceVector}
beside the empty-pack run of the same call (tests/cpp/harness_args.cpp): microseconds per inner iteration, the two
alternated `--reps` times, each the second run on its context.  The two launch the same kernels.

  python tools/bench_args_fusion.py [--grid 100 100 100] [--reps 5] [--out profiles/args_fusion_ab.md]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np  # noqa: E402

import args_py  # noqa: E402
import oracle_py  # noqa: E402
from optimization_amd import workloads as wl  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, nargs=3, default=[100, 100, 100])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--outer", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nx, ny, nz = a.grid
    n, p = nx * ny * nz, 3
    rowptr, col, val = wl.laplacian_3d(nx, ny, nz)
    X0 = wl.random_stiefel(n, p, seed=7)
    prm = oracle_py.Oracle().default_params(gradient_tolerance=0, relative_decrease_tolerance=0, stepsize_tolerance=0,
                                            preconditioned_gradient_tolerance=0, Delta_tolerance=0,
                                            max_iterations=a.outer, max_TPCG_iterations=50)
    H = args_py.ArgsHarness()
    us = {0: [], 1: []}
    last = {}
    for rep in range(a.reps):
        for pack in (0, 1):
            r = H.tnt_stiefel(n, p, rowptr, col, val, X0, prm, pack=pack, repeats=2)
            assert r["rc"] == 0, r.get("err")
            k = r["counters"]
            assert k["generic_stpcg_solves"] == 0 and k["fused_trial_steps"] == r["outer_iterations"], k
            us[pack].append(1e6 * k["seconds"] / int(np.sum(r["inner_iterations"])))
            last[pack] = r
    assert np.array_equal(last[0]["x"], last[1]["x"]) and last[0]["f"] == last[1]["f"]
    med = {k: statistics.median(v) for k, v in us.items()}
    out = dict(n=n, p=p, outer=int(last[0]["outer_iterations"]), inner=int(np.sum(last[0]["inner_iterations"])),
               us_per_inner_iteration={"empty_pack": med[0], "int_DeviceVector": med[1]},
               ranges={"empty_pack": [min(us[0]), max(us[0])], "int_DeviceVector": [min(us[1]), max(us[1])]})
    print(json.dumps(out))
    if a.out:
        lines = ["# TNT with an Args pack beside the empty-pack run", "",
                 "`tools/bench_args_fusion.py`: St(%d,%d), %d outer / %d inner iterations per run, the two calls alternated "
                 "%d times, wall time of the TNT call / inner iterations; bit-identical results." %
                 (n, p, out["outer"], out["inner"], a.reps), "",
                 "| call | us per inner iteration (median) | range |", "|---|---|---|",
                 "| `Args = {}` | %.1f | %.1f .. %.1f |" % (med[0], min(us[0]), max(us[0])),
                 "| `Args = {int, DeviceVector}` | %.1f | %.1f .. %.1f |" % (med[1], min(us[1]), max(us[1])), "",
                 "The two launch the same kernels; the difference of the medians is %.1f us (%.1f %%), %s the run-to-run "
                 "ranges above." % (med[1] - med[0], 100 * (med[1] / med[0] - 1),
                                    "inside" if min(us[1]) <= max(us[0]) and min(us[0]) <= max(us[1]) else "OUTSIDE"), ""]
        with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as f:
            f.write("\n".join(lines))


if __name__ == "__main__":
    main()
