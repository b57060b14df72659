#!/usr/bin/env python3
"""Cost of a user function in LSQR: microseconds per pass at n = 3e6 (tridiagonal operator of tools/bench_lsqr.py, built-in
CSR operators) of LinearAlgebra::LSQR<DeviceVector> through tests/cpp/harness_lsqr_observer.cpp for

  (a) the call without a user function            the un-observed fused solve, mi_lsqr
  (b) the call with a counting user function      the observed fused solve, mi_lsqr_observed
  (c) the same call with NO_FUSED_LSQR_OBSERVER=1   the generic template loop (what such a call ran before)

The three are alternated `--reps` times in one process; each measurement is the wall time of the LSQR call (device
drained, second run on a context) at `--passes` + 1 passes minus that at 1 pass, per pass.  The figure of a leg is the
median over the repetitions, with the range.

  python tools/bench_lsqr_observer.py [--n 3000000] [--passes 200] [--reps 5] [--out profiles/lsqr_observer_ab.md]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import lsqr_observer_py as lo  # noqa: E402

LEGS = (("a", "un-observed fused pass (mi_lsqr)", dict(user_function=False)),
        ("b", "observed fused pass (mi_lsqr_observed)", dict()),
        ("c", "generic template loop, same user function", dict(no_fused=True)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3_000_000)
    ap.add_argument("--passes", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.n
    lo_, di, up = np.full(n, -1.0), np.full(n, 2.02), np.full(n, -0.99)    # slow to converge (tools/bench_lsqr.py)
    b = di * np.sin(np.arange(n) * 1e-3)
    H = lo.LsqrObserverHarness()
    us = {leg: [] for leg, _, _ in LEGS}
    for rep in range(a.reps):
        for leg, _, kw in LEGS:
            t = {}
            for passes in (1, a.passes + 1):
                r = H.tridiag(1, 0, lo_, di, up, b, max_iterations=passes, btol=0.0, Atol=0.0, rec_cap=0, repeats=2,
                              **kw)
                assert r["rc"] == 0 and r["iterations"] == passes, (r["rc"], r["err"], r["iterations"])
                assert (r["fused_lsqr_solves"], r["generic_lsqr_solves"]) == ((0, 1) if leg == "c" else (1, 0)), r
                assert r["calls"] == (0 if leg == "a" else passes)
                t[passes] = r["seconds"]
            us[leg].append(1e6 * (t[a.passes + 1] - t[1]) / a.passes)
    med = {leg: statistics.median(v) for leg, v in us.items()}
    out = dict(n=n, passes=a.passes, reps=a.reps,
               legs={leg: dict(us_per_pass=med[leg], min=min(us[leg]), max=max(us[leg])) for leg in us},
               observed_over_unobserved=med["b"] / med["a"], observed_over_generic=med["b"] / med["c"])
    print(json.dumps(out))
    if a.out:
        lines = ["# LSQR with a user function: observed fused pass, un-observed fused pass, generic loop", "",
                 "`tools/bench_lsqr_observer.py`: n = %d, tridiagonal operator (built-in CSR), a user function that only "
                 "counts; the three legs alternated %d times in one process, each figure the median (range) of "
                 "(time at %d passes - time at 1 pass) / %d." % (n, a.reps, a.passes + 1, a.passes), "",
                 "| leg | us per pass | range |", "|---|---|---|"]
        for leg, name, _ in LEGS:
            lines.append("| %s | %.1f | %.1f .. %.1f |" % (name, med[leg], min(us[leg]), max(us[leg])))
        lines += ["", "Observed / un-observed: x%.2f (one kernel boundary and one polled host wait per pass, no run-ahead)."
                  % out["observed_over_unobserved"],
                  "Observed / generic loop: x%.2f -- the observed fused pass is %s than the generic loop, which is what a call "
                  "with a user function ran before." % (out["observed_over_generic"],
                                                        "FASTER" if med["b"] < med["c"] else "NOT faster"), ""]
        with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as f:
            f.write("\n".join(lines))


if __name__ == "__main__":
    main()
