"""Generate tests/golden/gd_so3n.json: the REAL reference's GradientDescent (oracle/_ref/libref.so, oracle_py.Reference.gd)
on chordal rotation averaging over SO(3)^N -- the problem of oracle/problems.c ("SO(3)^N") on the pose graphs of
optimization_amd.workloads.pose_graph, started at that generator's Rinit.  Data only: parameters, seed, N, status,
iteration count, every line-search count, the objective trace, f, the gradient norm and the final x.

Run where oracle/_ref/libref.so has been built:  python tests/golden/make_golden_gd_so3n.py

Cases: N = 40, seed 7 (the graph of tnt_so3n_40.json) and N = 150, seed 7.  The first step length is
alpha = k / (largest weighted degree): 1 / (4 max degree) is the safe step of a chordal cost (every Armijo test passes at
once: all line-search counts 1), so k is raised until the line search has to backtrack at some iterations and not at
others -- k = 1 at N = 40 (counts 1 and 2), k = 2 at N = 150 (counts 1 ... 4).  beta = sigma = 1/2, gradient tolerance 1e-6.
The conditions a fixture must meet are asserted below; the device test compares every count exactly, so a seed on which
a sufficient-decrease test is a near tie (device counts that differ while the iterates agree to 1e-12) would have to be
replaced here -- none of the two is."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import oracle_py  # noqa: E402
from optimization_amd import workloads as wl  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
CASES = (("N40", 40, 7, 1.0), ("N150", 150, 7, 2.0))      # key, N, seed, k of alpha = k / max weighted degree
MAX_ITERATIONS = 400


def lst(a):
    return [float(x) for x in np.asarray(a).ravel()]


def check_conditions(rec):
    """what tests/test_cpu_gd_so3n.py asserts again on the committed file"""
    ls = rec["linesearch_iterations"]
    assert rec["status"] == 0, rec["status"]                       # GradientDescentStatus::Gradient
    assert rec["iterations"] == len(ls) <= MAX_ITERATIONS
    assert rec["iterations"] < rec["params"]["max_iterations"]     # ... not the iteration limit
    assert rec["gradfx_norm"] < rec["params"]["gradient_tolerance"]
    assert any(v > 1 for v in ls) and any(v == 1 for v in ls), sorted(set(ls))
    assert len(rec["objective_values"]) == rec["iterations"]
    assert all(a > b for a, b in zip(rec["objective_values"], rec["objective_values"][1:] + [rec["f"]]))


def main():
    O = oracle_py.Oracle()
    R = oracle_py.Reference()
    T = oracle_py.TemplateHarness()      # this repository's template layer on a host vector: the oracle's restatement
    out = {}
    for key, N, seed, k in CASES:
        ei, ej, Rt, w, _, Rinit = wl.pose_graph(N, seed=seed)
        deg = np.zeros(N)
        np.add.at(deg, ei, w)
        np.add.at(deg, ej, w)
        kw = dict(max_iterations=MAX_ITERATIONS, gradient_tolerance=1e-6, relative_decrease_tolerance=0.0,
                  stepsize_tolerance=0.0, alpha=float(k / deg.max()), beta=.5, sigma=.5, max_ls_iterations=100)
        pr = O.so3n(N, ei, ej, Rt, w)
        r = R.gd(pr, Rinit.ravel(), **kw)
        t = T.gd(pr, Rinit.ravel(), **kw)
        O.free(pr)
        assert r["rc"] == 0 and t["rc"] == 0
        # the standard of the existing fixtures: restatement and reference agree on every count and on x bit for bit
        assert (r["status"], r["iterations"]) == (t["status"], t["iterations"])
        assert list(r["linesearch_iterations"]) == list(t["linesearch_iterations"])
        assert np.array_equal(r["x"], t["x"]) and np.array_equal(r["objective_values"], t["objective_values"])
        assert r["f"] == t["f"] and r["gradfx_norm"] == t["gradfx_norm"]
        rec = dict(N=N, seed=seed, alpha_times_max_weighted_degree=k, max_weighted_degree=float(deg.max()), params=kw,
                   status=int(r["status"]), iterations=int(r["iterations"]),
                   linesearch_iterations=[int(v) for v in r["linesearch_iterations"]],
                   objective_values=lst(r["objective_values"]), f=float(r["f"]), gradfx_norm=float(r["gradfx_norm"]),
                   x=lst(r["x"]))
        check_conditions(rec)
        print(key, "iterations", rec["iterations"], "line-search counts", np.bincount(rec["linesearch_iterations"])[1:],
              "f", rec["f"], "|grad|", rec["gradfx_norm"])
        out[key] = rec
    json.dump(out, open(os.path.join(OUT, "gd_so3n.json"), "w"), indent=1)
    print("written", os.path.join(OUT, "gd_so3n.json"))


if __name__ == "__main__":
    main()
