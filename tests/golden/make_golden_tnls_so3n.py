"""Generate tests/golden/tnls_so3n.json: Riemannian::TNLS of this repository's template layer on a plain host vector
(TNLS.h there is pinned bit for bit to the real reference on the sin-fit and affine problems) on chordal rotation averaging
as a nonlinear least-squares problem, F_e = sqrt(w_e) (R_j - R_i Rt_e), with the plain-C++ restatement of F, dF, dF* and
the retraction of tests/cpp/harness_tnls_so3n.cpp (mode 0).  Data only: parameters, seeds, status, outer count, every LSQR
count, the gain-ratio and radius traces, |F|, |grad L| and the final x.

Run where tests/cpp/libharness_tnls_so3n.so has been built:  python tests/golden/make_golden_tnls_so3n.py

Cases: the pose graphs of optimization_amd.workloads.pose_graph at N = 40 and N = 150 (seed 7) from that generator's Rinit,
each without and with the Gauss-Newton right preconditioner diag(1 / sqrt(2 degw)); Delta0 = 10 (at the default 1 the first
solves end on the trust region after 0 passes).  From Rinit every Gauss-Newton step of these graphs is accepted whatever
the radius, so the REJECTED-STEP case starts the N = 40 graph far from the solution, at seeded random rotations
(PCG64(11), exp of 2 * normal): with Delta0 = 2 its first step is rejected (rho = -23) and the next LSQR solve runs at the
same point with the old linearisation.  The conditions a fixture must meet are asserted below; the device test compares
every count exactly, so every run is repeated with LSQR's btol scaled by 1 +- 1e-9: a stop that is a near tie would change
a count, and the seed would have to be replaced here."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from harness_tnls_so3n_py import HOST, STATUS, TnlsSo3nHarness  # noqa: E402
from optimization_amd import workloads as wl  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
KAPPA, THETA = .1, .5                       # TNLSParams: btol = min(|F|^theta, kappa_fgr)
# key, N, graph seed, with_precon, Delta0, start (None: Rinit; else the seed of random rotations)
CASES = (("N40", 40, 7, 0, 10.0, None), ("N40_precon", 40, 7, 1, 10.0, None),
         ("N150", 150, 7, 0, 10.0, None), ("N150_precon", 150, 7, 1, 10.0, None),
         ("N40_rejected", 40, 7, 0, 2.0, 11))
REJECTED_CASE = "N40_rejected"
MAX_ITERATIONS = 200


def start_point(N, graph_seed, start):
    if start is None:
        return wl.pose_graph(N, seed=graph_seed)[5]
    rng = np.random.Generator(np.random.PCG64(start))
    return np.ascontiguousarray(wl.so3_exp(rng.normal(size=(N, 3)) * 2.0).reshape(N, 9))


def lst(a):
    return [float(x) for x in np.asarray(a).ravel()]


def check_conditions(key, rec):
    """what tests/test_cpu_so3n_nls.py asserts again on the committed file"""
    inner, acc = rec["inner_iterations"], rec["accepted"]
    assert STATUS[rec["status"]] in ("Gradient", "Root"), STATUS[rec["status"]]
    assert rec["outer"] == len(inner) == len(acc) < rec["params"]["max_iterations"]
    assert len(set(inner)) > 1, inner                                   # LSQR counts are not all equal
    assert max(inner) < rec["params"]["max_LSQR_iterations"]
    assert all(f ** THETA > rec["params"]["kappa_fgr"] for f in rec["F_norms"])   # btol is kappa_fgr in every solve
    if key == REJECTED_CASE:
        k = acc.index(False)
        assert k + 1 < rec["outer"], "the rejected step must be followed by a further solve at the same point"
    else:
        assert all(acc)


def main():
    H = TnlsSo3nHarness()
    out = {}
    for key, N, gseed, pre, Delta0, start in CASES:
        ei, ej, Rt, w = wl.pose_graph(N, seed=gseed)[:4]
        R0 = start_point(N, gseed, start)
        prm = dict(Delta0=Delta0, kappa_fgr=KAPPA, gradient_tolerance=1e-6, max_iterations=MAX_ITERATIONS,
                   max_LSQR_iterations=1000)
        r = H.tnls(N, ei, ej, Rt, w, R0, prm, HOST, pre)
        assert r["rc"] == 0, r["err"]
        for s in (1 - 1e-9, 1 + 1e-9):          # no LSQR stop is a near tie
            t = H.tnls(N, ei, ej, Rt, w, R0, dict(prm, kappa_fgr=KAPPA * s), HOST, pre)
            assert t["rc"] == 0 and (t["status"], t["inner_iterations"], t["accepted"]) == \
                (r["status"], r["inner_iterations"], r["accepted"]), (key, s)
        rec = dict(N=N, graph_seed=gseed, with_precon=pre, start_seed=start, params=prm, status=r["status"],
                   outer=r["outer"], inner_iterations=r["inner_iterations"], accepted=r["accepted"], rho=lst(r["rho"]),
                   trust_region_radius=lst(r["trust_region_radius"]), F_norms=lst(r["F_norms"]), f=float(r["f"]),
                   gradfx_norm=float(r["gradfx_norm"]), x=lst(r["x"]))
        check_conditions(key, rec)
        print(key, STATUS[rec["status"]], "outer", rec["outer"], "LSQR", rec["inner_iterations"], "accepted",
              "".join(str(int(a)) for a in rec["accepted"]), "|F|", rec["f"], "|grad L|", rec["gradfx_norm"])
        out[key] = rec
    json.dump(out, open(os.path.join(OUT, "tnls_so3n.json"), "w"), indent=1)
    print("written", os.path.join(OUT, "tnls_so3n.json"))


if __name__ == "__main__":
    main()
