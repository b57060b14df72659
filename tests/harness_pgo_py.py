"""ctypes loader of tests/cpp/libharness_pgo.so (harness_pgo.cpp): Riemannian::TNT on MI355::PoseGraph with the tagged
accessors (mode 0), with the objective and the retraction behind plain lambdas (1), PoseGraph::refine (2) and the pipeline
of examples/pose_graph_refinement.cpp (3), with the fusion counters around the run.  Test infrastructure."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "cpp", "libharness_pgo.so")
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
TAGGED, PLAIN, REFINE, PIPELINE = 0, 1, 2, 3


class PgoTntOut(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("f0", "f", "gradient_norm")] + \
               [(n, C.c_size_t) for n in ("outer", "inner_total", "syncs")] + \
               [(n, C.c_ulonglong) for n in ("fused_stpcg", "generic_stpcg", "fused_trials", "generic_trials",
                                             "generic_inner_products")] + \
               [("status", C.c_int)]


class PgoHarness:
    def __init__(self):
        if not os.path.exists(LIB):
            raise FileNotFoundError(LIB + " (run __graft_entry__.build())")
        L = self.L = C.CDLL(LIB)
        L.hg_last_error.restype = C.c_char_p
        L.hg_pgo_tnt.restype = C.c_int
        L.hg_pgo_tnt.argtypes = [C.c_int, C.c_size_t, C.c_size_t, _ip, _ip, _dp, _dp, _dp, _dp, _dp, C.c_size_t, C.c_size_t,
                                 C.POINTER(C.c_size_t), C.POINTER(C.c_int), _dp, C.POINTER(PgoTntOut)]

    def run(self, mode, N, ei, ej, Rt, tt, kappa, tau, x0, max_iterations=200):
        """dict of the PgoTntOut fields, rc / err, x (12N), and the per-iteration lists inner, accepted (modes 0 and 1)"""
        ei = np.ascontiguousarray(ei, dtype=np.int32)
        ej = np.ascontiguousarray(ej, dtype=np.int32)
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in (Rt, tt, kappa, tau, x0)]
        cap = max_iterations + 1
        inner, acc = (C.c_size_t * cap)(), (C.c_int * cap)()
        x, out = np.zeros(12 * N), PgoTntOut()
        rc = self.L.hg_pgo_tnt(mode, N, ei.size, ei.ctypes.data_as(_ip), ej.ctypes.data_as(_ip),
                               *[a.ctypes.data_as(_dp) for a in arrs], max_iterations, cap, inner, acc, x.ctypes.data_as(_dp),
                               C.byref(out))
        d = {name: getattr(out, name) for name, _ in PgoTntOut._fields_}
        n = d["outer"] if mode in (TAGGED, PLAIN) else 0
        d.update(rc=rc, err=self.L.hg_last_error().decode() if rc else "", x=x, inner=list(inner[:n]), accepted=list(acc[:n]))
        return d
