"""ctypes loader of tests/cpp/libharness_pgo_trans.so (harness_pgo_trans.cpp): MI355::TranslationRecovery::solve, the
client's own STPCG call with laplacian() / jacobi(), and the fusion counters around each.  Test infrastructure."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "cpp", "libharness_pgo_trans.so")
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


class PgoOut(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("objective", "relative_residual", "max_residual", "residuals_objective",
                                          "residuals_max", "client_M_norm")] + \
               [(n, C.c_size_t) for n in ("iterations", "client_iterations")] + \
               [(n, C.c_ulonglong) for n in ("solve_fused", "solve_generic", "solve_inner_products", "client_fused",
                                             "client_generic", "client_inner_products")] + \
               [("exit_reason", C.c_int)]


class PgoTransHarness:
    def __init__(self):
        if not os.path.exists(LIB):
            raise FileNotFoundError(LIB + " (run __graft_entry__.build())")
        L = self.L = C.CDLL(LIB)
        L.hp_last_error.restype = C.c_char_p
        L.hp_pgo_trans.restype = C.c_int
        L.hp_pgo_trans.argtypes = [C.c_size_t, C.c_size_t, _ip, _ip, _dp, _dp, C.c_longlong, _dp, C.c_double, C.c_size_t,
                                   _dp, _dp, _dp, _dp, C.POINTER(PgoOut)]

    def run(self, N, ei, ej, tt, tau, anchor, R, tol=1e-10, max_iterations=1000):
        """dict of the PgoOut fields, rc / err, and the arrays t_solve, t_client (3N), b (3N), r (3E)"""
        ei = np.ascontiguousarray(ei, dtype=np.int32)
        ej = np.ascontiguousarray(ej, dtype=np.int32)
        tt = np.ascontiguousarray(tt, dtype=np.float64)
        tau = np.ascontiguousarray(tau, dtype=np.float64)
        R = np.ascontiguousarray(R, dtype=np.float64)
        ts, tc, b, r = np.zeros(3 * N), np.zeros(3 * N), np.zeros(3 * N), np.zeros(max(1, 3 * ei.size))
        out = PgoOut()
        rc = self.L.hp_pgo_trans(N, ei.size, ei.ctypes.data_as(_ip), ej.ctypes.data_as(_ip), tt.ctypes.data_as(_dp),
                                 tau.ctypes.data_as(_dp), anchor, R.ctypes.data_as(_dp), tol, max_iterations,
                                 ts.ctypes.data_as(_dp), tc.ctypes.data_as(_dp), b.ctypes.data_as(_dp), r.ctypes.data_as(_dp),
                                 C.byref(out))
        d = {name: getattr(out, name) for name, _ in PgoOut._fields_}
        d.update(rc=rc, err=self.L.hp_last_error().decode() if rc else "", t_solve=ts, t_client=tc, b=b, r=r[:3 * ei.size])
        return d
