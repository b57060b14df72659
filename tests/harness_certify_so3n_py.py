"""ctypes loader of tests/cpp/libharness_certify_so3n.so (harness_certify_so3n.cpp): MI355::RotationAveraging::certify at a
point of SO(3)^N or at what TNT reaches from it, with the tagged operator (0), the same operator behind a plain lambda (1),
or the tagged one plus a product through its PanelBlocks form (2).  Test infrastructure."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "cpp", "libharness_certify_so3n.so")
TAGGED, PLAIN_LAMBDA, TAGGED_BLOCKS = 0, 1, 2
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


class CertOut(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("lambda_min", "lambda_min_safe", "f", "lower_bound", "stationarity",
                                          "norm_estimate", "eta", "tnt_gradnorm", "blocks_residual")] + \
               [("iterations", C.c_size_t), ("tnt_iterations", C.c_size_t), ("converged", C.c_int), ("certified", C.c_int),
                ("tnt_status", C.c_int)]


class CertifySo3nHarness:
    def __init__(self):
        if not os.path.exists(LIB):
            raise FileNotFoundError(LIB + " (run __graft_entry__.build())")
        L = self.L = C.CDLL(LIB)
        L.hc_last_error.restype = C.c_char_p
        L.hc_certify_so3n.restype = C.c_int
        L.hc_certify_so3n.argtypes = [C.c_size_t, C.c_size_t, _ip, _ip, _dp, _dp, _dp, C.c_int, C.c_double, C.c_size_t,
                                      C.c_double, C.c_size_t, C.c_double, C.c_int, _dp, _dp, C.POINTER(CertOut)]

    def certify(self, N, ei, ej, Rt, w, R0, run_tnt=False, tnt_gradient_tolerance=1e-9, nx=6, tau=1e-8,
                max_iterations=1000, eta=-1.0, op_mode=TAGGED):
        """dict of the CertifyResult fields, the point certified (R, 9N), the eigenvector (3N) and the TNT run's figures"""
        ei = np.ascontiguousarray(ei, dtype=np.int32)
        ej = np.ascontiguousarray(ej, dtype=np.int32)
        Rt = np.ascontiguousarray(Rt, dtype=np.float64)
        w = np.ascontiguousarray(w, dtype=np.float64)
        R0 = np.ascontiguousarray(R0, dtype=np.float64).ravel()
        R, v = np.zeros(9 * N), np.zeros(3 * N)
        out = CertOut()
        rc = self.L.hc_certify_so3n(N, ei.size, ei.ctypes.data_as(_ip), ej.ctypes.data_as(_ip), Rt.ctypes.data_as(_dp),
                                    w.ctypes.data_as(_dp), R0.ctypes.data_as(_dp), int(run_tnt), tnt_gradient_tolerance,
                                    nx, tau, max_iterations, eta, int(op_mode), R.ctypes.data_as(_dp),
                                    v.ctypes.data_as(_dp), C.byref(out))
        d = {name: getattr(out, name) for name, _ in CertOut._fields_}
        d.update(rc=rc, err=self.L.hc_last_error().decode() if rc else "", R=R, eigenvector=v,
                 converged=bool(out.converged), certified=bool(out.certified))
        return d
