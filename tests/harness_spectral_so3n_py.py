"""ctypes loader of tests/cpp/libharness_spectral_so3n.so (harness_spectral_so3n.cpp): MI355::RotationAveraging::
spectral_initialization, and with run_tnt the TNT run from the spectral point and certify() at what it reaches.  Test
infrastructure."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "cpp", "libharness_spectral_so3n.so")
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


class SpectralOut(C.Structure):
    _fields_ = [("eigenvalues", C.c_double * 3)] + \
               [(n, C.c_double) for n in ("f", "lower_bound", "min_separation", "f_final", "tnt_gradnorm", "cert_lambda_min",
                                          "cert_lambda_min_safe", "cert_eta", "seconds_spectral", "seconds_tnt")] + \
               [(n, C.c_size_t) for n in ("iterations", "degenerate", "tnt_iterations", "cert_iterations")] + \
               [(n, C.c_int) for n in ("converged", "flipped", "has_eigenvectors", "tnt_status", "certified",
                                       "cert_converged")]


class SpectralSo3nHarness:
    def __init__(self):
        if not os.path.exists(LIB):
            raise FileNotFoundError(LIB + " (run __graft_entry__.build())")
        L = self.L = C.CDLL(LIB)
        L.hs_last_error.restype = C.c_char_p
        L.hs_spectral_so3n.restype = C.c_int
        L.hs_spectral_so3n.argtypes = [C.c_size_t, C.c_size_t, _ip, _ip, _dp, _dp, C.c_size_t, C.c_double, C.c_size_t,
                                       C.c_int, C.c_int, C.c_double, C.c_size_t, _dp, _dp, _dp, C.POINTER(SpectralOut)]

    def run(self, N, ei, ej, Rt, w, nx=6, tau=1e-6, max_iterations=1000, precondition=True, run_tnt=False,
            tnt_gradient_tolerance=1e-9, cert_max_iterations=4000):
        """dict of the SpectralResult fields, R0 (9N), the eigenvector panel V (3N x 3, None without a solve) and, with
        run_tnt, the TNT run's figures, the certificate's and the final point R"""
        ei = np.ascontiguousarray(ei, dtype=np.int32)
        ej = np.ascontiguousarray(ej, dtype=np.int32)
        Rt = np.ascontiguousarray(Rt, dtype=np.float64)
        w = np.ascontiguousarray(w, dtype=np.float64)
        R0, V, R = np.zeros(9 * N), np.zeros(9 * N), np.zeros(9 * N)
        out = SpectralOut()
        rc = self.L.hs_spectral_so3n(N, ei.size, ei.ctypes.data_as(_ip), ej.ctypes.data_as(_ip), Rt.ctypes.data_as(_dp),
                                     w.ctypes.data_as(_dp), nx, tau, max_iterations, int(precondition), int(run_tnt),
                                     tnt_gradient_tolerance, cert_max_iterations, R0.ctypes.data_as(_dp),
                                     V.ctypes.data_as(_dp), R.ctypes.data_as(_dp), C.byref(out))
        d = {name: getattr(out, name) for name, _ in SpectralOut._fields_ if name != "eigenvalues"}
        d.update(rc=rc, err=self.L.hs_last_error().decode() if rc else "", eigenvalues=np.array(out.eigenvalues[:]),
                 R0=R0, V=V.reshape(3, 3 * N).T.copy() if out.has_eigenvectors else None, R=R,
                 converged=bool(out.converged), flipped=bool(out.flipped), certified=bool(out.certified),
                 cert_converged=bool(out.cert_converged))
        return d
