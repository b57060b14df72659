"""ctypes loader of tests/cpp/libharness_tnls_so3n.so (harness_tnls_so3n.cpp): Riemannian::TNLS on chordal rotation
averaging as a nonlinear least-squares problem, in three modes (0 host restatement on a host vector, 1 the tagged accessors
of MI355::RotationAveraging on DeviceVector, 2 the same device operators behind plain lambdas).  Test infrastructure."""
import ctypes as C
import os

import numpy as np

from optimization_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "cpp", "libharness_tnls_so3n.so")
HOST, DEVICE, GENERIC = 0, 1, 2
STATUS = ("Root", "Gradient", "RelativeDecrease", "Stepsize", "TrustRegion", "IterationLimit", "ElapsedTime", "UserFunction")
ETA1 = .05          # TNLSParams::eta1: a step is accepted when rho > eta1
_dp = C.POINTER(C.c_double)
_sp = C.POINTER(C.c_size_t)
_ip = C.POINTER(C.c_int32)


class TnlsOut(C.Structure):
    _fields_ = [("fusion", capi.FusionCounters), ("status", C.c_int), ("outer", C.c_size_t), ("f", C.c_double),
                ("gradnorm", C.c_double)]


class TnlsSo3nHarness:
    def __init__(self):
        if not os.path.exists(LIB):
            raise FileNotFoundError(LIB + " (run __graft_entry__.build())")
        L = self.L = C.CDLL(LIB)
        L.ht_last_error.restype = C.c_char_p
        L.ht_tnls_so3n.restype = C.c_int
        L.ht_tnls_so3n.argtypes = [C.c_size_t, C.c_size_t, _ip, _ip, _dp, _dp, _dp, C.c_int, C.c_int, C.c_double,
                                   C.c_double, C.c_double, C.c_size_t, C.c_size_t, C.c_size_t, _dp, _sp, _dp, _dp, _dp,
                                   C.POINTER(TnlsOut)]

    def tnls(self, N, ei, ej, Rt, w, R0, prm, mode, with_precon, cap=1024):
        """prm: the `params` of a case of tests/golden/tnls_so3n.json (Delta0, kappa_fgr, gradient_tolerance,
        max_iterations, max_LSQR_iterations)"""
        ei = np.ascontiguousarray(ei, dtype=np.int32)
        ej = np.ascontiguousarray(ej, dtype=np.int32)
        Rt = np.ascontiguousarray(Rt, dtype=np.float64)
        w = np.ascontiguousarray(w, dtype=np.float64)
        R0 = np.ascontiguousarray(R0, dtype=np.float64).ravel()
        x = np.zeros(9 * N)
        inner = np.zeros(cap, dtype=np.uint64)
        rho, radius, fn = np.zeros(cap), np.zeros(cap), np.zeros(cap)
        out = TnlsOut()
        rc = self.L.ht_tnls_so3n(N, ei.size, ei.ctypes.data_as(_ip), ej.ctypes.data_as(_ip), Rt.ctypes.data_as(_dp),
                                 w.ctypes.data_as(_dp), R0.ctypes.data_as(_dp), int(mode), int(bool(with_precon)),
                                 prm["Delta0"], prm["kappa_fgr"], prm["gradient_tolerance"], prm["max_iterations"],
                                 prm["max_LSQR_iterations"], cap, x.ctypes.data_as(_dp), inner.ctypes.data_as(_sp),
                                 rho.ctypes.data_as(_dp), radius.ctypes.data_as(_dp), fn.ctypes.data_as(_dp), C.byref(out))
        k = min(out.outer, cap)
        counters = {name: int(getattr(out.fusion, name)) for name, _ in capi.FusionCounters._fields_}
        return dict(rc=rc, err=self.L.ht_last_error().decode() if rc else "", x=x, f=out.f, gradfx_norm=out.gradnorm,
                    status=int(out.status), outer=int(out.outer), inner_iterations=[int(v) for v in inner[:k]],
                    rho=rho[:k].copy(), trust_region_radius=radius[:k].copy(), F_norms=fn[:k].copy(),
                    accepted=[bool(r > ETA1) for r in rho[:k]], counters=counters)
