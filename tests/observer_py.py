"""ctypes loader of tests/cpp/libharness_observer.so (harness_observer.cpp): STPCG with a recording user function through
one templated driver, on the host vector (device=0, the reference's arithmetic) and on MI355::DeviceVector (device=1, the
fused observed solve).  Test infrastructure."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "cpp", "libharness_observer.so")
NEVER = C.c_size_t(-1).value
REC_COLS = ("k", "alpha", "ss", "rr", "rv", "pp", "sp")
_dp = C.POINTER(C.c_double)
# kappa_fgr of the host-against-device records (tests/test_gpu_stpcg_observer.py; the depth at which the host loop's own
# record is stable to 1e-11 under one ulp of its input: tests/test_cpu_observer_resources.py)
KAPPA_PLAIN, KAPPA_PRECON = 1e-3, 0.5


class ObsOut(C.Structure):
    _fields_ = [("nrec", C.c_size_t), ("iterations", C.c_size_t), ("M_norm", C.c_double), ("P_engaged", C.c_int),
                ("At_engaged", C.c_int), ("v_is_r", C.c_int), ("fused_stpcg_solves", C.c_ulonglong),
                ("generic_stpcg_solves", C.c_ulonglong), ("generic_inner_products", C.c_ulonglong), ("syncs", C.c_size_t)]


def _p(a):
    return a.ctypes.data_as(_dp)


class ObserverHarness:
    def __init__(self):
        if not os.path.exists(LIB):
            from optimization_amd import build
            build.build()
            build.build_harness()
        self.L = C.CDLL(LIB)
        self.L.hob_last_error.restype = C.c_char_p
        self.L.hob_observed_diag.restype = C.c_int
        self.L.hob_observed_diag.argtypes = [C.c_int, C.c_size_t, _dp, _dp, _dp, C.c_double, C.c_size_t, C.c_double,
                                             C.c_double, C.c_size_t, C.c_size_t, C.c_int, C.c_int, _dp, C.c_size_t, _dp,
                                             C.POINTER(ObsOut)]
        self.L.hob_observed_projected.restype = C.c_int
        self.L.hob_observed_projected.argtypes = [C.c_int, C.c_size_t, C.c_size_t, _dp, _dp, _dp, _dp, C.c_double,
                                                  C.c_size_t, C.c_double, C.c_double, C.c_int, _dp, C.c_size_t, _dp,
                                                  C.POINTER(ObsOut)]

        self.L.hob_observed_on.restype = C.c_int
        self.L.hob_observed_on.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_size_t, C.c_double,
                                           C.c_double, C.c_int, _dp, _dp, C.POINTER(ObsOut)]

    def on(self, ctx, g, H, Delta, max_iterations, kappa, theta, reps=1, want_s=True):
        """the template call with a counting user function on capi objects (Context, Vec, Op); per-call seconds"""
        sec, s, out = np.zeros(reps), np.zeros(g.n if want_s else 1), ObsOut()
        rc = self.L.hob_observed_on(ctx.h, g.h, H.h, Delta, max_iterations, kappa, theta, reps, _p(sec),
                                    _p(s) if want_s else None, C.byref(out))
        r = {k: getattr(out, k) for k, _ in ObsOut._fields_}
        r.update(rc=rc, s=s, calls=out.nrec, seconds=sec)
        return r

    def err(self):
        return self.L.hob_last_error().decode()

    @staticmethod
    def _result(rc, out, rec, s):
        r = {k: getattr(out, k) for k, _ in ObsOut._fields_}
        r.update(rc=rc, s=s, calls=out.nrec, rec=rec[:min(out.nrec, rec.shape[0])].copy())
        return r

    def diag(self, device, g, D, Minv, Delta, max_iterations, kappa, theta, stop_at=NEVER, throw_at=NEVER,
             record_dots=True, no_fused_observer=False, rec_cap=1024):
        g, D = np.ascontiguousarray(g, dtype=np.float64), np.ascontiguousarray(D, dtype=np.float64)
        Mi = np.ascontiguousarray(Minv, dtype=np.float64) if Minv is not None else None
        rec, s, out = np.zeros((rec_cap, len(REC_COLS))), np.zeros(g.size), ObsOut()
        rc = self.L.hob_observed_diag(int(device), g.size, _p(g), _p(D), _p(Mi) if Mi is not None else None, Delta,
                                      max_iterations, kappa, theta, stop_at, throw_at, int(record_dots),
                                      int(no_fused_observer), _p(rec), rec_cap, _p(s), C.byref(out))
        return self._result(rc, out, rec, s)

    def projected(self, device, pr, record_dots=True, rec_cap=8192):
        g, P, M, A = (np.ascontiguousarray(pr[k], dtype=np.float64) for k in ("g", "P", "M", "A"))
        rec, s, out = np.zeros((rec_cap, len(REC_COLS))), np.zeros(g.size), ObsOut()
        rc = self.L.hob_observed_projected(int(device), pr["n"], pr["m"], _p(g), _p(P), _p(M), _p(A), pr["Delta"],
                                           pr["max_iterations"], pr["kappa"], pr["theta"], int(record_dots), _p(rec),
                                           rec_cap, _p(s), C.byref(out))
        return self._result(rc, out, rec, s)
