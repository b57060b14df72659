"""ctypes loader of tests/cpp/libharness_gd_so3n.so (harness_gd_so3n.cpp): Riemannian::GradientDescent on
MI355::RotationAveraging through the problem object's accessors, in four modes (0 fused Armijo trial, 1 plain_retraction(),
2 Args = {DeviceVector}, 3 objective wrapped in a lambda).  Test infrastructure."""
import ctypes as C
import os

import numpy as np

from optimization_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "cpp", "libharness_gd_so3n.so")
FUSED, PLAIN_RETRACTION, PACK, WRAPPED_OBJECTIVE = 0, 1, 2, 3
_dp = C.POINTER(C.c_double)
_sp = C.POINTER(C.c_size_t)
_ip = C.POINTER(C.c_int32)


class GdOut(C.Structure):
    _fields_ = [("fusion", capi.FusionCounters), ("syncs", C.c_size_t), ("seconds", C.c_double)]


class GdSo3nHarness:
    def __init__(self):
        if not os.path.exists(LIB):
            raise FileNotFoundError(LIB + " (run __graft_entry__.build())")
        L = self.L = C.CDLL(LIB)
        L.hg_last_error.restype = C.c_char_p
        L.hg_gd_so3n.restype = C.c_int
        L.hg_gd_so3n.argtypes = [C.c_size_t, C.c_size_t, _ip, _ip, _dp, _dp, _dp, C.c_size_t, C.c_double, C.c_double,
                                 C.c_double, C.c_double, C.c_size_t, C.c_int, _dp, _dp, _dp, C.POINTER(C.c_int), _sp,
                                 C.c_size_t, _dp, _sp, C.POINTER(GdOut)]

    def gd(self, N, ei, ej, Rt, w, R0, prm, mode, cap=4096):
        """prm: the `params` of a case of tests/golden/gd_so3n.json.  objective_values: one per iteration started (the
        last one is f at the final point when the run stops on the gradient tolerance)."""
        ei = np.ascontiguousarray(ei, dtype=np.int32)
        ej = np.ascontiguousarray(ej, dtype=np.int32)
        Rt = np.ascontiguousarray(Rt, dtype=np.float64)
        w = np.ascontiguousarray(w, dtype=np.float64)
        R0 = np.ascontiguousarray(R0, dtype=np.float64).ravel()
        x = np.zeros(9 * N)
        f, gn = C.c_double(0), C.c_double(0)
        st, it = C.c_int(-1), C.c_size_t(0)
        fv = np.zeros(cap)
        ls = np.zeros(cap, dtype=np.uint64)
        out = GdOut()
        rc = self.L.hg_gd_so3n(N, ei.size, ei.ctypes.data_as(_ip), ej.ctypes.data_as(_ip), Rt.ctypes.data_as(_dp),
                               w.ctypes.data_as(_dp), R0.ctypes.data_as(_dp), prm["max_iterations"],
                               prm["gradient_tolerance"], prm["alpha"], prm["beta"], prm["sigma"],
                               prm["max_ls_iterations"], int(mode), x.ctypes.data_as(_dp), C.byref(f), C.byref(gn),
                               C.byref(st), C.byref(it), cap, fv.ctypes.data_as(_dp), ls.ctypes.data_as(_sp),
                               C.byref(out))
        k = min(it.value, cap)
        counters = {name: int(getattr(out.fusion, name)) for name, _ in capi.FusionCounters._fields_}
        counters.update(syncs=int(out.syncs), seconds=out.seconds)
        return dict(rc=rc, err=self.L.hg_last_error().decode() if rc else "", x=x, f=f.value, gradfx_norm=gn.value,
                    status=st.value, iterations=it.value, objective_values=fv[:k + 1].copy(),
                    linesearch_iterations=ls[:k].astype(np.int64), counters=counters)
