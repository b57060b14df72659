"""ctypes loader of tests/cpp/libharness_args.so (harness_args.cpp): the optimizers of the template layer called with an
extra-argument pack (Args...), empty (pack=0) and not (pack=1), through one templated driver each.  Test infrastructure."""
import ctypes as C
import os

import numpy as np

import oracle_py as op
from harness_py import DeviceHarness
from optimization_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "cpp", "libharness_args.so")
NEVER = C.c_size_t(-1).value
_dp = C.POINTER(C.c_double)
_sp = C.POINTER(C.c_size_t)
_ip = C.POINTER(C.c_int32)


class ArgsOut(C.Structure):
    _fields_ = [("fusion", capi.FusionCounters), ("syncs", C.c_size_t), ("accepted", C.c_size_t),
                ("user_calls", C.c_size_t), ("seconds", C.c_double)]


class CountOut(C.Structure):
    _fields_ = [("counter", C.c_size_t), ("iterations", C.c_size_t), ("M_norm", C.c_double), ("dev", ArgsOut)]


def _p(a):
    return a.ctypes.data_as(_dp)


def _i(a):
    return a.ctypes.data_as(_ip)


def _out(o):
    d = {k: int(getattr(o.fusion, k)) for k, _ in capi.FusionCounters._fields_}
    d.update(syncs=o.syncs, user_calls=o.user_calls, seconds=o.seconds)
    return d


class ArgsHarness:
    def __init__(self):
        if not os.path.exists(LIB):
            raise FileNotFoundError(LIB + " (run __graft_entry__.build())")
        L = self.L = C.CDLL(LIB)
        L.ha_last_error.restype = C.c_char_p
        L.ha_tnt_stiefel.restype = C.c_int
        L.ha_tnt_stiefel.argtypes = [C.c_size_t, C.c_int, _ip, _ip, _dp, _dp, C.POINTER(op.TntParams), C.c_int, C.c_int,
                                     C.c_int, C.POINTER(op.TntResult), C.POINTER(ArgsOut)]
        L.ha_tnt_so3n.restype = C.c_int
        L.ha_tnt_so3n.argtypes = [C.c_size_t, C.c_size_t, _ip, _ip, _dp, _dp, _dp, C.POINTER(op.TntParams), C.c_int,
                                  C.POINTER(op.TntResult), C.POINTER(ArgsOut)]
        L.ha_gd_stiefel.restype = C.c_int
        L.ha_gd_stiefel.argtypes = [C.c_size_t, C.c_int, _ip, _ip, _dp, _dp, C.c_size_t, C.c_double, C.c_double,
                                    C.c_double, C.c_double, C.c_size_t, C.c_int, _dp, _dp, _dp, C.POINTER(C.c_int), _sp,
                                    C.c_size_t, _dp, _sp, C.POINTER(ArgsOut)]
        L.ha_lsqr_csr.restype = C.c_int
        L.ha_lsqr_csr.argtypes = [C.c_size_t, _ip, _ip, _dp, _ip, _ip, _dp, _dp, C.c_size_t, C.c_double, C.c_double,
                                  C.c_double, C.c_double, C.c_double, C.c_int, _dp, _dp, _sp, C.POINTER(ArgsOut)]
        L.ha_counting.restype = C.c_int
        L.ha_counting.argtypes = [C.c_int, C.c_int, C.c_int, C.c_size_t, _dp, _dp, _dp, C.c_double, C.c_size_t, C.c_double,
                                  C.c_double, C.c_size_t, _dp, C.POINTER(CountOut)]

    def err(self):
        return self.L.ha_last_error().decode()

    def tnt_stiefel(self, n, p, rowptr, col, val, X0, params, pack, wrap_hessian=False, repeats=1):
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        col = np.ascontiguousarray(col, dtype=np.int32)
        val = np.ascontiguousarray(val, dtype=np.float64)
        X0 = np.ascontiguousarray(X0, dtype=np.float64).ravel()
        bufs, res = DeviceHarness._result_buffers(n * p, params)
        out = ArgsOut()
        rc = self.L.ha_tnt_stiefel(n, p, _i(rowptr), _i(col), _p(val), _p(X0), C.byref(params), int(pack),
                                   int(wrap_hessian), int(repeats), C.byref(res), C.byref(out))
        r = DeviceHarness._unpack(rc, bufs, res, self.err() if rc else "")
        r["counters"] = _out(out)
        return r

    def tnt_so3n(self, N, ei, ej, Rt, w, R0, params, pack):
        ei = np.ascontiguousarray(ei, dtype=np.int32)
        ej = np.ascontiguousarray(ej, dtype=np.int32)
        Rt = np.ascontiguousarray(Rt, dtype=np.float64)
        w = np.ascontiguousarray(w, dtype=np.float64)
        R0 = np.ascontiguousarray(R0, dtype=np.float64).ravel()
        bufs, res = DeviceHarness._result_buffers(9 * N, params)
        out = ArgsOut()
        rc = self.L.ha_tnt_so3n(N, ei.size, _i(ei), _i(ej), _p(Rt), _p(w), _p(R0), C.byref(params), int(pack),
                                C.byref(res), C.byref(out))
        r = DeviceHarness._unpack(rc, bufs, res, self.err() if rc else "")
        r["counters"] = _out(out)
        return r

    def gd_stiefel(self, n, p, rowptr, col, val, X0, prm, pack, cap=4096):
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int32)
        col = np.ascontiguousarray(col, dtype=np.int32)
        val = np.ascontiguousarray(val, dtype=np.float64)
        X0 = np.ascontiguousarray(X0, dtype=np.float64).ravel()
        x = np.zeros(n * p)
        f, gn = C.c_double(0), C.c_double(0)
        st, it = C.c_int(-1), C.c_size_t(0)
        fv = np.zeros(cap)
        ls = np.zeros(cap, dtype=np.uint64)
        out = ArgsOut()
        rc = self.L.ha_gd_stiefel(n, p, _i(rowptr), _i(col), _p(val), _p(X0), prm["max_iterations"],
                                  prm["gradient_tolerance"], prm["alpha"], prm["beta"], prm["sigma"],
                                  prm["max_ls_iterations"], int(pack), _p(x), C.byref(f), C.byref(gn), C.byref(st),
                                  C.byref(it), cap, _p(fv), ls.ctypes.data_as(_sp), C.byref(out))
        k = min(it.value, cap)
        return dict(rc=rc, err=self.err() if rc else "", x=x, f=f.value, gradfx_norm=gn.value, status=st.value,
                    iterations=it.value, objective_values=fv[:k + 1].copy(),
                    linesearch_iterations=ls[:k].astype(np.int64), counters=_out(out))

    def lsqr_csr(self, A, b, pack, max_iterations=1000, lam=0.0, btol=1e-6, Atol=1e-6, Acond_limit=1e8, Delta=None):
        n = A.shape[0]
        rp, cl, vl, rpt, clt, vlt = DeviceHarness._csr_pair(A)
        b = np.ascontiguousarray(b, dtype=np.float64)
        if Delta is None:
            Delta = float(np.sqrt(np.finfo(np.float64).max))
        x = np.zeros(n)
        xn, it = C.c_double(0), C.c_size_t(0)
        out = ArgsOut()
        rc = self.L.ha_lsqr_csr(n, _i(rp), _i(cl), _p(vl), _i(rpt), _i(clt), _p(vlt), _p(b), max_iterations, lam, btol,
                                Atol, Acond_limit, Delta, int(pack), _p(x), C.byref(xn), C.byref(it), C.byref(out))
        return dict(rc=rc, err=self.err() if rc else "", x=x, xnorm=xn.value, iterations=it.value, counters=_out(out))

    def counting(self, device, solver, g, D, Minv=None, Delta=1e6, max_iterations=100, kappa=1e-10, theta=1.0,
                 stop_at=NEVER, pack=1):
        """Args = {size_t}: a counter of the caller's that the user function increments.  solver 0: STPCG, 1: TNT on the
        quadratic of g, D (pack=0, host vector only: the same TNT call with the empty pack)."""
        g, D = np.ascontiguousarray(g, dtype=np.float64), np.ascontiguousarray(D, dtype=np.float64)
        Mi = np.ascontiguousarray(Minv, dtype=np.float64) if Minv is not None else None
        s, out = np.zeros(g.size), CountOut()
        rc = self.L.ha_counting(int(device), int(solver), int(pack), g.size, _p(g), _p(D), _p(Mi) if Mi is not None else None,
                                Delta, max_iterations, kappa, theta, stop_at, _p(s), C.byref(out))
        return dict(rc=rc, err=self.err() if rc else "", s=s, counter=out.counter, iterations=out.iterations,
                    M_norm=out.M_norm, counters=_out(out.dev))
