"""ctypes loader of tests/cpp/libharness_lsqr_observer.so (harness_lsqr_observer.cpp): LinearAlgebra::LSQR with a recording
user function through one templated driver, on the host vector (device=0, the reference's arithmetic) and on
MI355::DeviceVector (device=1, the fused observed solve), with the empty pack and with Args = {size_t, Vec}; and the
tridiagonal test operator shared with the C-ABI tests.  Test infrastructure."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "cpp", "libharness_lsqr_observer.so")
NEVER = C.c_size_t(-1).value
REC_COLS = ("k", "xnorm", "xx", "rbar_norm", "Arnorm", "Anorm", "Acond")
_dp = C.POINTER(C.c_double)


class LsqrObsOut(C.Structure):
    _fields_ = [("nrec", C.c_size_t), ("counter", C.c_size_t), ("iterations", C.c_size_t), ("xnorm", C.c_double),
                ("fused_lsqr_solves", C.c_ulonglong), ("generic_lsqr_solves", C.c_ulonglong), ("syncs", C.c_size_t),
                ("seconds", C.c_double)]


def tridiagonal(n, seed=0):
    """(lo, di, up, b): a well-conditioned non-symmetric tridiagonal operator (row i: lo[i], di[i], up[i]) and a right-hand
    side; the same recipe at every n"""
    rng = np.random.default_rng(1000 + seed)
    di = 3.0 + rng.random(n)
    lo = -1.0 + .2 * rng.random(n)
    up = .5 + rng.random(n)
    b = rng.normal(size=n)
    return lo, di, up, b


def tridiagonal_csr(lo, di, up, transpose=False):
    """(rowptr, col, val) of the tridiagonal, or of its transpose"""
    import scipy.sparse as sps
    n = di.size
    A = sps.diags([lo[1:], di, up[:n - 1]], [-1, 0, 1], format="csr") if n > 1 else sps.csr_matrix(di.reshape(1, 1))
    if transpose:
        A = sps.csr_matrix(A.T)
    A.sort_indices()
    return (np.ascontiguousarray(A.indptr, dtype=np.int32), np.ascontiguousarray(A.indices, dtype=np.int32),
            np.ascontiguousarray(A.data, dtype=np.float64))


def _p(a):
    return a.ctypes.data_as(_dp)


class LsqrObserverHarness:
    def __init__(self):
        if not os.path.exists(LIB):
            raise FileNotFoundError(LIB + " (run __graft_entry__.build())")
        self.L = C.CDLL(LIB)
        self.L.hl_last_error.restype = C.c_char_p
        self.L.hl_observed_tridiag.restype = C.c_int
        self.L.hl_observed_tridiag.argtypes = [C.c_int, C.c_int, C.c_size_t, _dp, _dp, _dp, _dp, C.c_size_t, C.c_double,
                                               C.c_double, C.c_double, C.c_double, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int,
                                               _dp, C.c_size_t, _dp, C.POINTER(LsqrObsOut)]

    def err(self):
        return self.L.hl_last_error().decode()

    def tridiag(self, device, pack, lo, di, up, b, max_iterations=1000, lam=0.0, btol=1e-6, Atol=1e-6, Delta=None,
                stop_at=NEVER, throw_at=NEVER, no_fused=False, rec_cap=2048, user_function=True, repeats=1):
        """user_function=False: the call without a user function (no record; the un-observed fused solve on the device)"""
        if not user_function:
            rec_cap = 0
        lo, di, up, b = (np.ascontiguousarray(a, dtype=np.float64) for a in (lo, di, up, b))
        if Delta is None:
            Delta = float(np.sqrt(np.finfo(np.float64).max))
        rec, x, out = np.zeros((max(rec_cap, 1), len(REC_COLS))), np.zeros(di.size), LsqrObsOut()
        rc = self.L.hl_observed_tridiag(int(device), int(pack), di.size, _p(lo), _p(di), _p(up), _p(b), max_iterations,
                                        lam, btol, Atol, Delta, int(user_function), stop_at, throw_at, int(no_fused),
                                        int(repeats),
                                        _p(rec) if rec_cap else None, rec_cap, _p(x), C.byref(out))
        r = {k: getattr(out, k) for k, _ in LsqrObsOut._fields_}
        r.update(rc=rc, err=self.err() if rc else "", x=x, calls=out.nrec, rec=rec[:min(out.nrec, rec_cap)].copy())
        return r
