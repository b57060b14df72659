"""ctypes loader of tests/cpp/libharness_robust_so3n.so (harness_robust_so3n.cpp): a GNC loop of TNT + reweight on
MI355::RotationAveraging, every round repeated on a fresh problem with the downloaded weights; the planted-outlier problem
of tests/test_gpu_so3n_robust_solve.py and the error measure.  Test infrastructure."""
import ctypes as C
import os

import numpy as np

import so3_cases as sc
from optimization_amd import workloads as wl

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "cpp", "libharness_robust_so3n.so")
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_lp = C.POINTER(C.c_longlong)
# the robust scale and the first mu of the GNC loop (profiles/so3n_robust.md: the two errors they give on the CPU oracle)
C_SCALE, MU0, ROUNDS = 0.15, 64.0, 4


def planted_problem(N=300, noise=0.02, share=0.1, seed=11):
    """ring with chords, inlier noise `noise` rad, `share` of the measurements replaced by random rotations; the start is the
    ground truth perturbed by 0.3 rad.  Returns dict(N, ei, ej, Rt, w, R0, truth, outlier mask)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    ei, ej = (np.asarray(x, dtype=np.int32) for x in wl.pose_graph(N, seed=seed)[:2])
    E = ei.size
    T = sc.round_orth(sc.exp_ld(rng.normal(size=(N, 3)) * 1.5)).astype(sc.LD)
    Rt = sc.round_orth(np.swapaxes(T[ei], 1, 2) @ T[ej] @ sc.exp_ld(rng.normal(size=(E, 3)) * noise))
    out = rng.random(E) < share
    Rt[out] = sc.round_orth(sc.exp_ld(rng.normal(size=(int(out.sum()), 3)) * 1.5))
    R0 = sc.round_orth(T @ sc.exp_ld(rng.normal(size=(N, 3)) * 0.3))
    return dict(N=N, ei=ei, ej=ej, Rt=np.ascontiguousarray(Rt.reshape(E, 9)), w=np.ones(E),
                R0=np.ascontiguousarray(R0.reshape(N, 9)), truth=T.astype(np.float64), outliers=out)


def mean_angular_error(R, truth):
    """mean angle between G R_i and T_i with the global rotation G = polar(sum T_i R_i') (the problem's gauge: R_i -> G R_i)"""
    R, T = np.asarray(R).reshape(-1, 3, 3), np.asarray(truth).reshape(-1, 3, 3)
    U, _, Vt = np.linalg.svd((T @ np.swapaxes(R, 1, 2)).sum(axis=0))
    G = U @ np.diag([1, 1, np.linalg.det(U @ Vt)]) @ Vt
    D = np.swapaxes(G @ R, 1, 2) @ T
    cosang = np.clip((np.trace(D, axis1=1, axis2=2) - 1) / 2, -1, 1)
    return float(np.arccos(cosang).mean())


class RobustSo3nHarness:
    def __init__(self):
        if not os.path.exists(LIB):
            raise FileNotFoundError(LIB + " (run __graft_entry__.build())")
        L = self.L = C.CDLL(LIB)
        L.hr_last_error.restype = C.c_char_p
        L.hr_gnc_so3n.restype = C.c_int
        L.hr_gnc_so3n.argtypes = [C.c_size_t, C.c_size_t, _ip, _ip, _dp, _dp, _dp, C.c_double, C.c_double, C.c_int, _dp, _dp,
                                  _dp, _dp, _lp, _lp]

    def gnc(self, p, c=C_SCALE, mu0=MU0, rounds=ROUNDS):
        N, E = p["N"], p["ei"].size
        R_l2, Rr, Rf, W = np.zeros(9 * N), np.zeros((rounds, 9 * N)), np.zeros((rounds, 9 * N)), np.zeros((rounds, E))
        counts, outl = np.zeros((rounds, 6), dtype=np.longlong), np.zeros(rounds, dtype=np.longlong)
        R0 = np.ascontiguousarray(p["R0"], dtype=np.float64).ravel()
        rc = self.L.hr_gnc_so3n(N, E, p["ei"].ctypes.data_as(_ip), p["ej"].ctypes.data_as(_ip), p["Rt"].ctypes.data_as(_dp),
                                p["w"].ctypes.data_as(_dp), R0.ctypes.data_as(_dp), c, mu0, rounds, R_l2.ctypes.data_as(_dp),
                                Rr.ctypes.data_as(_dp), Rf.ctypes.data_as(_dp), W.ctypes.data_as(_dp),
                                counts.ctypes.data_as(_lp), outl.ctypes.data_as(_lp))
        return dict(rc=rc, err=self.L.hr_last_error().decode() if rc else "", R_l2=R_l2, R_rounds=Rr, R_fresh=Rf, W=W,
                    counts=counts, outliers=outl)
