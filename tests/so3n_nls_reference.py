"""Chordal rotation averaging as a nonlinear least-squares problem: a numpy longdouble restatement of F, dF and dF* from the
formulas (a helper module for test_cpu_so3n_nls.py and test_gpu_so3n_nls.py; not a conftest), independent of the C++ of
tests/cpp/harness_tnls_so3n.cpp and of the kernels:

    F(R)_e     = sqrt(w_e) (R_j - R_i Rt_e)                                    e = (i -> j), 9 doubles per edge, row-major
    (dF xi)_e  = sqrt(w_e) (R_j hat(xi_j) - R_i hat(xi_i) Rt_e)
    (dF* Y)_i  = sum_{e: i first node} -sqrt(w_e) vee(R_i' Y_e Rt_e')  +  sum_{e: i second node} sqrt(w_e) vee(R_i' Y_e)
    vee(M)     = (M21 - M12, M02 - M20, M10 - M01)                             [(M7 - M5, M2 - M6, M3 - M1) row-major]

and the graphs both test files run on."""
import functools
from collections import namedtuple

import numpy as np

from optimization_amd import workloads as wl
from so3_cases import LD, exp_ld, hat_ld, round_orth

Graph = namedtuple("Graph", "name N ei ej Rt w R")


def vee_ld(M):
    return np.stack([M[:, 2, 1] - M[:, 1, 2], M[:, 0, 2] - M[:, 2, 0], M[:, 1, 0] - M[:, 0, 1]], axis=1)


class NlsRef:
    def __init__(self, g, R=None):
        self.N, self.E = g.N, g.ei.size
        self.ei, self.ej = g.ei.astype(np.int64), g.ej.astype(np.int64)
        self.Rt = g.Rt.astype(LD).reshape(-1, 3, 3)
        self.sw = np.sqrt(g.w.astype(LD))
        self.R = np.asarray(g.R if R is None else R).astype(LD).reshape(g.N, 3, 3)

    def F(self, R=None):
        R = self.R if R is None else np.asarray(R, dtype=LD).reshape(self.N, 3, 3)
        return (self.sw[:, None, None] * (R[self.ej] - R[self.ei] @ self.Rt)).ravel()

    def dF(self, xi):
        K = hat_ld(xi)
        V = self.R @ K
        return (self.sw[:, None, None] * (V[self.ej] - V[self.ei] @ self.Rt)).ravel()

    def dFt(self, Y):
        Y = np.asarray(Y, dtype=LD).reshape(self.E, 3, 3)
        Rt_ = np.swapaxes(self.R, 1, 2)
        first = -self.sw[:, None] * vee_ld(Rt_[self.ei] @ Y @ np.swapaxes(self.Rt, 1, 2))
        second = self.sw[:, None] * vee_ld(Rt_[self.ej] @ Y)
        out = np.zeros((self.N, 3), dtype=LD)
        np.add.at(out, self.ei, first)
        np.add.at(out, self.ej, second)
        return out.ravel()

    def retract(self, xi, R=None):
        R = self.R if R is None else np.asarray(R, dtype=LD).reshape(self.N, 3, 3)
        return (R @ exp_ld(xi)).ravel()


def _pose(name, N, seed=7, scale=None):
    ei, ej, Rt, w, _, Rinit = wl.pose_graph(N, seed=seed)
    if scale is not None:
        Rt = Rt * scale          # not rotations: the problem takes the 9-component measurement forms
    return Graph(name, N, ei, ej, np.ascontiguousarray(Rt), np.linspace(0.5, 1.5, ei.size) if scale is None and N == 65 else w,
                 np.ascontiguousarray(Rinit))


def _star_chain():
    """hub 0 of degree 70 (alternating orientation), 70 leaves of degree 1, then a chain hanging off the hub's last
    leaf... no: off a node of its own, so that the leaves keep degree 1.  E = 70 + 230 = 300 (no multiple of 256)."""
    N = 1 + 70 + 231
    ei, ej = [], []
    for k in range(70):
        a, b = (0, 1 + k) if k % 2 == 0 else (1 + k, 0)
        ei.append(a)
        ej.append(b)
    for k in range(230):
        ei.append(71 + k)
        ej.append(72 + k)
    ei, ej = np.asarray(ei, dtype=np.int32), np.asarray(ej, dtype=np.int32)
    E = ei.size
    assert E == 300 and E % 256 != 0
    rng = np.random.Generator(np.random.PCG64(301))
    Rtrue = round_orth(exp_ld(rng.normal(size=(N, 3)) * 1.5)).astype(LD)
    noise = exp_ld(rng.normal(size=(E, 3)) * 0.05)
    Rt = round_orth(np.swapaxes(Rtrue[ei], 1, 2) @ Rtrue[ej] @ noise)
    R = round_orth(Rtrue @ exp_ld(rng.normal(size=(N, 3)) * 0.2))
    w = np.linspace(0.25, 4.0, E)
    return Graph("star_chain", N, ei, ej, np.ascontiguousarray(Rt.reshape(E, 9)), w, np.ascontiguousarray(R.reshape(N, 9)))


_GRAPHS = {
    "pose_40": lambda: _pose("pose_40", 40),
    "pose_150": lambda: _pose("pose_150", 150),
    "pose_65": lambda: _pose("pose_65", 65),            # padding lanes in the last (second) slice; weights 0.5 ... 1.5
    "pose_1100": lambda: _pose("pose_1100", 1100),      # a second sigma = 1024 window
    "star_chain": _star_chain,
    "nonrot_1100": lambda: _pose("nonrot_1100", 1100, scale=1.01),
}
GRAPH_NAMES = tuple(_GRAPHS)


@functools.lru_cache(maxsize=None)
def graph(name):
    g = _GRAPHS[name]()
    assert g.name == name
    return g


def degw(g):
    d = np.zeros(g.N, dtype=LD)
    np.add.at(d, g.ei, g.w.astype(LD))
    np.add.at(d, g.ej, g.w.astype(LD))
    return d


@functools.lru_cache(maxsize=None)
def probes(name):
    """(xi (3N), Y (9E), u (9E), v (3N)) in double: inputs of the single applications and of the fused forms"""
    g = graph(name)
    rng = np.random.Generator(np.random.PCG64(11 + g.N))
    return (rng.normal(size=3 * g.N), rng.normal(size=9 * g.ei.size), rng.normal(size=9 * g.ei.size),
            rng.normal(size=3 * g.N))


def rel_inf(a, exact):
    """max |a - exact| / max |exact|, the difference in longdouble"""
    a, exact = np.asarray(a, dtype=LD), np.asarray(exact, dtype=LD)
    return float(np.max(np.abs(a - exact)) / np.max(np.abs(exact)))
