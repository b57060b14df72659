"""Robust reweighting of the SO(3)^N problem (mi_so3n_reweight) in numpy longdouble: the unweighted chordal residual r_e, the
weight functions phi and losses rho (rho' = r phi), the new weights, the three info sums and the Gauss-Newton degree scaling
-- a helper module for test_cpu_so3n_robust.py and test_gpu_so3n_robust.py (not a conftest).  Built on so3_cases (cases,
longdouble rotations); the cases and evaluation points the GPU tests use are defined here once."""
import functools
from collections import namedtuple

import numpy as np

import so3_cases as sc
from so3_cases import LD

KINDS = ("l2", "huber", "cauchy", "geman_mcclure")
SCALES = (0.05, 0.5, 3.0)
EPS = float(np.finfo(np.float64).eps)


def weight_tol(c):
    """|w_e - w_ref| <= 64 eps max(1, 1/c) |w0_e|: r <= 2 sqrt 2 on rotations with an fp64 error <~ 30 eps (nine differences
    of three-term products), every phi Lipschitz in r with constant <= 1.04 / c, a factor 2 over the product"""
    return 64 * EPS * max(1.0, 1.0 / c)


def residual_norms(c, R=None):
    """r_e = |R_j - R_i Rt_e|_F, longdouble"""
    R = np.asarray(c.R if R is None else R).astype(LD).reshape(c.N, 3, 3)
    if c.ei.size == 0:
        return np.zeros(0, dtype=LD)
    d = R[c.ej.astype(np.int64)] - R[c.ei.astype(np.int64)] @ c.Rt.astype(LD).reshape(-1, 3, 3)
    return np.sqrt((d * d).sum(axis=(1, 2)))


def phi(kind, r, c):
    r, c = np.asarray(r, dtype=LD), LD(c)
    if kind == "l2":
        return np.ones_like(r)
    if kind == "huber":
        return np.where(r <= c, LD(1), c / np.where(r > 0, r, LD(1)))
    s = r * r / (c * c)
    if kind == "cauchy":
        return 1 / (1 + s)
    if kind == "geman_mcclure":
        return 1 / ((1 + s) * (1 + s))
    raise ValueError(kind)


def rho(kind, r, c):
    r, c = np.asarray(r, dtype=LD), LD(c)
    if kind == "l2":
        return r * r / 2
    if kind == "huber":
        return np.where(r <= c, r * r / 2, c * r - c * c / 2)
    s = r * r / (c * c)
    if kind == "cauchy":
        return c * c / 2 * np.log1p(s)
    if kind == "geman_mcclure":
        return r * r / 2 / (1 + s)
    raise ValueError(kind)


Reweighted = namedtuple("Reweighted", "r phi w robust_cost weighted_cost outliers")


def reweight(c, kind, scale, R=None):
    r = residual_norms(c, R)
    p = phi(kind, r, scale)
    w = c.w.astype(LD) * p
    return Reweighted(r, p, w, (c.w.astype(LD) * rho(kind, r, scale)).sum(), (w * r * r / 2).sum(), int((p < LD(1) / 2).sum()))


def gn_scaling(c, w):
    """diag(1 / sqrt(2 degw_i)), each three times; 1 where degw_i is not positive"""
    degw = np.zeros(c.N, dtype=LD)
    np.add.at(degw, c.ei.astype(np.int64), np.asarray(w, dtype=LD))
    np.add.at(degw, c.ej.astype(np.int64), np.asarray(w, dtype=LD))
    d = np.where(degw > 0, 1 / np.sqrt(2 * np.where(degw > 0, degw, LD(1))), LD(1))
    return np.repeat(d, 3)


# ------------------------------------------------------------------------------------------------------------------
# the cases and points of the GPU tests
# ------------------------------------------------------------------------------------------------------------------
GRAPHS = {
    "tiny_2": lambda: sc.tiny(2),
    "tiny_3": lambda: sc.tiny(3),
    "ring_chords_1500": lambda: sc.ring_chords(1500, "linspace"),
    "hub": lambda: sc.hub(False, "linspace"),
    "isolated": lambda: sc.isolated(),
    "multigraph": lambda: sc.multigraph("linspace"),
    "nonrot_1025": lambda: sc.nonrot("scaled", 1025),
    "powerlaw_5000": lambda: sc.powerlaw(5000),
}
POINTS = ("random", "outliers")
VARIANTS = tuple(f"{g}:{p}" for g in GRAPHS for p in POINTS) + ("special_point:own",)


def _random_rotations(n, rng, scale=1.5):
    return sc.round_orth(sc.exp_ld(rng.normal(size=(n, 3)) * scale))


@functools.lru_cache(maxsize=None)
def variant(name):
    """Case for "graph:point".  random: the graph's measurements at a random point of SO(3)^N.  outliers: the graph's own
    point taken as the ground truth -- measurements R_i' R_j with 0.02 rad of noise, about 10 % of them replaced by random
    rotations (a measurement that is not a rotation stays what it is: the 9-component form).  own: the case as it is."""
    g, p = name.split(":")
    if g == "special_point":
        return sc.special_point()
    c = GRAPHS[g]()
    rng = np.random.Generator(np.random.PCG64(abs(hash_name(name))))
    if p == "random":
        return c._replace(name=name, R=np.ascontiguousarray(_random_rotations(c.N, rng).reshape(c.N, 9)))
    E = c.ei.size
    T = c.R.astype(LD).reshape(c.N, 3, 3)
    Rt = sc.round_orth(np.swapaxes(T[c.ei], 1, 2) @ T[c.ej] @ sc.exp_ld(rng.normal(size=(E, 3)) * 0.02))
    out = rng.random(E) < 0.1
    if E >= 2:
        out[0], out[1] = True, False
    Rt[out] = _random_rotations(int(out.sum()), rng)
    Rt = Rt.reshape(E, 9)
    M = c.Rt.reshape(E, 3, 3)
    keep = np.abs(np.swapaxes(M, 1, 2) @ M - np.eye(3)).max(axis=(1, 2)) > 1e-13
    Rt[keep] = c.Rt[keep]
    return c._replace(name=name, Rt=np.ascontiguousarray(Rt))


def hash_name(name):
    """a seed that does not depend on the interpreter's string hashing"""
    return int.from_bytes(name.encode(), "little") % (2 ** 31 - 1)


@functools.lru_cache(maxsize=None)
def reference(name, kind, scale):
    return reweight(variant(name), kind, scale)
