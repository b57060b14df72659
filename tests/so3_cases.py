"""SO(3)^N edge cases and a longdouble reference (a helper module for test_cpu_so3n_reference.py and
test_gpu_so3n_edges.py; not a conftest).

(a) Case generators: irregular graphs (hub, isolated nodes and slices, multigraph, path, power law), weight patterns
(zero, negative, twelve decades) and the rotations on which Shepperd's matrix -> quaternion branch changes sides, placed
where the device gathers them (hub and its neighbours, both ends of duplicated edges) and used as measurements in both
directions.  Every rotation is built in longdouble, rounded once to double and re-orthonormalised (one Newton polar step
in longdouble), so that a point is a rotation to rounding and the quaternion gather of the device stays within
rounding of the matrix form.

(b) A longdouble reference of the objective, gradient, Hessian, block-Jacobi preconditioner and retraction, written from
the formulas in the header comments of optimization_amd/csrc/so3.hip and oracle/problems.c: the edge-loop objective, the
connection Laplacian, the OPERATOR form of the Hessian (no assembled blocks) and exp through sin / cos with no series
switch."""
import functools
from collections import namedtuple

import numpy as np

from optimization_amd import workloads as wl

LD = np.longdouble
Case = namedtuple("Case", "name N ei ej Rt w R")

# |xi| of the retraction sweep: both sides of and at the series switch (1e-4), 0, pi, 2 pi and a large angle
SWEEP = (0.0, 1e-7, float(np.nextafter(1e-4, 0.0)), 1e-4, float(np.nextafter(1e-4, 1.0)), 1.0, float(np.pi),
         float(2 * np.pi), 10.0)
FORMS = {"default": {}, "no_quat": {"SO3_NO_QUAT": 1}, "no_rquat": {"SO3_NO_RQUAT": 1},
         "no_quat_no_rquat": {"SO3_NO_QUAT": 1, "SO3_NO_RQUAT": 1}, "sort_nbr": {"SO3_SORT_NBR": 1}}


# ------------------------------------------------------------------------------------------------------------------
# longdouble building blocks
# ------------------------------------------------------------------------------------------------------------------
def hat_ld(x):
    x = np.asarray(x, dtype=LD).reshape(-1, 3)
    K = np.zeros((x.shape[0], 3, 3), dtype=LD)
    K[:, 0, 1], K[:, 0, 2] = -x[:, 2], x[:, 1]
    K[:, 1, 0], K[:, 1, 2] = x[:, 2], -x[:, 0]
    K[:, 2, 0], K[:, 2, 1] = -x[:, 1], x[:, 0]
    return K


def vee2_ld(T):
    """vee(T - T') = (T32 - T23, T13 - T31, T21 - T12)"""
    return np.stack([T[:, 2, 1] - T[:, 1, 2], T[:, 0, 2] - T[:, 2, 0], T[:, 1, 0] - T[:, 0, 1]], axis=1)


def exp_ld(xi):
    """exp(hat(xi)) = I + sin(t)/t K + (1 - cos t)/t^2 K^2 in longdouble, no series: (1 - cos t) = 2 sin^2(t/2), and the
    exact limits 1 and 1/2 at t = 0 itself"""
    xi = np.asarray(xi, dtype=LD).reshape(-1, 3)
    th = np.sqrt((xi * xi).sum(axis=1))
    safe = np.where(th > 0, th, LD(1))
    a = np.where(th > 0, np.sin(safe) / safe, LD(1))
    sh = np.sin(safe / 2) / safe
    b = np.where(th > 0, 2 * sh * sh, LD(1) / 2)
    K = hat_ld(xi)
    return np.eye(3, dtype=LD) + a[:, None, None] * K + b[:, None, None] * (K @ K)


def round_orth(R):
    """longdouble (n,3,3) -> double, rounded once, then one Newton polar step R (3 I - R'R) / 2 in longdouble"""
    R = np.asarray(R, dtype=LD).reshape(-1, 3, 3).astype(np.float64).astype(LD)
    RtR = np.swapaxes(R, 1, 2) @ R
    R = R @ ((3 * np.eye(3, dtype=LD) - RtR) / 2)
    return R.astype(np.float64)


def _axis_angle(axis, angle):
    axis = np.asarray(axis, dtype=LD)
    axis = axis / np.sqrt((axis * axis).sum())
    return round_orth(exp_ld(axis * LD(angle)))[0]


def _half_turn(axis):
    """exactly 2 n n' - I (no sine of a rounded pi)"""
    n = np.asarray(axis, dtype=LD)
    n = n / np.sqrt((n * n).sum())
    return round_orth((2 * np.outer(n, n) - np.eye(3, dtype=LD))[None])[0]


@functools.lru_cache(maxsize=None)
def special_rotations():
    """[(name, 3x3 double)]: where Shepperd's branch (device: trace > 0, else the largest diagonal entry with `>`; host:
    the largest of trace and diagonal with `>=`) changes sides or ties"""
    t23 = 2 * np.pi / 3
    gen = np.array([0.3, -0.5, 0.81])
    out = [("identity", np.eye(3)),
           ("pi_x", _half_turn([1, 0, 0])), ("pi_y", _half_turn([0, 1, 0])), ("pi_z", _half_turn([0, 0, 1])),
           ("pi_110", _half_turn([1, 1, 0])), ("pi_111", _half_turn([1, 1, 1])),
           # trace exactly 0 with all three diagonal entries tied: the cyclic permutation and its inverse
           ("perm", np.array([[0., 0, 1], [1, 0, 0], [0, 1, 0]])), ("perm_t", np.array([[0., 1, 0], [0, 0, 1], [1, 0, 0]])),
           ("t23", _axis_angle(gen, t23)), ("t23_below", _axis_angle(gen, np.nextafter(t23, 0))),
           ("t23_above", _axis_angle(gen, np.nextafter(t23, 4))),
           # (rounding the matrix moves the trace by about as much as one ulp of the angle does: a few ulps of the angle to
           # either side, about each dominant axis, put the trace on a known side of 0)
           ("t23_x_lo", _axis_angle([0.9, 0.3, -0.1], t23 - 2e-15)), ("t23_x_hi", _axis_angle([0.9, 0.3, -0.1], t23 + 2e-15)),
           ("t23_y_lo", _axis_angle([0.2, -0.95, 0.1], t23 - 2e-15)), ("t23_y_hi", _axis_angle([0.2, -0.95, 0.1], t23 + 2e-15)),
           ("t23_z_lo", _axis_angle([0.1, 0.2, 0.97], t23 - 2e-15)), ("t23_z_hi", _axis_angle([0.1, 0.2, 0.97], t23 + 2e-15)),
           ("near_pi", _axis_angle([0.6, -0.3, 0.74], np.pi - 1e-8)),
           ("near_pi_x", _axis_angle([0.99, 0.05, 0.02], np.pi - 1e-8)),
           # two largest diagonal entries equal, trace < 0 (rotation by 2.5 about a face diagonal)
           ("tie_xy", _axis_angle([1, 1, 0], 2.5)), ("tie_yz", _axis_angle([0, 1, 1], 2.5)),
           ("tie_xz", _axis_angle([1, 0, 1], 2.5))]
    return out


def device_branch(R):
    """the branch mat_to_quat (so3.hip) takes: 0 trace, 1 x, 2 y, 3 z"""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        return 0
    if R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        return 1
    return 2 if R[1, 1] > R[2, 2] else 3


def host_branch(M):
    """the branch to_quat (mi_so3n_create) takes"""
    M = np.asarray(M, dtype=np.float64).reshape(3, 3)
    tr = M[0, 0] + M[1, 1] + M[2, 2]
    if tr >= M[0, 0] and tr >= M[1, 1] and tr >= M[2, 2]:
        return 0
    if M[0, 0] >= M[1, 1] and M[0, 0] >= M[2, 2]:
        return 1
    return 2 if M[1, 1] >= M[2, 2] else 3


# ------------------------------------------------------------------------------------------------------------------
# (a) cases
# ------------------------------------------------------------------------------------------------------------------
def _weights(kind, ei, ej, rng, zero_node=5):
    E = ei.size
    if kind == "ones":
        return np.ones(E)
    if kind == "linspace":
        return np.linspace(0.5, 1.5, E)
    if kind == "spread":          # twelve decades
        return 10.0 ** rng.uniform(-6, 6, size=E)
    if kind == "some_zero":       # every 7th edge exactly 0
        w = np.linspace(0.5, 1.5, E)
        w[::7] = 0.0
        return w
    if kind == "node_zero":       # every edge of one node exactly 0 (its block D_i is singular)
        w = np.linspace(0.5, 1.5, E)
        w[(ei == zero_node) | (ej == zero_node)] = 0.0
        return w
    if kind == "negative":        # a few negative ones, small enough that every D_i stays well conditioned
        w = np.ones(E)
        w[rng.choice(E, size=min(5, E), replace=False)] = -0.25
        return w
    raise ValueError(kind)


def _build(name, N, ei, ej, seed, wkind, fixed=None, exact_edges=(), zero_node=5):
    """Rotation-averaging problem on the given graph, as workloads.pose_graph builds it (Rt_e = R_i' R_j noise, sigma =
    0.05; the point = truth perturbed by 0.2) but in longdouble.  fixed: {node: 3x3} rotations held exactly, at the truth
    AND at the point.  exact_edges: edges whose measurement carries no noise -- with R_i = I exactly the special R_j."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ei, ej = np.asarray(ei, dtype=np.int32), np.asarray(ej, dtype=np.int32)
    E = ei.size
    Rtrue = round_orth(exp_ld(rng.normal(size=(N, 3)) * 1.5))
    fixed = fixed or {}
    for k, S in fixed.items():
        Rtrue[k] = S
    noise = exp_ld(rng.normal(size=(E, 3)) * 0.05)
    if len(exact_edges):
        noise[np.asarray(exact_edges)] = np.eye(3, dtype=LD)
    Tl = Rtrue.astype(LD)
    Rt = round_orth(np.swapaxes(Tl[ei], 1, 2) @ Tl[ej] @ noise) if E else np.zeros((0, 3, 3))
    R = round_orth(Tl @ exp_ld(rng.normal(size=(N, 3)) * 0.2))
    for k, S in fixed.items():
        R[k] = S
    w = _weights(wkind, ei, ej, rng, zero_node) if E else np.zeros(0)
    return Case(name, N, ei, ej, np.ascontiguousarray(Rt.reshape(E, 9)), np.ascontiguousarray(w, dtype=np.float64),
                np.ascontiguousarray(R.reshape(N, 9)))


def ring_chords(N, wkind, seed=None):
    ei, ej = wl.pose_graph(N, seed=N if seed is None else seed)[:2]
    return _build(f"ring_chords_{N}_{wkind}", N, ei, ej, 1000 + N, wkind)


def hub(at_end, wkind, N=1500):
    """one node joined to every other node (degree N - 1 > the 1024-node window of the degree sort) plus a ring; the hub
    is the identity and its first neighbours are the special rotations, the spokes to them noise-free: as the hub is
    the tail (hub first) or the head (hub last) of its spokes, each special rotation or its transpose is a measurement"""
    h = N - 1 if at_end else 0
    others = np.array([i for i in range(N) if i != h])
    if at_end:
        ei, ej = others, np.full(N - 1, h)
    else:
        ei, ej = np.full(N - 1, h), others
    ei = np.concatenate([ei, np.arange(N)])
    ej = np.concatenate([ej, (np.arange(N) + 1) % N])
    sp = special_rotations()
    fixed = {h: np.eye(3)}
    for k, (_, S) in enumerate(sp):
        fixed[int(others[k])] = S
    return _build(f"hub_{'last' if at_end else 'first'}_{wkind}", N, ei, ej, 77 + at_end, wkind, fixed,
                  exact_edges=np.arange(len(sp)))


def isolated(N=1500, wkind="ones"):
    """nodes 0 and N - 1 and the whole slice 128..191 without edges"""
    alive = np.array([i for i in range(1, N - 1) if not 128 <= i < 192])
    ei, ej = alive[:-1], alive[1:]
    rng = np.random.Generator(np.random.PCG64(3))
    ca, cb = rng.choice(alive, size=2 * N), rng.choice(alive, size=2 * N)
    keep = ca != cb
    return _build(f"isolated_{N}", N, np.concatenate([ei, ca[keep]]), np.concatenate([ej, cb[keep]]), 31, wkind)


def tiny(N):
    """N = 1 with E = 0, N = 2 with E = 1"""
    ei = np.arange(N - 1)
    return _build(f"tiny_{N}", N, ei, ei + 1, 40 + N, "linspace")


def multigraph(wkind, N=700):
    """ring + chords, plus pairs (a, b) with R_a = I and R_b special: a -> b twice (one measurement exactly the special
    rotation, one noisy; different weights) and b -> a (exactly its transpose)"""
    ei, ej = (x.astype(np.int64) for x in wl.pose_graph(N, seed=13)[:2])
    sp = special_rotations()
    fixed, extra_i, extra_j, exact = {}, [], [], []
    for k, (_, S) in enumerate(sp):
        a, b = 16 * k + 3, 16 * k + 9
        fixed[a], fixed[b] = np.eye(3), S
        extra_i += [a, a, b]
        extra_j += [b, b, a]
        exact += [3 * k, 3 * k + 2]
    E0 = len(extra_i)
    # the special pairs first (their edge numbers are the exact ones), then the generic graph with every 50th edge doubled
    # and every 70th also present in the other orientation
    ei2 = np.concatenate([extra_i, ei, ei[::50], ej[::70]])
    ej2 = np.concatenate([extra_j, ej, ej[::50], ei[::70]])
    assert E0 == 3 * len(sp)
    return _build(f"multigraph_{wkind}", N, ei2, ej2, 55, wkind, fixed, exact_edges=np.array(exact), zero_node=3)


def path(N=300):
    return _build(f"path_{N}", N, np.arange(N - 1), np.arange(1, N), 61, "linspace")


def powerlaw(N=5000):
    """seeded random degrees from 1 to about 300 (Pareto tail)"""
    rng = np.random.Generator(np.random.PCG64(9))
    deg = np.minimum(300, np.floor(rng.pareto(1.2, size=N)).astype(np.int64) + 1)
    half = np.maximum(1, deg // 2)    # every edge counts at both ends
    half[:3] = (297, 248, 1)          # (the ends of the range, whatever the draw)
    ei = np.repeat(np.arange(N), half)
    ej = rng.integers(0, N, size=ei.size)
    ej = np.where(ej == ei, (ej + 1) % N, ej)
    return _build(f"powerlaw_{N}", N, ei, ej, 71, "linspace")


def nonrot(kind, N=1025):
    """one measurement that is not a rotation: the whole problem must take the 9-component form"""
    c = ring_chords(N, "linspace", seed=17)
    Rt = c.Rt.copy()
    e = 2 * N + 11
    if kind == "scaled":
        Rt[e] *= 1 + 1e-6
    else:
        Rt[e] += 1e-3 * np.random.Generator(np.random.PCG64(5)).normal(size=9)
    return c._replace(name=f"nonrot_{kind}", Rt=Rt)


def special_point():
    """a small ring-and-chords problem whose whole point is the special rotations (repeated): the retraction sweep ON
    them, and every gather through them"""
    sp = special_rotations()
    N = 4 * len(sp)
    ei, ej = wl.pose_graph(N, seed=23)[:2]
    fixed = {i: sp[i % len(sp)][1] for i in range(N)}
    return _build("special_point", N, ei, ej, 91, "linspace", fixed)


_CASES = {
    "ring_chords_1023_ones": lambda: ring_chords(1023, "ones"),
    "ring_chords_1024_linspace": lambda: ring_chords(1024, "linspace"),
    "ring_chords_1025_spread": lambda: ring_chords(1025, "spread"),
    "ring_chords_2049_some_zero": lambda: ring_chords(2049, "some_zero"),
    "ring_chords_1024_node_zero": lambda: ring_chords(1024, "node_zero"),
    "ring_chords_1024_negative": lambda: ring_chords(1024, "negative"),
    "hub_first_linspace": lambda: hub(False, "linspace"),
    "hub_last_spread": lambda: hub(True, "spread"),
    "hub_first_some_zero": lambda: hub(False, "some_zero"),
    "isolated_1500": lambda: isolated(),
    "tiny_1": lambda: tiny(1),
    "tiny_2": lambda: tiny(2),
    "multigraph_linspace": lambda: multigraph("linspace"),
    "multigraph_negative": lambda: multigraph("negative"),
    "multigraph_node_zero": lambda: multigraph("node_zero"),
    "path_300": lambda: path(),
    "powerlaw_5000": lambda: powerlaw(),
    "nonrot_scaled": lambda: nonrot("scaled"),
    "nonrot_perturbed": lambda: nonrot("perturbed"),
    "special_point": special_point,
}
CASE_NAMES = tuple(_CASES)
NONROT_CASES = ("nonrot_scaled", "nonrot_perturbed")
STRUCTURE_CASES = ("hub_first_linspace", "hub_last_spread", "multigraph_linspace", "multigraph_negative",
                   "nonrot_scaled", "nonrot_perturbed")


@functools.lru_cache(maxsize=None)
def case(name):
    c = _CASES[name]()
    assert c.name == name, (c.name, name)
    return c


def singular_nodes(c):
    """nodes whose diagonal block D_i is exactly zero: no edge, or every incident weight exactly 0"""
    aw = np.zeros(c.N)
    np.add.at(aw, c.ei, np.abs(c.w))
    np.add.at(aw, c.ej, np.abs(c.w))
    return aw == 0


def sweep_xi(c, mag, seed=0):
    """a tangent vector whose every block has length `mag`: the first three nodes along x, y, z (|xi| is then `mag`
    itself in double), the others along random axes"""
    rng = np.random.Generator(np.random.PCG64(seed + 101))
    ax = rng.normal(size=(c.N, 3)).astype(LD)
    ax /= np.sqrt((ax * ax).sum(axis=1))[:, None]
    ax[:min(3, c.N)] = np.eye(3, dtype=LD)[:min(3, c.N)]
    return np.ascontiguousarray((ax * LD(mag)).astype(np.float64).ravel())


# ------------------------------------------------------------------------------------------------------------------
# (b) the longdouble reference
# ------------------------------------------------------------------------------------------------------------------
class So3Ref:
    def __init__(self, c, R=None):
        self.N, self.ei, self.ej = c.N, c.ei.astype(np.int64), c.ej.astype(np.int64)
        self.Rt = c.Rt.astype(LD).reshape(-1, 3, 3)
        self.w = c.w.astype(LD)
        self.R = np.asarray(c.R if R is None else R).astype(LD).reshape(c.N, 3, 3)
        self._C = None

    def _laplacian(self, Y):
        """(L Y)_j += w (Y_j - Y_i Rt),  (L Y)_i += w (Y_i - Y_j Rt')   for e = (i -> j)"""
        out = np.zeros((self.N, 3, 3), dtype=LD)
        if self.ei.size:
            w = self.w[:, None, None]
            terms = np.concatenate([w * (Y[self.ej] - Y[self.ei] @ self.Rt),
                                    w * (Y[self.ei] - Y[self.ej] @ np.swapaxes(self.Rt, 1, 2))])
            nodes = np.concatenate([self.ej, self.ei])
            order = np.argsort(nodes, kind="stable")
            present, start = np.unique(nodes[order], return_index=True)
            out[present] = np.add.reduceat(terms[order], start, axis=0)     # (every segment is non-empty)
        return out

    def f(self, chunk=1 << 18):
        """1/2 sum_e w_e |R_j - R_i Rt_e|_F^2"""
        acc = LD(0)
        for a in range(0, self.ei.size, chunk):
            s = slice(a, a + chunk)
            d = self.R[self.ej[s]] - self.R[self.ei[s]] @ self.Rt[s]
            acc += (self.w[s] * (d * d).sum(axis=(1, 2))).sum()
        return acc / 2

    def _Q(self):
        return np.swapaxes(self.R, 1, 2) @ self._laplacian(self.R)

    def grad(self):
        """grad_i = vee(Q_i - Q_i'),  Q_i = R_i' (L R)_i"""
        return vee2_ld(self._Q()).ravel()

    def symQ(self):
        if self._C is None:
            Q = self._Q()
            self._C = (Q + np.swapaxes(Q, 1, 2)) / 2
        return self._C

    def hess(self, xi):
        """Hess[xi]_i = vee(T_i - T_i'),  T_i = R_i' (L V)_i - hat(xi_i) sym(Q_i),  V_i = R_i hat(xi_i)"""
        K = hat_ld(xi)
        T = np.swapaxes(self.R, 1, 2) @ self._laplacian(self.R @ K) - K @ self.symQ()
        return vee2_ld(T).ravel()

    def precon(self, v):
        """D_i^-1 v_i,  D_i = 2 degw_i I - (tr(C_i) I - C_i),  C_i = sym(Q_i); the adjugate over the determinant (numpy
        has no longdouble solver).  Rows of a singular D_i come out non-finite."""
        C = self.symQ()
        degw = np.zeros(self.N, dtype=LD)
        np.add.at(degw, self.ei, self.w)
        np.add.at(degw, self.ej, self.w)
        d = 2 * degw - (C[:, 0, 0] + C[:, 1, 1] + C[:, 2, 2])
        D = C + d[:, None, None] * np.eye(3, dtype=LD)
        x = np.asarray(v, dtype=LD).reshape(self.N, 3)
        det = (D[:, 0, 0] * (D[:, 1, 1] * D[:, 2, 2] - D[:, 1, 2] * D[:, 2, 1])
               - D[:, 0, 1] * (D[:, 1, 0] * D[:, 2, 2] - D[:, 1, 2] * D[:, 2, 0])
               + D[:, 0, 2] * (D[:, 1, 0] * D[:, 2, 1] - D[:, 1, 1] * D[:, 2, 0]))
        out = np.zeros((self.N, 3), dtype=LD)
        with np.errstate(invalid="ignore", divide="ignore"):
            for k in range(3):    # Cramer: column k of D replaced by x
                Dk = D.copy()
                Dk[:, :, k] = x
                dk = (Dk[:, 0, 0] * (Dk[:, 1, 1] * Dk[:, 2, 2] - Dk[:, 1, 2] * Dk[:, 2, 1])
                      - Dk[:, 0, 1] * (Dk[:, 1, 0] * Dk[:, 2, 2] - Dk[:, 1, 2] * Dk[:, 2, 0])
                      + Dk[:, 0, 2] * (Dk[:, 1, 0] * Dk[:, 2, 1] - Dk[:, 1, 1] * Dk[:, 2, 0]))
                out[:, k] = dk / det
        return out.ravel()

    def retract(self, xi):
        """Y_i = R_i exp(hat(xi_i))"""
        return (self.R @ exp_ld(xi)).ravel()


def so3_ref_f(c):
    return So3Ref(c).f()


def so3_ref_grad(c):
    return So3Ref(c).grad()


def so3_ref_hess(c, xi):
    return So3Ref(c).hess(xi)


def so3_ref_precon(c, v):
    return So3Ref(c).precon(v)


def so3_ref_retract(c, xi, R=None):
    return So3Ref(c, R).retract(xi)


def rel_err_ld(a, b):
    """conftest.rel_err with the difference taken in longdouble (b: the longdouble reference)"""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b * b).sum()), LD(1e-300)))


TOL_F = TOL_G = TOL_Y = 1e-13     # the bars of test_gpu_so3n.py::test_so3n_pieces_vs_oracle
TOL_H = TOL_P = 1e-12


def oracle_vs_reference(oracle, name):
    """{quantity: rel. distance of the fp64 oracle from the longdouble reference}: the floor of the device comparisons
    (the preconditioner on the rows of non-singular blocks).  Measures only; "precon_finite" is the oracle's finite mask,
    which test_cpu_so3n_reference.py holds against singular_nodes."""
    c = case(name)
    ref = reference_values(name)
    op = oracle.so3n(c.N, c.ei, c.ej, c.Rt, c.w, precon_kind=1)
    try:
        x = c.R.ravel()
        out = {}
        fo, fr = oracle.eval_f(op, x), ref["f"]
        out["f"] = float(abs(np.longdouble(fo) - fr) / abs(fr)) if fr != 0 else float(abs(fo))
        out["grad"] = rel_err_ld(oracle.eval_grad(op, x), ref["grad"])
        out["hess"] = max(rel_err_ld(oracle.eval_hess(op, x, xi), hr) for xi, hr in zip(ref["xis"], ref["hess"]))
        with np.errstate(all="ignore"):
            po = oracle.eval_precon(op, x, ref["v"])
        sing = np.repeat(singular_nodes(c), 3)
        out["precon"] = rel_err_ld(po[~sing], ref["precon"][~sing])
        out["precon_finite"] = np.isfinite(po)
        for m in SWEEP:
            out[f"retract_{m:.17g}"] = rel_err_ld(oracle.eval_retract(op, x, ref["sweep"][m]), ref["retract"][m])
        return out
    finally:
        oracle.free(op)


def bar_of(quantity):
    return {"f": TOL_F, "grad": TOL_G, "hess": TOL_H, "precon": TOL_P}.get(quantity, TOL_Y)


def probes(c, k=3, seed=1):
    """k tangent vectors for Hessian products and one for the preconditioner"""
    rng = np.random.Generator(np.random.PCG64(seed + 7))
    return [rng.normal(size=3 * c.N) for _ in range(k)], rng.normal(size=3 * c.N)


@functools.lru_cache(maxsize=None)
def reference_values(name):
    """the longdouble reference of every quantity the tests compare, once per case:
    dict(f, grad, hess [3], precon, retract {mag: Y}, and the inputs xis, v, sweep {mag: xi})"""
    c = case(name)
    ref = So3Ref(c)
    xis, v = probes(c)
    sweep = {m: sweep_xi(c, m, seed=k) for k, m in enumerate(SWEEP)}
    return dict(f=ref.f(), grad=ref.grad(), xis=xis, v=v, hess=[ref.hess(x) for x in xis], precon=ref.precon(v),
                sweep=sweep, retract={m: ref.retract(x) for m, x in sweep.items()})


def bit_contract_point(N=1500):
    """(Case, h): a point R and a step h whose retraction Y_i = R_i exp(hat h_i) lands on every branch of mat_to_quat and
    on its edges: R_i = I with h_i = angle x axis (half turns about the axes, the face and the body diagonal, 2 pi / 3
    about the body diagonal = the cyclic permutation, trace ~ 0, tied diagonals, and one ulp around each angle); R_i = a
    special rotation with a zero, tiny or half-turn step; generic rotations with steps of up to pi elsewhere."""
    ei, ej = wl.pose_graph(N, seed=29)[:2]
    axes = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1), (-1, 1, 1), (0.3, -0.5, 0.81),
            (0.9, 0.3, -0.1), (0.2, -0.95, 0.1), (0.1, 0.2, 0.97)]
    t23 = 2 * np.pi / 3
    angles = [np.pi, np.nextafter(np.pi, 0), np.nextafter(np.pi, 4), np.pi - 1e-8, t23, np.nextafter(t23, 0),
              np.nextafter(t23, 4), t23 - 2e-15, t23 + 2e-15, 2.5, 0.0, 2 * np.pi, 1e-4, 3.0]
    fixed, hs = {}, {}
    k = 0
    for ax in axes:
        n = np.asarray(ax, dtype=LD)
        n = n / np.sqrt((n * n).sum())
        for ang in angles:
            fixed[k], hs[k] = np.eye(3), (n * LD(ang)).astype(np.float64)
            k += 1
    rng = np.random.Generator(np.random.PCG64(37))
    for _, S in special_rotations():
        for step in (np.zeros(3), 1e-7 * rng.normal(size=3), np.array([np.pi, 0, 0]), np.array([0, 0, np.pi])):
            fixed[k], hs[k] = S, step
            k += 1
    assert k < N
    c = _build("bit_contract", N, ei, ej, 93, "linspace", fixed)
    u = rng.normal(size=(N, 3))
    h = u / np.linalg.norm(u, axis=1)[:, None] * rng.uniform(0, np.pi, size=(N, 1))
    for i, v in hs.items():
        h[i] = v
    return c, np.ascontiguousarray(h.ravel())
