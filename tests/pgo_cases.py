"""Joint pose-graph problems on SE(3)^N and their restatements (a helper module for test_cpu_pgo_pack.py,
test_cpu_pgo_fd.py, test_gpu_pgo.py and test_gpu_pgo_tnt.py; not a conftest).

    f(R, t) = 1/2 sum_e kappa_e |R_j - R_i Rt_e|_F^2 + 1/2 sum_e tau_e |t_j - t_i - R_i tt_e|^2,   e = (i -> j)

Point: 12N doubles [R | t]; tangent: 6N doubles, node-major [xi_i, delta_i].  What is restated here shares no code with
optimization_amd/csrc/pgo_pack.h or pgo.hip:
  layout()     the host layout, in numpy, from the header comment of pgo_pack.h
  PgoRef       f, the gradient, H eta, the retraction and the written blocks in np.longdouble.  The rotation term is the
               reference of tests/so3_cases.py (So3Ref: edge-loop objective, connection Laplacian, operator-form Hessian); the
               translation term is written EDGE BY EDGE from the quadratic form
                   tau ( |delta_j - delta_i + A xi_i|^2 + xi_i' [(u.tt) I - 1/2 (u tt' + tt u')] xi_i ),
               not from the node blocks the kernel assembles.  test_cpu_pgo_fd.py holds it against central differences."""
import functools

import numpy as np

import so3_cases as sc
from optimization_amd import workloads as wl

LD = np.longdouble
WINDOW = 1024


# ---- graphs ----
def _ring_chords(N, seed):
    ei, ej = wl.pose_graph(N, seed=seed)[:2]
    return ei.astype(np.int64), ej.astype(np.int64)


def _hub(N, at_end):
    """one node joined to every other node: out of the hub to the even nodes, into it from the odd ones, plus a path"""
    h = N - 1 if at_end else 0
    others = np.array([i for i in range(N) if i != h])
    a = np.where(others % 2 == 0, h, others)
    b = np.where(others % 2 == 0, others, h)
    return np.concatenate([a, others[:-1]]), np.concatenate([b, others[1:]])


def _fd12():
    """12 nodes: a ring forwards, chords backwards, a two-way pair (2 -> 7, 7 -> 2) and a doubled edge"""
    ring = np.arange(12)
    ei = np.concatenate([ring, [9, 11, 6, 2, 7, 4, 4]])
    ej = np.concatenate([(ring + 1) % 12, [3, 5, 0, 7, 2, 10, 10]])
    return ei, ej


def _isolated(N):
    """nodes 0 and N - 1 without an edge"""
    ei, ej = _ring_chords(N - 2, seed=5)
    return ei + 1, ej + 1


def _multigraph(N):
    ei, ej = _ring_chords(N, seed=9)
    return np.concatenate([ei, ei[::5], ej[::7]]), np.concatenate([ej, ej[::5], ei[::7]])


_GRAPHS = {
    "n1": lambda: (1, np.zeros(0, np.int64), np.zeros(0, np.int64)),
    "n2": lambda: (2, np.array([0, 1]), np.array([1, 0])),
    "fd12": lambda: (12,) + _fd12(),
    "hub10": lambda: (10,) + _hub(10, False),
    "ring65": lambda: (65,) + _ring_chords(65, seed=65),
    "ring300": lambda: (300,) + _ring_chords(300, seed=300),
    "hub_first200": lambda: (200,) + _hub(200, False),
    "hub_last200": lambda: (200,) + _hub(200, True),
    # beyond the 1024-node window of the degree sort: the hub (degree N - 1) heads the LAST window, so the widest slice is
    # slice 16 of 24, not the first
    "hub_last1500": lambda: (1500,) + _hub(1500, True),
    "isolated70": lambda: (70,) + _isolated(70),
    "multigraph130": lambda: (130,) + _multigraph(130),
}
# weight patterns: (kappa kind, tau kind)
_WEIGHTS = {
    "": ("linspace", "linspace"),
    "_tau7": ("linspace", "every_7th_zero"),       # tau = 0 on single edges
    "_taunode": ("linspace", "node_zero"),        # tau = 0 on every edge of node 5
    "_kappa0": ("zero", "linspace"),              # the pure translation term
    "_tau0": ("linspace", "zero"),                # must reproduce rotation averaging
}
FD_CASES = ("fd12", "hub10")
GPU_CASES = ("n1", "n2", "ring65", "ring300", "hub_first200", "hub_last200", "hub_last1500", "isolated70", "multigraph130",
             "ring300_tau7", "ring65_taunode", "ring65_kappa0", "ring300_tau0", "multigraph130_tau0")


def _weights(kind, ei, ej, lo, hi):
    E = ei.size
    w = np.linspace(lo, hi, E)
    if kind == "zero":
        w[:] = 0.0
    elif kind == "every_7th_zero":
        w[::7] = 0.0
    elif kind == "node_zero":
        w[(ei == 5) | (ej == 5)] = 0.0
    return w


@functools.lru_cache(maxsize=None)
def problem(name):
    """dict(N, ei, ej, Rt (E, 9), tt (E, 3), kappa, tau, x (12N)): measurements = the truth's relative poses with noise
    (0.05 rad, 0.05 length), the point = the truth moved by 0.2 rad and 0.5 length units: |r_e| of order one"""
    base, suffix = name, ""
    for s in sorted(_WEIGHTS, key=len, reverse=True):
        if s and name.endswith(s):
            base, suffix = name[:-len(s)], s
            break
    N, ei, ej = _GRAPHS[base]()
    ei, ej = np.asarray(ei, dtype=np.int64), np.asarray(ej, dtype=np.int64)
    E = ei.size
    rng = np.random.Generator(np.random.PCG64(7000 + sum(map(ord, base))))
    Rtrue = sc.round_orth(sc.exp_ld(rng.normal(size=(N, 3)) * 1.5)).astype(LD)
    ttrue = (rng.normal(size=(N, 3)) * 2.0).astype(LD)
    noise = sc.exp_ld(rng.normal(size=(E, 3)) * 0.05)
    RiT = np.swapaxes(Rtrue[ei], 1, 2)
    Rt = sc.round_orth(RiT @ Rtrue[ej] @ noise) if E else np.zeros((0, 3, 3))
    tt = (np.einsum("eab,eb->ea", RiT, ttrue[ej] - ttrue[ei]) + rng.normal(size=(E, 3)) * 0.05).astype(np.float64)
    R = sc.round_orth(Rtrue @ sc.exp_ld(rng.normal(size=(N, 3)) * 0.2))
    t = (ttrue + rng.normal(size=(N, 3)) * 0.5).astype(np.float64)
    kk, tk = _WEIGHTS[suffix]
    return dict(name=name, N=N, ei=ei.astype(np.int32), ej=ej.astype(np.int32), Rt=np.ascontiguousarray(Rt.reshape(E, 9)),
                tt=np.ascontiguousarray(tt.reshape(E, 3)), kappa=_weights(kk, ei, ej, 0.5, 1.5), tau=_weights(tk, ei, ej, 0.25, 2.0),
                x=np.concatenate([R.ravel(), t.ravel()]))


def probes(p, k=2, seed=3):
    """k tangent vectors (6N), steps of 0.3 rad / 0.3 length units"""
    rng = np.random.Generator(np.random.PCG64(seed + 11 * p["N"]))
    return [0.3 * rng.normal(size=6 * p["N"]) for _ in range(k)]


# ---- the layout, restated from the header comments of pgo_pack.h and so3_pack.h ----
def layout(p):
    N, ei, ej = p["N"], p["ei"], p["ej"]
    E = ei.size
    inc = [[] for _ in range(N)]
    for e in range(E):
        inc[ej[e]].append((e, 0, int(ei[e])))
        inc[ei[e]].append((e, 1, int(ej[e])))
    deg = np.array([len(l) for l in inc], dtype=np.int64)
    nslices = (N + 63) // 64
    perm = np.full(nslices * 64, -1, dtype=np.int32)
    for w0 in range(0, N, WINDOW):
        w1 = min(N, w0 + WINDOW)
        perm[w0:w1] = w0 + np.argsort(-deg[w0:w1], kind="stable")
    width = [max([deg[i] for i in perm[64 * s:64 * s + 64] if i >= 0], default=0) for s in range(nslices)]
    slice_ptr = np.concatenate([[0], np.cumsum(width)]).astype(np.int64)
    padded = 64 * int(slice_ptr[-1])
    nbr, word = np.zeros(padded, dtype=np.int32), np.zeros(max(1, padded), dtype=np.uint32)
    rinc, tinc = np.zeros(max(1, 9 * padded)), np.zeros(max(1, 3 * padded))
    kinc, tauinc = np.zeros(max(1, padded)), np.zeros(max(1, padded))
    owner, edge = np.full(padded, -1, dtype=np.int64), np.full(padded, -1, dtype=np.int64)
    Rt = p["Rt"].reshape(E, 3, 3)
    for s in range(nslices):
        for lane in range(64):
            node = perm[64 * s + lane]
            for k in range(width[s]):
                nbr[(slice_ptr[s] + k) * 64 + lane] = node if node >= 0 else N - 1
            if node < 0:
                continue
            for k, (e, first, j) in enumerate(inc[node]):
                kk = int(slice_ptr[s]) + k
                slot = kk * 64 + lane
                nbr[slot], word[slot], owner[slot], edge[slot] = j, (e << 1) | first, node, e
                S = Rt[e].T if first else Rt[e]
                rinc[(kk * 9 + np.arange(9)) * 64 + lane] = S.ravel()
                tinc[(kk * 3 + np.arange(3)) * 64 + lane] = p["tt"][e]
                kinc[slot], tauinc[slot] = p["kappa"][e], p["tau"][e]
    return dict(N=N, E=E, nslices=nslices, nnzb=2 * E, padded=padded, slice_ptr=slice_ptr, perm=perm, nbr=nbr, slot=word,
                rinc=rinc, tinc=tinc, kinc=kinc, tauinc=tauinc, owner=owner, edge=edge)


# ---- the arithmetic ----
def cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def right_jacobian(xi):
    """J_r(xi) with exp(hat(xi + d)) = exp(hat xi) exp(hat(J_r d)) + o(d): I - (1 - cos t)/t^2 K + (t - sin t)/t^3 K^2"""
    xi = np.asarray(xi, dtype=LD).reshape(-1, 3)
    th = np.sqrt((xi * xi).sum(axis=1))
    safe = np.where(th > 0, th, LD(1))
    sh = np.sin(safe / 2) / safe
    b = np.where(th > 0, 2 * sh * sh, LD(1) / 2)
    # (t - sin t) / t^3 by its series below 1e-2 (cancellation), else directly
    t2 = safe * safe
    ser = LD(1) / 6 - t2 / 120 + t2 * t2 / 5040 - t2 * t2 * t2 / 362880
    c = np.where(th > LD(1e-2), (safe - np.sin(safe)) / (safe * t2), np.where(th > 0, ser, LD(1) / 6))
    K = sc.hat_ld(xi)
    return np.eye(3, dtype=LD) - b[:, None, None] * K + c[:, None, None] * (K @ K)


class PgoRef:
    """the reference at the point x (default: the problem's), dtype longdouble (or float64: the restatement's own distance)"""

    def __init__(self, p, x=None, dtype=LD):
        self.p, self.N, self.dt = p, p["N"], dtype
        N = self.N
        x = np.asarray(p["x"] if x is None else x)
        self.R = x[:9 * N].astype(dtype).reshape(N, 3, 3)
        self.t = x[9 * N:].astype(dtype).reshape(N, 3)
        self.ei, self.ej = p["ei"].astype(np.int64), p["ej"].astype(np.int64)
        self.tt, self.tau, self.kappa = p["tt"].astype(dtype), p["tau"].astype(dtype), p["kappa"].astype(dtype)
        # (So3Ref is longdouble throughout: with dtype float64 only the translation term is evaluated in float64)
        self.rot = sc.So3Ref(sc.Case(p["name"], N, p["ei"], p["ej"], p["Rt"], p["kappa"], None), R=self.R.astype(LD))
        Ri = self.R[self.ei]
        self.r = self.t[self.ej] - self.t[self.ei] - np.einsum("eab,eb->ea", Ri, self.tt)
        self.u = np.einsum("eba,eb->ea", Ri, self.r)

    def f(self):
        return self.rot.f() + (self.tau * (self.r * self.r).sum(axis=1)).sum() / 2

    def grad(self):
        g = np.zeros((self.N, 6), dtype=self.dt)
        g[:, :3] = self.rot.grad().reshape(self.N, 3)
        tr = self.tau[:, None] * self.r
        np.add.at(g[:, :3], self.ei, -self.tau[:, None] * cross(self.tt, self.u))
        np.add.at(g[:, 3:], self.ei, -tr)
        np.add.at(g[:, 3:], self.ej, tr)
        return g.ravel()

    def hess(self, eta):
        eta = np.asarray(eta).astype(self.dt).reshape(self.N, 6)
        xi, de = eta[:, :3], eta[:, 3:]
        h = np.zeros((self.N, 6), dtype=self.dt)
        h[:, :3] = self.rot.hess(xi.astype(LD)).reshape(self.N, 3)
        A = self.R[self.ei] @ sc.hat_ld(self.tt).astype(self.dt)                      # A_e = R_i hat(tt_e)
        w = de[self.ej] - de[self.ei] + np.einsum("eab,eb->ea", A, xi[self.ei])
        ut = (self.u * self.tt).sum(axis=1)
        xe = xi[self.ei]
        Mx = ut[:, None] * xe - ((self.tt * xe).sum(axis=1)[:, None] * self.u + (self.u * xe).sum(axis=1)[:, None] * self.tt) / 2
        tau = self.tau[:, None]
        np.add.at(h[:, 3:], self.ej, tau * w)
        np.add.at(h[:, 3:], self.ei, -tau * w)
        np.add.at(h[:, :3], self.ei, tau * (np.einsum("eba,eb->ea", A, w) + Mx))
        return h.ravel()

    def retract(self, eta):
        eta = np.asarray(eta).astype(LD).reshape(self.N, 6)
        Y = self.R.astype(LD) @ sc.exp_ld(eta[:, :3])
        return np.concatenate([Y.ravel(), (self.t.astype(LD) + eta[:, 3:]).ravel()])

    def blocks(self, lay):
        """(Bblk, Gblk, Nsl, Minv, acted): what mi_pgo_model writes, in its layouts; acted[2 i + b] = block b of node i has no
        inverse (the identity is written there)"""
        N, E, padded, nslices = self.N, self.ei.size, lay["padded"], lay["nslices"]
        Rt = self.p["Rt"].astype(LD).reshape(E, 3, 3)
        B, G = np.zeros(max(1, 9 * padded), dtype=LD), np.zeros(max(1, 9 * padded), dtype=LD)
        eye = np.eye(3, dtype=LD)
        hat_tt = sc.hat_ld(self.tt)
        for slot in np.flatnonzero(lay["edge"] >= 0):
            e, first = int(lay["edge"][slot]), int(lay["slot"][slot] & 1)
            i, j = int(lay["owner"][slot]), int(lay["nbr"][slot])
            k, lane = slot // 64, slot % 64
            S = Rt[e].T if first else Rt[e]
            Q = self.R[i].T @ self.R[j]
            Bk = np.stack([sc.vee2_ld((Q @ sc.hat_ld(eye[m])[0] @ S)[None])[0] for m in range(3)], axis=1) * self.kappa[e]
            A = self.tau[e] * (self.R[i if first else j] @ hat_tt[e])
            B[(k * 9 + np.arange(9)) * 64 + lane] = Bk.ravel()
            G[(k * 9 + np.arange(9)) * 64 + lane] = (A.T if first else A).ravel()
        C = self.rot.symQ()
        degk, degt = np.zeros(N, dtype=LD), np.zeros(N, dtype=LD)
        for arr, w in ((degk, self.kappa), (degt, self.tau)):
            np.add.at(arr, self.ei, w)
            np.add.at(arr, self.ej, w)
        H = C + (2 * degk - np.trace(C, axis1=1, axis2=2))[:, None, None] * eye
        ut = (self.u * self.tt).sum(axis=1)
        tt2 = (self.tt * self.tt).sum(axis=1)
        T = self.tau[:, None, None] * ((tt2 + ut)[:, None, None] * eye - self.tt[:, :, None] * self.tt[:, None, :]
                                       - (self.u[:, :, None] * self.tt[:, None, :] + self.tt[:, :, None] * self.u[:, None, :]) / 2)
        np.add.at(H, self.ei, T)
        stt = np.zeros((N, 3), dtype=LD)
        np.add.at(stt, self.ei, self.tau[:, None] * self.tt)
        K = self.R @ sc.hat_ld(stt)
        Nsl = np.zeros(nslices * 19 * 64, dtype=LD)
        Minv = np.zeros((N, 2, 3, 3), dtype=LD)
        acted = np.zeros(2 * N, dtype=bool)
        for l, node in enumerate(lay["perm"]):
            if node < 0:
                continue
            s, lane = l // 64, l % 64
            Nsl[(s * 19 + np.arange(9)) * 64 + lane] = H[node].ravel()
            Nsl[(s * 19 + 9 + np.arange(9)) * 64 + lane] = K[node].ravel()
            Nsl[(s * 19 + 18) * 64 + lane] = degt[node]
            if _cofactor_det64(H[node]) == 0:    # (the kernel's rule: the float64 cofactor determinant is exactly 0)
                Minv[node, 0], acted[2 * node] = eye, True
            else:
                Minv[node, 0] = _inv3(H[node])
            if degt[node] == 0:
                Minv[node, 1], acted[2 * node + 1] = eye, True
            else:
                Minv[node, 1] = eye / degt[node]
        return B, G, Nsl, Minv.ravel(), acted


def _cofactor_det64(D):
    """a c00 + b c01 + c c02 of the symmetric block's upper triangle, every operation rounded to float64"""
    a, b, c, e, f, g = (np.float64(D[i, j]) for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)))
    return a * (e * g - f * f) + b * (c * f - b * g) + c * (b * f - c * e)


def _inv3(D):
    c = np.array([[D[1, 1] * D[2, 2] - D[1, 2] * D[2, 1], D[0, 2] * D[2, 1] - D[0, 1] * D[2, 2], D[0, 1] * D[1, 2] - D[0, 2] * D[1, 1]],
                  [D[1, 2] * D[2, 0] - D[1, 0] * D[2, 2], D[0, 0] * D[2, 2] - D[0, 2] * D[2, 0], D[0, 2] * D[1, 0] - D[0, 0] * D[1, 2]],
                  [D[1, 0] * D[2, 1] - D[1, 1] * D[2, 0], D[0, 1] * D[2, 0] - D[0, 0] * D[2, 1], D[0, 0] * D[1, 1] - D[0, 1] * D[1, 0]]],
                 dtype=LD)
    return c / (D[0, 0] * c[0, 0] + D[0, 1] * c[1, 0] + D[0, 2] * c[2, 0])


def pullback_grad(p, x, eta, s):
    """the gradient of  v -> f(x (+) (s eta + v))  at v = 0, in longdouble: J_r(s xi)' g_xi(x (+) s eta), g_delta unchanged"""
    N = p["N"]
    se = LD(s) * np.asarray(eta, dtype=LD)
    y = PgoRef(p).retract(se) if x is None else PgoRef(p, x).retract(se)
    g = PgoRef(p, y).grad().reshape(N, 6)
    J = right_jacobian(se.reshape(N, 6)[:, :3])
    out = g.copy()
    out[:, :3] = np.einsum("nba,nb->na", J, g[:, :3])
    return out.ravel()


def rel_ld(a, ref):
    a, ref = np.asarray(a, dtype=LD).ravel(), np.asarray(ref, dtype=LD).ravel()
    return float(np.sqrt(((a - ref) ** 2).sum()) / max(np.sqrt((ref * ref).sum()), LD(1e-300)))


@functools.lru_cache(maxsize=None)
def reference_values(name):
    """the longdouble reference of every quantity test_gpu_pgo.py compares, once per case, and the float64 restatement's own
    distance from it (`floor`): dict(f, grad, etas, hess, retract, lay, blocks, floor)"""
    p = problem(name)
    ref, r64 = PgoRef(p), PgoRef(p, dtype=np.float64)
    etas = probes(p)
    lay = layout(p)
    out = dict(f=ref.f(), grad=ref.grad(), etas=etas, hess=[ref.hess(e) for e in etas], retract=ref.retract(etas[0]), lay=lay,
               blocks=ref.blocks(lay))
    f64 = r64.f()
    out["floor"] = dict(f=float(abs(LD(f64) - out["f"]) / abs(out["f"])) if out["f"] != 0 else 0.0,
                        grad=rel_ld(r64.grad(), out["grad"]),
                        hess=max(rel_ld(r64.hess(e), h) for e, h in zip(etas, out["hess"])))
    return out
