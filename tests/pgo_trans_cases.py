"""Pose-graph translation problems and restatements (a helper module for test_cpu_pgo_trans_pack.py and
test_gpu_pgo_trans.py; not a conftest).

Graphs and points come from tests/so3_cases.py (imported, not edited): the smallest shapes that cross a slice (64), the
degree-sort window (1024), a hub beyond the window, empty slices and duplicate edges.  What is restated here shares no code
with optimization_amd/csrc/pgo_trans_pack.h or pgo_trans.hip:
  layout()      the host layout, in numpy, from the header comment of pgo_trans_pack.h
  rhs_ld() ...  the right-hand side, the residuals, the Laplacian product and the dense solve in np.longdouble
  pcg_f64()     a float64 Jacobi-PCG with the stopping rule of mi_pgo_trans_solve"""
import functools

import numpy as np

import so3_cases as sc

LD = np.longdouble
WINDOW = 1024
# the issue's name -> the graph and point of so3_cases (its weights are not used: tau is made here)
CASES = {"tiny_1": "tiny_1", "tiny_2": "tiny_2", "ring_chords_1023": "ring_chords_1023_ones",
         "ring_chords_1024": "ring_chords_1024_linspace", "ring_chords_1025": "ring_chords_1025_spread",
         "hub_first": "hub_first_linspace", "hub_last": "hub_last_spread", "isolated_1500": "isolated_1500",
         "multigraph_linspace": "multigraph_linspace", "path_300": "path_300"}
TAU_KINDS = ("linspace", "every_7th_zero")


def graph(name):
    c = sc.case(CASES[name])
    return c.N, c.ei.astype(np.int32), c.ej.astype(np.int32), c.R.reshape(c.N, 9)


def make_tau(E, kind):
    tau = np.linspace(0.5, 2.0, E)
    if kind == "every_7th_zero":
        tau[::7] = 0.0
    return tau


@functools.lru_cache(maxsize=None)
def problem(name, kind):
    """(N, ei, ej, tt (E, 3), tau, R (N, 9)): tt seeded normal"""
    N, ei, ej, R = graph(name)
    rng = np.random.Generator(np.random.PCG64(500 + len(name) + 7 * TAU_KINDS.index(kind)))
    return N, ei, ej, rng.normal(size=(ei.size, 3)), make_tau(ei.size, kind), R


def weighted_degree(N, ei, ej, tau):
    deg = np.zeros(N)
    np.add.at(deg, np.stack([ei, ej], axis=1).ravel(), np.repeat(tau, 2))   # (unbuffered: every node in edge order)
    return deg


def anchors(name, kind):
    """0, N - 1, the hub, a node of the ragged last slice, a zero-degree node (where the case has them)"""
    N, ei, ej, _, tau, _ = problem(name, kind)
    out = [0, N - 1]
    if name == "hub_first":
        out.append(0)
    if name == "hub_last":
        out.append(N - 1)
    if N % 64:
        out.append(N - 1 - (N % 64) // 2)
    zero = np.flatnonzero(weighted_degree(N, ei, ej, tau) == 0)
    if zero.size:
        out.append(int(zero[zero.size // 2]))
    return list(dict.fromkeys(out))


# ---- the layout, restated from the header comment of pgo_trans_pack.h ----
@functools.lru_cache(maxsize=None)
def slots(name):
    """the part of the layout that depends on the graph alone: dict(nslices, padded, slice_ptr, perm, nbr, word, owner, edge)
    with owner / edge = the node and the edge of every slot (-1: padding)"""
    N, ei, ej, _ = graph(name)
    inc = [[] for _ in range(N)]
    for e in range(ei.size):
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
    nbr, word = np.zeros(padded, dtype=np.int32), np.zeros(padded, dtype=np.uint32)
    owner, edge = np.full(padded, -1, dtype=np.int64), np.full(padded, -1, dtype=np.int64)
    for s in range(nslices):
        for lane in range(64):
            node = perm[64 * s + lane]
            base = slice_ptr[s] * 64 + lane
            nbr[base:base + 64 * width[s]:64] = node if node >= 0 else N - 1
            if node < 0:
                continue
            for k, (e, first, j) in enumerate(inc[node]):
                slot = base + 64 * k
                nbr[slot], word[slot], owner[slot], edge[slot] = j, (e << 1) | first, node, e
    return dict(nslices=nslices, padded=padded, slice_ptr=slice_ptr, perm=perm, nbr=nbr, word=word, owner=owner, edge=edge)


def laplacian_csr(N, ei, ej, tau, anchor):
    """(rowptr, col, val, dinv, unit): the anchored Laplacian, merged weights summed in edge order"""
    deg = weighted_degree(N, ei, ej, tau)
    unit = deg == 0
    unit[anchor] = True
    pair = {}
    for e in range(ei.size):
        key = (min(ei[e], ej[e]), max(ei[e], ej[e]))
        pair[key] = pair.get(key, 0.0) + tau[e]
    rows = [dict() for _ in range(N)]
    for (a, b), s in pair.items():
        if s != 0.0:
            rows[a][b] = -s
            rows[b][a] = -s
    rowptr, col, val = [0], [], []
    for i in range(N):
        ent = {} if unit[i] else {j: v for j, v in rows[i].items() if j != anchor}
        ent[i] = 1.0 if unit[i] else deg[i]
        for j in sorted(ent):
            col.append(j)
            val.append(ent[j])
        rowptr.append(len(col))
    dinv = np.repeat(np.where(unit, 1.0, 1.0 / np.where(unit, 1.0, deg)), 3)
    return (np.array(rowptr, dtype=np.int32), np.array(col, dtype=np.int32), np.array(val, dtype=np.float64), dinv, unit)


def layout(name, kind, anchor):
    N, ei, ej, tt, tau, _ = problem(name, kind)
    g = slots(name)
    E, padded = ei.size, g["padded"]
    rowptr, col, val, dinv, unit = laplacian_csr(N, ei, ej, tau, anchor)
    live = g["edge"] >= 0
    tauinc = np.zeros(max(1, padded))
    tinc = np.zeros(max(1, 3 * padded))
    sl = np.flatnonzero(live)
    tauinc[sl] = np.where(unit[g["owner"][sl]], 0.0, tau[g["edge"][sl]])
    k, lane = sl // 64, sl % 64
    for c in range(3):
        tinc[(k * 3 + c) * 64 + lane] = tt[g["edge"][sl], c]
    word = g["word"] if padded else np.zeros(1, dtype=np.uint32)
    return dict(N=N, E=E, nslices=g["nslices"], nnzb=2 * E, padded=padded, nnz=col.size, anchor=anchor,
                rowptr=rowptr, col=col, val=val, dinv=dinv, slice_ptr=g["slice_ptr"], perm=g["perm"], nbr=g["nbr"], slot=word,
                tinc=tinc, tauinc=tauinc, e_ij=np.stack([ei, ej], axis=1).ravel(), e_t=tt.T.ravel().copy(), e_tau=tau.copy())


# ---- the arithmetic, in longdouble (and in float64 where dtype says so) ----
def unit_rows(N, ei, ej, tau, anchor):
    unit = weighted_degree(N, ei, ej, tau) == 0
    unit[anchor] = True
    return unit


def rot_t(R, ei, tt, dtype=LD):
    """R_i tt_e per edge, (E, 3)"""
    return np.einsum("eab,eb->ea", R.reshape(-1, 3, 3).astype(dtype)[ei], tt.astype(dtype))


def rhs_ref(N, ei, ej, tt, tau, R, anchor, dtype=LD):
    v = tau.astype(dtype)[:, None] * rot_t(R, ei, tt, dtype)
    b = np.zeros((N, 3), dtype=dtype)
    np.add.at(b, ej, v)
    np.add.at(b, ei, -v)
    b[unit_rows(N, ei, ej, tau, anchor)] = 0
    return b.ravel()


def residual_ref(N, ei, ej, tt, tau, R, t, dtype=LD):
    """(r (3E), f_tau, max_e |r_e|)"""
    t = np.asarray(t).reshape(N, 3).astype(dtype)
    r = t[ej] - t[ei] - rot_t(R, ei, tt, dtype)
    rr = (r * r).sum(axis=1)
    return r.ravel(), (tau.astype(dtype) * rr).sum() / 2, np.sqrt(rr.max(initial=dtype(0)))


def laplacian_apply_ref(N, ei, ej, tau, anchor, X, dtype=LD):
    """L_a X for an N x 3 field, edge by edge (no assembled matrix)"""
    X = np.asarray(X).reshape(N, 3).astype(dtype)
    unit = unit_rows(N, ei, ej, tau, anchor)
    Xa = X.copy()
    Xa[anchor] = 0            # the anchor's column is removed
    d = tau.astype(dtype)[:, None] * (Xa[ej] - Xa[ei])
    out = np.zeros((N, 3), dtype=dtype)
    np.add.at(out, ej, d)
    np.add.at(out, ei, -d)
    out[unit] = X[unit]
    return out.ravel()


def dense_laplacian(N, ei, ej, tau, anchor):
    rowptr, col, val, _, _ = laplacian_csr(N, ei, ej, tau, anchor)
    A = np.zeros((N, N))
    A[np.repeat(np.arange(N), np.diff(rowptr)), col] = val
    return A


def floating_components(N, ei, ej, tau, anchor):
    """the components that carry weight but not the anchor, as index arrays: on them L_a is singular (outside the method;
    every_7th_zero cuts path_300 into such pieces)"""
    lab = np.arange(N)
    a, b = ei[tau > 0].astype(np.int64), ej[tau > 0].astype(np.int64)
    while True:
        new = lab.copy()
        np.minimum.at(new, a, lab[b])
        np.minimum.at(new, b, lab[a])
        new = new[new]
        if np.array_equal(new, lab):
            break
        lab = new
    return [np.flatnonzero(lab == c) for c in np.unique(lab) if c != lab[anchor] and np.count_nonzero(lab == c) > 1]


def dense_solve_refined(N, ei, ej, tau, anchor, b, rounds=3):
    """L_a t = b by the dense float64 factorisation, refined with longdouble residuals: (t in longdouble, (N, 3)).
    Where tau leaves components that do not hold the anchor, L_a is singular and the system consistent: the dense
    least-squares solution is refined instead, and on every such component the solution is the one Jacobi-PCG from t = 0
    converges to -- the one whose degree-weighted mean over the component is zero (the iterates stay D-orthogonal to the
    null vectors, D = diag L_a)."""
    A = dense_laplacian(N, ei, ej, tau, anchor)
    b = np.asarray(b, dtype=LD).reshape(N, 3)
    floating = floating_components(N, ei, ej, tau, anchor)
    if floating:
        def solve(rhs):
            return np.linalg.lstsq(A, rhs, rcond=None)[0]
    else:
        def solve(rhs):
            return np.linalg.solve(A, rhs)
    t = solve(b.astype(np.float64)).astype(LD)
    for _ in range(rounds):
        r = b - laplacian_apply_ref(N, ei, ej, tau, anchor, t).reshape(N, 3)
        t = t + solve(r.astype(np.float64)).astype(LD)
    deg = weighted_degree(N, ei, ej, tau).astype(LD)
    for idx in floating:
        t[idx] -= (deg[idx, None] * t[idx]).sum(axis=0) / deg[idx].sum()
    return t


def pcg_f64(A, dinv, b, tol, max_iterations):
    """Jacobi-PCG in float64 from t = 0 on the dense matrix, stop at sqrt(<r,v>) <= tol sqrt(<r0,v0>): (t, iterations)"""
    b = b.reshape(-1, 3)
    d = dinv.reshape(-1, 3)
    t = np.zeros_like(b)
    r = -b
    v = d * r
    rv = float((r * v).sum())
    target = tol * np.sqrt(rv)
    p = -v
    k = 0
    while k < max_iterations and not np.sqrt(rv) <= target:
        Hp = A @ p
        alpha = rv / float((p * Hp).sum())
        t += alpha * p
        r += alpha * Hp
        v = d * r
        rv_new = float((r * v).sum())
        p = -v + (rv_new / rv) * p
        rv = rv_new
        k += 1
    return t, k


def rel_ld(a, ref):
    a, ref = np.asarray(a, dtype=LD).ravel(), np.asarray(ref, dtype=LD).ravel()
    return float(np.sqrt(((a - ref) ** 2).sum()) / max(np.sqrt((ref * ref).sum()), LD(1e-300)))
