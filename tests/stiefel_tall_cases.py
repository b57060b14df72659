"""The tall-row Stiefel family (optimization_amd/csrc/stiefel_tall.hip, St(n, p) for p = 9 ... 16) restated in
np.longdouble, and the named problems its parity tests run (a helper module for test_cpu_stiefel_tall_reference.py and
test_gpu_stiefel_tall_parity.py; not a conftest).

Nothing here shares code with the kernels, the oracle or optimization_amd.workloads.  Every number used as a bar comes
out of numpy's own loops on longdouble arrays (numpy has no BLAS or LAPACK path for that type):
  spmm()        the sparse product summed entry by entry in storage order
  TallRef       Gram X'Z, projection Z - X sym(X'Z), objective 1/2 tr(X'AX), gradient AX - X sym(X'AX), Hessian
                P_X(A V - V S), preconditioner P_X(D^-1 r), the three curvature dots, the retraction
  polar()       the polar factor of Y through a one-sided (Hestenes) Jacobi SVD of its p x p factor R (Y = Q R by
                Gram-Schmidt in longdouble), swept until no pair rotates.  Not an
                inverse square root of Y'Y: that squares the condition number before the first operation, and a plain
                Newton iteration for G^-1/2 in longdouble was unstable from cond(G) = 1e2 on
  gram_floor()  how far Y G64^-1/2 lies from the polar factor when G64 is Y'Y formed exactly and rounded once to
                float64: what any method that passes through a float64 Gram pays
  newton_schulz64()  the kernel's own method (tall_invsqrt_wave: Newton-Schulz and one corrective step) re-enacted in
                float64: a restatement of the method for diagnosis, never a bar
  stpcg()       Steihaug-Toint CG without a preconditioner in any numpy precision"""
import functools
import re

import numpy as np

LD = np.longdouble
EPS_LD = np.finfo(LD).eps
TALL_P = (9, 12, 13, 16)
RAGGED_N = (16, 17, 63, 64, 65, 241, 255, 256, 257, 1025)    # and n = p; 241 = 15 * 16 + 1: a last tile of one row
STRIDE_N = (1025, 600)
LARGE_N = 66000                                               # 258 workgroup steps of 256 rows: 255 workgroups, a partial second stride
PROLOGUE_COUNTS = (1, 7, 8, 9, 17)                            # Gram rows summed: below, at and past the 8-way unrolled body
HARD_P, HARD_N, HARD_COND = (9, 16), (0, 17, 300), (2, 4, 6)  # n = 0 stands for n = p; cond(Y'Y) ~ 1e2, 1e4, 1e6
# the smallest symmetric matrix that can hold more than 256 distinct values (one of the 256 table entries of the packed
# copy may be the padding zero): n (n + 1) / 2 > 255
MIN_N_UNPACKABLE = 23


# ---- matrices ----
def _csr_from_pairs(n, pi, pj, w):
    """CSR (int32 rowptr, int32 col, float64 val) of the symmetric matrix with w on (i, j) and (j, i), columns ascending"""
    pi, pj, w = np.asarray(pi, np.int64), np.asarray(pj, np.int64), np.asarray(w, np.float64)
    off = pi != pj
    rows = np.concatenate([pi, pj[off]])
    cols = np.concatenate([pj, pi[off]])
    vals = np.concatenate([w, w[off]])
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    rowptr = np.zeros(n + 1, np.int64)
    np.add.at(rowptr, rows + 1, 1)
    return np.cumsum(rowptr).astype(np.int32), cols.astype(np.int32), vals


@functools.lru_cache(maxsize=None)
def ragged_pattern(n):
    """unordered pairs (i <= j) of a ragged pattern and its transpose: 1 ... 16 random columns a row, every 5th row and
    column empty"""
    rng = np.random.Generator(np.random.PCG64(4100 + n))
    pairs = set()
    for i in range(n):
        k = int(rng.integers(1, 17))
        cols = np.unique(rng.integers(0, n, size=k))
        if i % 5 == 0:
            continue
        pairs.update((min(i, int(c)), max(i, int(c))) for c in cols if c % 5 != 0)
    pairs = sorted(pairs)
    return np.array([a for a, _ in pairs], np.int64), np.array([b for _, b in pairs], np.int64)


@functools.lru_cache(maxsize=None)
def matrix(n, form):
    """(rowptr, col, val), exactly symmetric.  form "general": normal weights (distinct with probability one: a matrix
    with more than 255 of them has no value-indexed packed copy); "few": weights from {-1, 0.5, 2} (always packed);
    "banded": offsets 0, 1, 2, 7 with normal weights and a dominant diagonal (the large case)"""
    rng = np.random.Generator(np.random.PCG64(77 + 3 * n + len(form)))
    if form == "banded":
        pi, pj, w = [np.arange(n)], [np.arange(n)], [4.0 + rng.random(n)]
        for d in (1, 2, 7):
            pi.append(np.arange(n - d))
            pj.append(np.arange(n - d) + d)
            w.append(rng.normal(size=n - d))
        return _csr_from_pairs(n, np.concatenate(pi), np.concatenate(pj), np.concatenate(w))
    pi, pj = ragged_pattern(n)
    w = rng.normal(size=pi.size) if form == "general" else rng.choice(np.array([-1.0, 0.5, 2.0]), size=pi.size)
    return _csr_from_pairs(n, pi, pj, w)


def distinct_values(val):
    """distinct bit patterns among the stored values and the zero that pads a slice: what the packed copy has to index"""
    return np.unique(np.concatenate([np.asarray(val, np.float64), [0.0]]).view(np.uint64)).size


def expect_packed(val):
    return distinct_values(val) <= 256


# ---- the arithmetic ----
def spmm(rowptr, col, val, V, absolute=False):
    """A V, every row summed entry by entry in storage order (absolute: sum |a| |v|, the scale of that sum)"""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    val, V = np.asarray(val).astype(LD), np.asarray(V).astype(LD)
    if absolute:
        val, V = np.abs(val), np.abs(V)
    W = np.zeros((rowptr.size - 1, V.shape[1]), dtype=LD)
    count = np.diff(rowptr)
    for k in range(int(count.max(initial=0))):
        rows = np.flatnonzero(count > k)
        e = rowptr[rows] + k
        W[rows] = W[rows] + val[e][:, None] * V[col[e]]
    return W


def sym(M):
    return (M + M.T) / 2


def orthonormalise(M):
    """modified Gram-Schmidt, twice, in longdouble"""
    Qt = np.array(np.asarray(M).T, dtype=LD)      # columns as contiguous rows
    for _ in range(2):
        for j in range(Qt.shape[0]):
            for i in range(j):
                Qt[j] = Qt[j] - (Qt[i] * Qt[j]).sum() * Qt[i]
            Qt[j] = Qt[j] / np.sqrt((Qt[j] * Qt[j]).sum())
    return np.ascontiguousarray(Qt.T)


def jacobi_svd(Y, max_sweeps=80):
    """one-sided (Hestenes) Jacobi: Y = W diag(s) V' with W'W = I, V orthogonal; rotations until every pair of columns
    has |cos| <= 16 eps (numpy's sums over a column are pairwise: their own rounding stays below that)"""
    Wt = np.array(np.asarray(Y).T, dtype=LD)      # columns as contiguous rows
    p = Wt.shape[0]
    Vt = np.eye(p, dtype=LD)
    tol = 16 * EPS_LD
    for _ in range(max_sweeps):
        rotated = False
        for i in range(p - 1):
            for j in range(i + 1, p):
                a, b = Wt[i], Wt[j]
                aa, bb, ab = (a * a).sum(), (b * b).sum(), (a * b).sum()
                if abs(ab) <= tol * np.sqrt(aa * bb):
                    continue
                rotated = True
                zeta = (bb - aa) / (2 * ab)
                t = (LD(1) if zeta >= 0 else LD(-1)) / (abs(zeta) + np.sqrt(1 + zeta * zeta))
                c = 1 / np.sqrt(1 + t * t)
                s = c * t
                Wt[i], Wt[j] = c * a - s * b, s * a + c * b
                va, vb = Vt[i].copy(), Vt[j].copy()
                Vt[i], Vt[j] = c * va - s * vb, s * va + c * vb
        if not rotated:
            break
    else:
        raise RuntimeError("the Jacobi sweeps did not settle")
    s = np.sqrt((Wt * Wt).sum(axis=1))
    return (Wt / s[:, None]).T, s, Vt.T


def polar(Y):
    """(U, s): the polar factor of Y and its singular values.  Y = Q R with Q orthonormal (Gram-Schmidt above) and
    R = Q'Y square, R = W diag(s) V' by Jacobi: U = Q W V'.  The sweeps then run on p rows, not n"""
    Y = np.asarray(Y).astype(LD)
    Q = orthonormalise(Y)
    W, s, V = jacobi_svd(Q.T @ Y)
    return Q @ (W @ V.T), s


def invsqrt_spd(G):
    """G^-1/2 of a symmetric positive definite G through its Jacobi decomposition G = V diag(s) V'"""
    _, s, V = jacobi_svd(G)
    return sym((V / np.sqrt(s)) @ V.T)


def gram_floor(Y, U=None):
    """max |U - Y G64^-1/2| / max |U|: G64 = Y'Y in longdouble rounded once to float64, its inverse square root by Jacobi"""
    Y = np.asarray(Y).astype(LD)
    U = polar(Y)[0] if U is None else U
    G64 = sym(Y.T @ Y).astype(np.float64).astype(LD)
    return float(np.abs(U - Y @ invsqrt_spd(G64)).max() / np.abs(U).max())


def newton_schulz64(G, stop=1e-26, max_iterations=100, correct=True):
    """tall_invsqrt_wave in float64: Y0 = G / |G|_F, Z0 = I; T = Z Y; Y <- Y (3 I - T) / 2, Z <- (3 I - T) Z / 2; one more
    step after |T - I|_F^2 <= stop; then (correct) the kernel's corrective step M <- M + M (I - M G M) / 2 with the
    residual formed in longdouble (the kernel forms it in double-double).  Returns (G^-1/2, iterations taken)"""
    G = np.asarray(G, dtype=np.float64)
    p = G.shape[0]
    sc = np.sqrt((G * G).sum())
    Y, Z, I = G / sc, np.eye(p), np.eye(p)
    last, steps = False, 0
    for _ in range(max_iterations):
        T = Z @ Y
        err = ((T - I) ** 2).sum()
        Y, Z = 0.5 * (Y @ (3 * I - T)), 0.5 * ((3 * I - T) @ Z)
        steps += 1
        if last:
            break
        if not err > stop:
            last = True
    M = Z / np.sqrt(sc)
    if correct:
        Ml = M.astype(LD)
        M = M + 0.5 * (M @ (np.eye(p, dtype=LD) - Ml @ G.astype(LD) @ Ml).astype(np.float64))
    return M, steps


def field_err(a, ref):
    """max |a - ref| relative to the largest entry of ref (absolute where ref is zero)"""
    ref = np.asarray(ref, dtype=LD)
    a = np.asarray(a).astype(LD).reshape(ref.shape)
    scale = np.abs(ref).max(initial=0)
    return float(np.abs(a - ref).max(initial=0) / (scale if scale > 0 else LD(1)))


class TallRef:
    """the Rayleigh-quotient problem f(X) = 1/2 tr(X'AX) on St(n, p) at the float64 point X, in longdouble"""

    def __init__(self, rowptr, col, val, X):
        self.A = (rowptr, col, val)
        self.X = np.asarray(X).astype(LD)
        self.n, self.p = self.X.shape
        self.AX = spmm(rowptr, col, val, self.X)
        self.S = sym(self.X.T @ self.AX)

    def gram(self, Z, X=None):
        return (self.X if X is None else np.asarray(X).astype(LD)).T @ np.asarray(Z).astype(LD)

    def gram_scale(self, Z):
        return np.abs(self.X).T @ np.abs(np.asarray(Z).astype(LD))

    def project(self, Z):
        Z = np.asarray(Z).astype(LD)
        return Z - self.X @ sym(self.X.T @ Z)

    def f(self):
        return np.trace(self.X.T @ self.AX) / 2

    def f_scale(self):
        """1/2 tr(|X|'(|A| |X|)): the sum of the absolute values of the terms of f"""
        return np.trace(np.abs(self.X).T @ spmm(*self.A, self.X, absolute=True)) / 2

    def grad(self):
        return self.AX - self.X @ self.S

    def hess(self, V):
        V = np.asarray(V).astype(LD)
        return self.project(spmm(*self.A, V) - V @ self.S)

    def precon(self, dinv, r):
        return self.project(np.asarray(dinv).astype(LD)[:, None] * np.asarray(r).astype(LD))

    def dots(self, eta):
        """<eta, H eta>, <H eta, H eta>, <eta, eta>"""
        eta = np.asarray(eta).astype(LD)
        h = self.hess(eta)
        return (eta * h).sum(), (h * h).sum(), (eta * eta).sum()

    def retract(self, V):
        return polar(self.X + np.asarray(V).astype(LD))[0]


def stpcg(hess, g, Delta, max_iterations, dtype=LD):
    """Steihaug-Toint CG on the model <g, s> + 1/2 <s, H s> without a preconditioner, the residual rule switched off
    (a fixed number of passes): (s, passes, why) with why in "maxit", "boundary" (step beyond Delta or kappa <= 0)"""
    g = np.asarray(g).astype(dtype)
    s, r = np.zeros_like(g), g.copy()
    p = -r
    rv = (r * r).sum()
    for k in range(max_iterations):
        Hp = np.asarray(hess(p)).astype(dtype)
        kappa = (p * Hp).sum()
        ss, sp, pp = (s * s).sum(), (s * p).sum(), (p * p).sum()
        alpha = rv / kappa if kappa != 0 else dtype(np.inf)
        if kappa <= 0 or ss + 2 * alpha * sp + alpha * alpha * pp > dtype(Delta) ** 2:
            sigma = (-sp + np.sqrt(sp * sp + pp * (dtype(Delta) ** 2 - ss))) / pp
            return s + sigma * p, k, "boundary"
        s = s + alpha * p
        r = r + alpha * Hp
        rv_new = (r * r).sum()
        p = -r + (rv_new / rv) * p
        rv = rv_new
    return s, max_iterations, "maxit"


# ---- points, tangents and the inputs of a case ----
def stiefel_point(n, p, seed):
    """a random point on St(n, p): orthonormalised in longdouble, rounded once"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return orthonormalise(rng.normal(size=(n, p))).astype(np.float64)


def _tangent(X, Z):
    """P_X(Z) in longdouble, rounded once"""
    X = np.asarray(X).astype(LD)
    Z = np.asarray(Z).astype(LD)
    return (Z - X @ sym(X.T @ Z)).astype(np.float64)


def hard_name(p, n, k):
    return f"p{p}_n{n}_cond1e{k}"


HARD_CASES = tuple(hard_name(p, n or p, k) for p in HARD_P for n in HARD_N for k in HARD_COND)


@functools.lru_cache(maxsize=None)
def hard_retraction(name):
    """dict(n, p, cap, X, V, U, s, cond, floor): a tangent V at X whose singular values make cond(Y'Y), Y = X + V, about
    the number in the name.  Y'Y = I + V'V, so cond = (1 + smax^2) / (1 + smin^2): one direction carries smax (a
    trust-region step dominated by one direction: smax = 1e3 for 1e6), the others 0.1 ... 1.  n >= 2 p: V = Q diag(s) R'
    with Q orthonormal and orthogonal to X; else (St(p, p) has no normal space) V = X Omega, Omega skew with rotation
    rates s in pairs, and one rate 0 if p is odd.  V is rounded once, so it is tangent to rounding only; cond is taken
    from the singular values of the float64 Y itself"""
    p, n, k = map(int, re.fullmatch(r"p(\d+)_n(\d+)_cond1e(\d+)", name).groups())
    target = LD(10) ** k
    rng = np.random.Generator(np.random.PCG64(900 + 37 * p + 11 * n + k))
    X = stiefel_point(n, p, seed=5000 + 13 * n + p)
    Xl = X.astype(LD)
    R = orthonormalise(rng.normal(size=(p, p)))
    if n >= 2 * p:
        small = np.linspace(0.1, 1.0, p - 1).astype(LD)
        smax = np.sqrt(target * (1 + small.min() ** 2) - 1)
        Q = rng.normal(size=(n, p)).astype(LD)
        for _ in range(2):
            Q = Q - Xl @ (Xl.T @ Q)
        Q = orthonormalise(Q)
        V = (Q * np.concatenate([[smax], small])) @ R.T
    else:
        pairs = p // 2
        small = np.linspace(0.1, 1.0, pairs - 1).astype(LD)
        smin = LD(0) if p % 2 else small.min()
        rates = np.concatenate([[np.sqrt(target * (1 + smin ** 2) - 1)], small])
        B = np.zeros((p, p), dtype=LD)
        for q, th in enumerate(rates):
            B[2 * q, 2 * q + 1], B[2 * q + 1, 2 * q] = -th, th
        V = Xl @ (R @ B @ R.T)
    V = V.astype(np.float64)
    U, s = polar(Xl + V.astype(LD))
    return dict(name=name, n=n, p=p, cap=float(target), X=X, V=V, U=U, s=s, cond=float((s.max() / s.min()) ** 2),
                floor=gram_floor(Xl + V.astype(LD), U))


def inputs(n, p):
    """dict(X, Z, W, V, eta, r, dinv): the point, two fields with no relation to it (Z, W: asymmetric operands of the Gram,
    the argument of the projection), the moderate step V = 0.3 P_X(Z), a tangent eta, a residual r, inverse row weights"""
    rng = np.random.Generator(np.random.PCG64(31 * n + p))
    X = stiefel_point(n, p, seed=1000 + 17 * n + p)
    Z, W, r = rng.normal(size=(n, p)), rng.normal(size=(n, p)), rng.normal(size=(n, p))
    V = (LD(0.3) * _tangent(X, Z).astype(LD)).astype(np.float64)
    return dict(X=X, Z=Z, W=W, V=V, r=r, dinv=np.linspace(0.5, 2.0, n), etas=[_tangent(X, rng.normal(size=(n, p))) for _ in range(1)])


@functools.lru_cache(maxsize=None)
def reference_values(n, p, form, large=False):
    """every longdouble reference the GPU tests compare, once per case.  eta is a tangent built so that
    <eta, H eta> > 0.3 |eta| |H eta| (H is indefinite; a solve whose first curvature is not positive leaves no trace to
    read it from, and a curvature that nearly cancels is no fair object of a relative bar); large: the operations of the large case only"""
    rowptr, col, val = matrix(n, form)
    q = inputs(n, p)
    ref = TallRef(rowptr, col, val, q["X"])
    out = dict(q, n=n, p=p, form=form, rowptr=rowptr, col=col, val=val, ref=ref)
    out["gram"], out["gram_scale"] = ref.gram(q["Z"]), ref.gram_scale(q["Z"])
    out["project"] = ref.project(q["Z"])
    out["retract"] = ref.retract(q["V"])
    out["grad"] = ref.grad()
    out["eta"] = q["etas"][0]
    if not large:
        out["spmm"], out["spmm_scale"] = spmm(rowptr, col, val, q["W"]), spmm(rowptr, col, val, q["W"], absolute=True)
        out["f"], out["f_scale"] = ref.f(), ref.f_scale()
        out["precon"] = ref.precon(q["dinv"], q["r"])
        if n == p:       # St(p, p): f is constant, the gradient and the Hessian vanish, no solve has a curvature to show
            out["dots"] = None
            out["hess"] = ref.hess(out["eta"])
            del out["etas"]
            return out
        # eta <- P_X(eta / |eta| + H eta / |H eta|), rounded once, until <eta, H eta> > 0.3 |eta| |H eta|: every step turns
        # eta towards the positive end of the spectrum of H
        eta = q["etas"][0]
        for _ in range(40):
            k, hh, ee = ref.dots(eta)
            if k > LD(0.3) * np.sqrt(hh * ee):
                break
            el = eta.astype(LD)
            eta = _tangent(q["X"], el / np.sqrt(ee) + ref.hess(el) / np.sqrt(hh))
        else:
            raise RuntimeError(f"the curvature along eta is not safely positive at n = {n}, p = {p}, {form}")
        out["eta"] = eta
        out["dots"] = ref.dots(out["eta"])
    out["hess"] = ref.hess(out["eta"])
    del out["etas"]
    return out
