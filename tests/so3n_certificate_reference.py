"""The global-optimality certificate of chordal rotation averaging on SO(3)^N, restated in numpy (a helper module for
test_cpu_so3n_certificate.py and test_gpu_so3n_certificate.py; not a conftest).  Written from the mathematics alone --
it shares no code with the library and none with tests/so3_cases.py's So3Ref -- in float64 and in longdouble (`dtype`).

    f(R) = 1/2 sum_e w_e |R_j - R_i Rt_e|_F^2,  e = (i -> j)
    Y in R^{3N x 3}: block Y_i = R_i'                     Lap: the 3N x 3N connection Laplacian,
    Lap_ii = degw_i I,  Lap_ij = -w_e Rt_e,  Lap_ji = -w_e Rt_e'          f = const + 1/2 tr(Y' Lap Y)
    Q_i = R_i' (L R)_i = sum over the edges at i of w (I - R_i' R_nbr M),  M = Rt_e' at the first node of e, Rt_e at the second
    S(R) = Lap - BlockDiag(C_i),  C_i = sym(Q_i)

Facts the tests hold: tr(Y'SY) = 0 at every R; |S Y|_F = |skew Q|_F with skew Q_i = (Q_i - Q_i') / 2; f(R') >= f(R) +
(3N / 2) min(lambda_min(S), 0) for every R' in O(3)^N; on an N-cycle with identity measurements and unit weights the
winding R_i = rot_z(2 pi i / N) is a critical point with f = N (2 - 2 cos(2 pi / N)) and the spectrum of S starts with
2 cos(2 pi / N) - 2 twice, then 0 three times."""
import numpy as np

LD = np.longdouble


class CertRef:
    def __init__(self, N, ei, ej, Rt, w, R, dtype=np.float64):
        self.N, self.dtype = int(N), dtype
        self.ei, self.ej = np.asarray(ei, dtype=np.int64), np.asarray(ej, dtype=np.int64)
        self.Rt = np.asarray(Rt).astype(dtype).reshape(-1, 3, 3)
        self.w = np.asarray(w).astype(dtype).reshape(-1)
        self.R = np.asarray(R).astype(dtype).reshape(self.N, 3, 3)
        self._C = self._Q = None

    # -- per-node sums over the edges at each node: the first node's term, then the second node's -------------------
    def _scatter(self, at_first, at_second, shape):
        out = np.zeros((self.N,) + shape, dtype=self.dtype)
        np.add.at(out, self.ei, at_first)
        np.add.at(out, self.ej, at_second)
        return out

    def degw(self):
        return self._scatter(self.w, self.w, ())

    def abs_degw(self):
        """sum over the edges at each node of |w|"""
        return self._scatter(np.abs(self.w), np.abs(self.w), ())

    def Q(self):
        if self._Q is None:
            Ri, Rj, w = self.R[self.ei], self.R[self.ej], self.w[:, None, None]
            eye = np.eye(3, dtype=self.dtype)
            tr = lambda A: np.swapaxes(A, 1, 2)
            first = w * (eye - tr(Ri) @ Rj @ tr(self.Rt))     # at i: the neighbour is j, M = Rt'
            second = w * (eye - tr(Rj) @ Ri @ self.Rt)        # at j: the neighbour is i, M = Rt
            self._Q = self._scatter(first, second, (3, 3))
        return self._Q

    def C(self):
        if self._C is None:
            Q = self.Q()
            self._C = (Q + np.swapaxes(Q, 1, 2)) / 2
        return self._C

    def f(self):
        d = self.R[self.ej] - self.R[self.ei] @ self.Rt
        return (self.w * (d * d).sum(axis=(1, 2))).sum() / 2

    def stationarity(self):
        """|skew Q|_F, skew Q_i = (Q_i - Q_i') / 2"""
        Q = self.Q()
        K = (Q - np.swapaxes(Q, 1, 2)) / 2
        return np.sqrt((K * K).sum())

    def trace_C(self):
        C = self.C()
        return (C[:, 0, 0] + C[:, 1, 1] + C[:, 2, 2]).sum()

    def Y(self):
        """3N x 3: block i is R_i'"""
        return np.swapaxes(self.R, 1, 2).reshape(3 * self.N, 3).copy()

    def apply(self, X):
        """S X for X of shape (3N, k): (S x)_i = (degw_i I - C_i) x_i - sum over the edges at i of w M' x_nbr"""
        X = np.asarray(X).astype(self.dtype)
        k = X.shape[1]
        x = X.reshape(self.N, 3, k)
        E = self.degw()[:, None, None] * np.eye(3, dtype=self.dtype) - self.C()
        w = self.w[:, None, None]
        first = w * (self.Rt @ x[self.ej])                          # M' = Rt at the first node
        second = w * (np.swapaxes(self.Rt, 1, 2) @ x[self.ei])      # M' = Rt' at the second
        return (E @ x - self._scatter(first, second, (3, k))).reshape(3 * self.N, k)

    def dense(self):
        """S as a dense 3N x 3N matrix (small N)"""
        N = self.N
        S = np.zeros((3 * N, 3 * N), dtype=self.dtype)
        for e in range(self.ei.size):
            i, j, w = self.ei[e], self.ej[e], self.w[e]
            S[3 * i:3 * i + 3, 3 * i:3 * i + 3] += w * np.eye(3, dtype=self.dtype)
            S[3 * j:3 * j + 3, 3 * j:3 * j + 3] += w * np.eye(3, dtype=self.dtype)
            S[3 * i:3 * i + 3, 3 * j:3 * j + 3] -= w * self.Rt[e]
            S[3 * j:3 * j + 3, 3 * i:3 * i + 3] -= w * self.Rt[e].T
        C = self.C()
        for i in range(N):
            S[3 * i:3 * i + 3, 3 * i:3 * i + 3] -= C[i]
        return S

    def row_bar(self, X, rel=1e-12):
        """The operator bar, per row block and column: rel (sum_inc |w| + |degw_i|) max |X_c| over node i and its
        neighbours; shape (3N, k) (each node's figure three times)"""
        X = np.abs(np.asarray(X, dtype=np.float64))
        k = X.shape[1]
        xm = X.reshape(self.N, 3, k).max(axis=1)                   # (N, k): the node's own rows
        nb = xm.copy()
        np.maximum.at(nb, self.ei, xm[self.ej])
        np.maximum.at(nb, self.ej, xm[self.ei])
        scale = (self.abs_degw() + np.abs(self.degw())).astype(np.float64)
        return np.repeat(rel * scale[:, None] * nb, 3, axis=0)


def of_case(c, dtype=np.float64, R=None):
    """CertRef of a tests/so3_cases.py Case"""
    return CertRef(c.N, c.ei, c.ej, c.Rt, c.w, c.R if R is None else R, dtype)


# ---- the problems the certificate tests add to tests/so3_cases.py ----------------------------------------------------
def rot_z(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def winding(N):
    """(N, ei, ej, Rt, w, R): the N-cycle with identity measurements and unit weights at R_i = rot_z(2 pi i / N)"""
    ei = np.arange(N, dtype=np.int32)
    ej = ((ei + 1) % N).astype(np.int32)
    Rt = np.tile(np.eye(3).ravel(), (N, 1))
    R = np.stack([rot_z(2 * np.pi * i / N) for i in range(N)]).reshape(N, 9)
    return N, ei, ej, Rt, np.ones(N), R


def winding_lambda_min(N):
    return 2 * np.cos(2 * np.pi / N) - 2


def winding_f(N):
    return N * (2 - 2 * np.cos(2 * np.pi / N))


def _exp(v):
    t = np.linalg.norm(v)
    if t < 1e-14:
        return np.eye(3)
    K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]]) / t
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def ring_with_chords(N, chords, noise, seed):
    """(N, ei, ej, Rt, w, R_truth): a ring plus `chords` random chords, measurements R_i' R_j exp(noise * gaussian),
    weights uniform in [0.5, 2]"""
    r = np.random.default_rng(seed)
    Rgt = [_exp(r.normal(size=3)) for _ in range(N)]
    ei = list(range(N))
    ej = [(i + 1) % N for i in range(N)]
    for _ in range(chords):
        a, b = r.choice(N, 2, replace=False)
        ei.append(int(a))
        ej.append(int(b))
    Rt = np.stack([Rgt[i].T @ Rgt[j] @ _exp(noise * r.normal(size=3)) for i, j in zip(ei, ej)]).reshape(-1, 9)
    w = r.uniform(0.5, 2, len(ei))
    return N, np.array(ei, dtype=np.int32), np.array(ej, dtype=np.int32), Rt, w, np.stack(Rgt).reshape(N, 9)
