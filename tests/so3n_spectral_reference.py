"""Spectral initialisation of chordal rotation averaging on SO(3)^N, restated in numpy (a helper module for
test_cpu_so3n_spectral.py and test_gpu_so3n_spectral.py; not a conftest).  Written from the mathematics alone: the dense
connection Laplacian from the edge list, `eigh`, SVD rounding and the global sign rule.

    Lap_ii = degw_i I,  Lap_ij = -w_e Rt_e,  Lap_ji = -w_e Rt_e'  for e = (i -> j)
    f(R) = 1/2 sum_e w_e |R_j - R_i Rt_e|_F^2 = 1/2 tr(Y' Lap Y),  Y_i = R_i', when every Rt_e is a rotation
    V: the eigenvectors of the three lowest eigenvalues;  M_i = V[3i .. 3i+2, :]'
    global sign: sum_i sign(det M_i) < 0  =>  round -V (a tie does not flip)
    R_i = U diag(1, 1, det(U V')) V'  for  M_i = U Sigma V'  (the nearest rotation in the Frobenius norm)
    (N / 2) (lambda_1 + lambda_2 + lambda_3) <= min f: Y' Y = N I for every point of SO(3)^N
The problems are ring_with_chords and winding of so3n_certificate_reference.py."""
import numpy as np

import so3n_certificate_reference as cr

# (N, chords, noise, seed) of ring_with_chords, and the cycle lengths of winding
RING_CASES = ((7, 3, 0.0, 1), (40, 30, 0.0, 2), (40, 30, 0.2, 3), (150, 100, 0.2, 4), (65, 40, 0.2, 6), (257, 200, 0.3, 7))
WINDING_CASES = (12, 25)


def problem(case):
    """(N, ei, ej, Rt, w, R) with R the ground truth of a ring or the winding of a cycle"""
    return cr.winding(case) if isinstance(case, int) else cr.ring_with_chords(*case)


def dense_laplacian(N, ei, ej, Rt, w):
    L = np.zeros((3 * N, 3 * N))
    Rt = np.asarray(Rt, dtype=np.float64).reshape(-1, 3, 3)
    for e in range(len(ei)):
        i, j = int(ei[e]), int(ej[e])
        L[3 * i:3 * i + 3, 3 * i:3 * i + 3] += w[e] * np.eye(3)
        L[3 * j:3 * j + 3, 3 * j:3 * j + 3] += w[e] * np.eye(3)
        L[3 * i:3 * i + 3, 3 * j:3 * j + 3] -= w[e] * Rt[e]
        L[3 * j:3 * j + 3, 3 * i:3 * i + 3] -= w[e] * Rt[e].T
    return L


def objective(ei, ej, Rt, w, R):
    R = np.asarray(R, dtype=np.float64).reshape(-1, 3, 3)
    d = R[np.asarray(ej)] - R[np.asarray(ei)] @ np.asarray(Rt, dtype=np.float64).reshape(-1, 3, 3)
    return float((np.asarray(w) * (d * d).sum(axis=(1, 2))).sum() / 2)


def panel_blocks(V):
    """(N, 3, 3): M_i = V[3i .. 3i+2, :]' of a 3N x 3 panel"""
    V = np.asarray(V, dtype=np.float64)
    return np.swapaxes(V.reshape(-1, 3, 3), 1, 2).copy()


def round_blocks(M):
    """SVD rounding of (n, 3, 3) blocks: dict(R (n, 3, 3), d (the sign det(U V')), sep ((sigma_2 + d sigma_3) / sigma_1),
    degenerate (bool: a non-finite entry or the zero block -> R = I, sep = nan), negative (det M < 0))"""
    M = np.asarray(M, dtype=np.float64).reshape(-1, 3, 3)
    n = M.shape[0]
    degenerate = ~np.isfinite(M).all(axis=(1, 2)) | (np.abs(M).max(axis=(1, 2)) == 0)
    safe = np.where(degenerate[:, None, None], np.eye(3), M)
    U, s, Vt = np.linalg.svd(safe)
    d = np.where(np.linalg.det(U @ Vt) < 0, -1.0, 1.0)
    U = U.copy()
    U[:, :, 2] *= d[:, None]
    R = np.where(degenerate[:, None, None], np.eye(3), U @ Vt)
    sep = np.where(degenerate, np.nan, (s[:, 1] + d * s[:, 2]) / s[:, 0])
    with np.errstate(invalid="ignore"):
        negative = np.linalg.det(np.where(degenerate[:, None, None], np.eye(3), M)) < 0
    return dict(R=R, d=d, sep=sep, degenerate=degenerate, negative=negative & ~degenerate, n=n)


def round_panel(V):
    """the sign rule, then round_blocks: adds flipped, and `negative` counts the blocks of V as given"""
    M = panel_blocks(V)
    sgn = np.sign(np.linalg.det(M))
    flipped = bool(sgn.sum() < 0)
    out = round_blocks(-M if flipped else M)
    out.update(flipped=flipped, negative=sgn < 0, sign_sum=int(sgn.sum()))
    return out


def spectral(N, ei, ej, Rt, w):
    """dict(L, lam (all 3N eigenvalues), V (3N x 3), R (N, 9) the rounded point, f, lower_bound, flipped, negative (count),
    sign_sum)"""
    L = dense_laplacian(N, ei, ej, Rt, w)
    lam, vec = np.linalg.eigh(L)
    V = vec[:, :3]
    r = round_panel(V)
    R = r["R"].reshape(N, 9)
    return dict(L=L, lam=lam, V=V, R=R, f=objective(ei, ej, Rt, w, R), lower_bound=N / 2 * float(lam[:3].sum()),
                flipped=r["flipped"], negative=int(r["negative"].sum()), sign_sum=r["sign_sum"], sep=r["sep"])


def _orth(rng, n, det):
    Q = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]
    Q[:, :, 0] *= (np.sign(np.linalg.det(Q)) * det)[:, None]
    return Q


def synthetic_blocks(N, seed=0):
    """(N, 3, 3) blocks for the rounding tests with prescribed singular values: both determinant signs, scales from 1e-3
    to 1e3, exact rotations, exact reflections, one zero block (N >= 5) -- every other block with (sigma_2 + d sigma_3) /
    sigma_1 >= 0.05, except the exact reflections: an orthogonal block with det < 0 has three equal singular values, so its
    separation is 0 and its nearest rotation is not unique (only the distance to it is defined).  Singular values: sigma_1 = 1, sigma_2 in [0.3, 1], sigma_3 in [0, sigma_2 - 0.06] where det < 0 and in
    [0.001, sigma_2] where det > 0, so sep >= 0.06 (det < 0) or >= 0.3 (det > 0) before rounding."""
    rng = np.random.default_rng(1000 + 7 * N + seed)
    det = np.where(rng.uniform(size=N) < 0.5, -1.0, 1.0)
    U, V = _orth(rng, N, np.ones(N)), _orth(rng, N, det)
    s2 = rng.uniform(0.3, 1.0, size=N)
    s3 = np.where(det < 0, rng.uniform(0, 1, size=N) * (s2 - 0.06), 0.001 + rng.uniform(0, 1, size=N) * (s2 - 0.001))
    s = np.stack([np.ones(N), s2, s3], axis=1)
    scale = 10.0 ** rng.uniform(-3, 3, size=N)
    M = (U * s[:, None, :]) @ np.swapaxes(V, 1, 2) * scale[:, None, None]
    kinds = np.zeros(N, dtype=np.int64)            # 0 general, 1 exact rotation, 2 exact reflection, 3 zero
    if N >= 2:
        M[0], kinds[0] = cr.rot_z(0.7) @ cr._exp(np.array([0.3, -1.0, 0.2])), 1
        M[1], kinds[1] = np.diag([1.0, -1.0, 1.0]) @ cr.rot_z(-2.1), 2
    if N >= 5:
        M[2], kinds[2] = np.eye(3), 1
        M[3], kinds[3] = -np.eye(3), 2
        M[N // 2], kinds[N // 2] = 0.0, 3
    return M, kinds
