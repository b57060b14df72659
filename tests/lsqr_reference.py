"""A plain numpy restatement of LSQR (Paige & Saunders) as LinearAlgebra/IterativeSolvers.h states it (reference
:552-855): the same statements in the same order, in any numpy precision.  numpy.longdouble is the reference of record
for the device solve (tests/test_gpu_lsqr_parity.py); float64 with re-associated inner products gives the conditioning
floor of a case (how far the algorithm itself moves when only the order of its sums changes).

Nothing here knows about the device code: the matrix products are scipy's row-by-row sums over a CSR copy in the working
precision, the inner products are sums in the order `order` names."""
import numpy as np
import scipy.sparse as sps

# MI_LSQR_EXIT_* (include/mi355opt.h)
EXIT_MAXIT, EXIT_S1, EXIT_S2, EXIT_S3, EXIT_S4, EXIT_TRIVIAL = 0, 1, 2, 3, 4, 5

DELTA_DEFAULT = float(np.sqrt(np.finfo(np.float64).max))

# the summation orders of the inner products: the first is the reference's own sequential loop
SEQUENTIAL = None
REASSOCIATIONS = (("pairwise",), ("block", 64), ("reverse",), ("perm", 7))


def operators(A, dtype):
    """(A, A') as CSR matrices in the working precision; their products are one sequential sum per row.  lsqr takes
    the pair in place of A, so that several solves on one matrix share the conversion."""
    M = sps.csr_matrix(A, dtype=np.float64)
    Mt = sps.csr_matrix(M.T)
    for m in (M, Mt):
        m.sum_duplicates()
        m.sort_indices()
    return M.astype(dtype), Mt.astype(dtype)


def _inner(order, n):
    """the inner product of two vectors of length n with its sum taken in the order named"""
    if order is None:
        return lambda a, b: np.cumsum(a * b)[-1]
    if order[0] == "pairwise":
        return lambda a, b: np.sum(a * b)
    if order[0] == "reverse":
        return lambda a, b: np.cumsum((a * b)[::-1])[-1]
    if order[0] == "block":
        at = np.arange(0, n, order[1])
        return lambda a, b: np.sum(np.add.reduceat(a * b, at))
    if order[0] == "perm":
        p = np.random.default_rng(order[1]).permutation(n)
        return lambda a, b: np.cumsum((a * b)[p])[-1]
    raise ValueError(order)


def lsqr(A, b, max_iterations=1000, lam=0.0, btol=1e-6, Atol=1e-6, Acond_limit=1e8, Delta=None,
         dtype=np.longdouble, order=SEQUENTIAL, keep_x=()):
    """min |A x - b|^2 + lam |x|^2  s.t. |x| <= Delta.  A: dense or scipy.sparse (n_y x n_x), or operators(A, dtype).

    Returns a dict: x, xnorm, iterations, exit_reason (MI_LSQR_EXIT_* numbering), rbar_norm, Arnorm, Anorm, Acond;
    trace: one row per pass with xnorm, rbar_norm, Arnorm, Anorm, Acond, alpha, beta as they stand at the end of it;
    sides: one dict per pass with the two sides (left, right) of every comparison the pass evaluated --
    "branch" (xnorm <= Delta, :779), "s1" (<=), "s2" (<=), "s3" (>=), "s4" (>=); a rule behind the one that ended the
    pass is not evaluated and not listed.  Where the step was shortened, xnorm IS Delta by assignment, so "s4" lists the
    estimate before the assignment: that is the comparison which decided it;
    shortened: the passes that took the shortened step (:785-793);  iterates: {k: x after pass k} for k in keep_x."""
    T = dtype
    M, Mt = A if isinstance(A, tuple) else operators(A, T)
    ny, nx = M.shape
    b = np.asarray(b, dtype=np.float64).astype(T)
    ipx, ipy = _inner(order, nx), _inner(order, ny)
    lam, btol, Atol, Acond_limit = T(lam), T(btol), T(Atol), T(Acond_limit)
    Delta = T(DELTA_DEFAULT if Delta is None else Delta)
    zero = T(0)

    out = dict(xnorm=zero, iterations=0, exit_reason=EXIT_MAXIT, rbar_norm=zero, Arnorm=zero, Anorm=zero, Acond=zero,
               trace=[], sides=[], shortened=[], iterates={})
    xx = Anorm = Acond = D_frob_sq = zero
    sqrt_lam = np.sqrt(lam)

    u = b.copy()
    v = Mt.dot(u)
    x = zero * v
    alpha = np.sqrt(ipx(v, v))
    beta = np.sqrt(ipy(u, u))
    w = np.zeros(nx, dtype=T)
    if beta > 0:
        u = u / beta
    if alpha > 0:
        v = v / alpha
        alpha = alpha / beta
        w = v.copy()
    Arnorm = alpha * beta
    out.update(x=x, Arnorm=Arnorm)
    if Arnorm == 0:
        out.update(exit_reason=EXIT_TRIVIAL)
        return out
    bnorm = rbar_norm = beta
    out.update(rbar_norm=rbar_norm)
    rhobar, phibar = alpha, beta
    cs2, sn2, z, res2 = T(-1), zero, zero, zero
    xnorm = zero

    k = 0
    while k < max_iterations:
        u = M.dot(v) - alpha * u
        beta = np.sqrt(ipy(u, u))
        if beta > 0:
            u = u / beta
            Anorm = np.sqrt(Anorm * Anorm + alpha * alpha + beta * beta + lam)
            v = Mt.dot(u) - beta * v
            alpha = np.sqrt(ipx(v, v))
            if alpha > 0:
                v = v / alpha

        rhobar1 = np.sqrt(rhobar * rhobar + lam)
        cs1 = rhobar / rhobar1
        sn1 = sqrt_lam / rhobar1
        psi = sn1 * phibar
        phibar = phibar * cs1

        rho = np.sqrt(rhobar1 * rhobar1 + beta * beta)
        cs = rhobar1 / rho
        sn = beta / rho
        theta = sn * alpha
        rhobar = -cs * alpha
        phi = cs * phibar
        phibar = phibar * sn
        tau = sn * phi

        delta = sn2 * rho
        gammabar = -cs2 * rho
        rhs = phi - delta * z
        zbar = rhs / gammabar
        gamma = np.sqrt(gammabar * gammabar + theta * theta)
        cs2 = gammabar / gamma
        sn2 = theta / gamma
        z = rhs / gamma

        w_sq = ipx(w, w)
        d_sq = w_sq / (rho * rho)
        xnorm = np.sqrt(xx + zbar * zbar)
        xx = xx + z * z
        t2 = -theta / rho
        sides = {"branch": (xnorm, Delta)}
        estimate = xnorm
        if xnorm <= Delta:
            t1 = phi / rho
        else:
            xtx = ipx(x, x)
            wtx = ipx(w, x)
            t1 = (-wtx + np.sqrt(wtx * wtx + w_sq * (Delta * Delta - xtx))) / w_sq
            xnorm = Delta
            out["shortened"].append(k)
        x = x + t1 * w
        w = v + t2 * w

        D_frob_sq = D_frob_sq + d_sq
        Acond = Anorm * np.sqrt(D_frob_sq)
        res1 = phibar * phibar
        res2 = res2 + psi * psi
        rbar_norm = np.sqrt(res1 + res2)
        Arnorm = alpha * abs(tau)

        out["trace"].append(dict(xnorm=xnorm, rbar_norm=rbar_norm, Arnorm=Arnorm, Anorm=Anorm, Acond=Acond,
                                 alpha=alpha, beta=beta))
        out["sides"].append(sides)
        if k in keep_x:
            out["iterates"][k] = x.copy()
        ended = None
        sides["s1"] = (rbar_norm, btol * bnorm + Atol * Anorm * xnorm)
        if sides["s1"][0] <= sides["s1"][1]:
            ended = EXIT_S1
        if ended is None:
            sides["s2"] = (Arnorm, Atol * Anorm * rbar_norm)
            if sides["s2"][0] <= sides["s2"][1]:
                ended = EXIT_S2
        if ended is None:
            sides["s3"] = (Acond, Acond_limit)
            if Acond >= Acond_limit:
                ended = EXIT_S3
        if ended is None:
            sides["s4"] = (estimate, Delta)
            if xnorm >= Delta:
                ended = EXIT_S4
        if ended is not None:  # left through a break: the loop index is not advanced (:696)
            out.update(exit_reason=ended)
            break
        k += 1
    out.update(x=x, xnorm=xnorm, iterations=k, rbar_norm=rbar_norm, Arnorm=Arnorm, Anorm=Anorm, Acond=Acond)
    return out


SCALARS = ("xnorm", "rbar_norm", "Arnorm", "Anorm", "Acond")


def margin(sides):
    """the smallest relative distance between the two sides of any comparison of any pass (1 where one side is 0 and
    the other is not; 0 < 0 <= 0 by both being exactly zero counts as decided: it is no rounding tie)"""
    worst = np.inf
    for row in sides:
        for left, right in row.values():
            left, right = abs(float(left)), abs(float(right))
            if left == 0 and right == 0:
                continue
            if np.isinf(left) or np.isinf(right):
                continue
            worst = min(worst, abs(left - right) / max(left, right))
    return worst


def deviation(r, ref):
    """how far the solve r lies from ref in the quantities the parity test compares: max-norm relative in x, relative
    in xnorm, rbar_norm, Anorm, Acond (final and per pass), Arnorm in units of Anorm * rbar_norm"""
    def rel(a, c):
        a, c = np.longdouble(a), np.longdouble(c)
        return 0.0 if a == c else float(abs(a - c) / abs(c))
    xs = np.abs(ref["x"]).max()
    e = float(np.abs(r["x"].astype(np.longdouble) - ref["x"]).max() / xs) if xs > 0 else 0.0
    rows = list(zip(r["trace"], ref["trace"])) + [(r, ref)]
    for a, c in rows:
        for key in ("xnorm", "rbar_norm", "Anorm", "Acond"):
            e = max(e, rel(a[key], c[key]))
        scale = np.longdouble(c["Anorm"]) * np.longdouble(c["rbar_norm"])
        if scale > 0:
            e = max(e, float(abs(np.longdouble(a["Arnorm"]) - c["Arnorm"]) / scale))
    return e
