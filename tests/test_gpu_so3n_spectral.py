"""GPU tests of the spectral initialisation of SO(3)^N (k_so3_lap_diag, k_so3_lap_jacobi, k_so3_round_sign, k_so3_round;
mi_so3n_laplacian / mi_so3n_lap_jacobi / mi_so3n_round / mi_so3n_project; MI355::RotationAveraging::
spectral_initialization) against tests/so3n_spectral_reference.py.

Bars.  Laplacian product: row-wise 1e-12 (|Lap| |X|)_row against the dense longdouble product.  Rounding: |R_dev - R_ref|_F
<= 1e-12 sigma_1 / (sigma_2 + d sigma_3) against numpy's SVD rounding of the same bits -- the conditioning of the polar
factor times a rounding allowance; for an exact reflection (three equal singular values, d = -1) the bar is infinite, as
it must be: the nearest rotation is not unique there, and what is held instead is the distance to it.  Eigenvectors:
|P_dev - P_ref|_2 <= 4 tau |Lap|_2 / (lambda_4 - lambda_3), Davis-Kahan on LOBPCG's stopping rule (every column's residual
is at most tau (|Lap|est + |theta|) |x| <= 2 tau |Lap|_2, three columns: 2 sqrt(3) < 4).  Bit contracts are exact."""
import functools

import numpy as np
import pytest

import so3_cases as sc
import so3n_certificate_reference as cr
import so3n_spectral_reference as sr

pytestmark = pytest.mark.gpu

LD = np.longdouble
SIZES = (1, 2, 7, 65, 257)     # 65 crosses a 64-lane slice, 257 a 4-slice workgroup
TAU = 1e-9


@functools.lru_cache(maxsize=None)
def _graph(N):
    """(N, ei, ej, Rt, w, R) of the kernel tests: the tiny cases, then the rings of the reference's list"""
    if N <= 2:
        c = sc.case("tiny_%d" % N)
        return c.N, c.ei, c.ej, c.Rt, c.w, c.R
    return sr.problem({7: sr.RING_CASES[0], 65: sr.RING_CASES[4], 257: sr.RING_CASES[5]}[N])


@functools.lru_cache(maxsize=None)
def _spectral_reference(case):
    N, ei, ej, Rt, w, Rgt = sr.problem(case)
    s = sr.spectral(N, ei, ej, Rt, w)
    s.update(f_truth=sr.objective(ei, ej, Rt, w, Rgt), L2=float(np.abs(s["lam"]).max()), sum_w=float(np.sum(w)))
    s["bar"] = 4 * TAU * s["L2"] / float(s["lam"][3] - s["lam"][2])
    for a in (s["L"], s["V"], s["R"]):
        a.setflags(write=False)
    return s


def _panel(Zvec, m, k):
    return Zvec.numpy()[:m * k].reshape(k, m).T           # column-major m x k


def _up(ctx, X):
    return ctx.upload(np.ascontiguousarray(np.asarray(X, dtype=np.float64).T).ravel())


def _empty_problem(ctx, N):
    """a problem of N rotations without edges: what mi_so3n_round / mi_so3n_project need is N alone"""
    return ctx.so3n(N, np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros((0, 9)), np.zeros(0))


def _check_product(lap, ctx, L, m, tag):
    X = np.random.Generator(np.random.PCG64(m + 3)).normal(size=(m, 7))
    X[:, 1] *= 1e6
    Zref = L.astype(LD) @ X.astype(LD)
    bar = 1e-12 * (np.abs(L) @ np.abs(X))
    cols = {}
    for k in (1, 3, 7):
        Z = _panel(lap.apply(k, _up(ctx, X[:, :k])), m, k)
        err = np.abs((Z.astype(LD) - Zref[:, :k]).astype(np.float64))
        print(tag, "k", k, "worst error / bar", float((err / np.maximum(bar[:, :k], 1e-300)).max()))
        assert np.all(err <= bar[:, :k]), (tag, k)
        cols[k] = Z
    assert np.array_equal(cols[1][:, 0], cols[7][:, 0]) and np.array_equal(cols[3], cols[7][:, :3])
    return X, cols[7]


@pytest.mark.parametrize("N", SIZES)
def test_laplacian_product_reweighted_blocks_and_own_slot(ctx, N):
    N, ei, ej, Rt, w, R = _graph(N)
    m = 3 * N
    prob = ctx.so3n(N, ei, ej, Rt, w)
    lap = prob.laplacian()
    X, Z7 = _check_product(lap, ctx, sr.dense_laplacian(N, ei, ej, Rt, w), m, "N %d" % N)
    from optimization_amd import capi
    with pytest.raises(capi.MiError):
        lap.null_panel()
    # the three-block form has the bits of the assembled panel: columns [0, 2) | [2, 5) | [5, 7) from two panels
    P1, P2 = _up(ctx, X[:, 5:7]), _up(ctx, np.hstack([X[:, 2:5], X[:, 0:2]]))
    blocks = [(P2.view(3 * m, 2 * m), 2), (P2.view(0, 3 * m), 3), (P1, 2)]
    assert np.array_equal(_panel(lap.apply_blocks(blocks), m, 7), Z7)
    # a certificate at another point lives in a slot of its own
    Rv = ctx.upload(np.roll(np.asarray(R).reshape(N, 9), 1, axis=0).ravel())
    cert, _ = prob.certificate(Rv)
    assert cert.h.value != lap.h.value
    assert np.array_equal(_panel(lap.apply(7, _up(ctx, X)), m, 7), Z7)
    if N > 1:
        assert not np.array_equal(_panel(cert.apply(7, _up(ctx, X)), m, 7), Z7)
    # ... and the next mi_so3n_laplacian call does not rebind the certificate
    before = cert.apply(3, _up(ctx, X[:, :3])).numpy()
    assert prob.laplacian().h.value == lap.h.value
    assert np.array_equal(cert.apply(3, _up(ctx, X[:, :3])).numpy(), before)
    # the reweighted Laplacian (Cauchy at the roll of the ground truth: weights well below the creation-time ones)
    prob.reweight(Rv, "cauchy", 0.5)
    w2 = prob.weights()
    if N > 1:
        assert np.all(w2 <= w) and np.any(w2 < np.asarray(w))
    lap2 = prob.laplacian()
    assert lap2.h.value == lap.h.value
    _check_product(lap2, ctx, sr.dense_laplacian(N, ei, ej, Rt, w2), m, "N %d reweighted" % N)


def _check_rounding(R, ref, tag):
    """R (N, 3, 3) from the device against round_blocks' dict: the bar, orthogonality, determinant"""
    live = ~ref["degenerate"]
    assert np.array_equal(R[~live], np.broadcast_to(np.eye(3), (int((~live).sum()), 3, 3)))
    err = np.linalg.norm((R - ref["R"]).reshape(-1, 9), axis=1)[live]
    with np.errstate(divide="ignore"):
        bar = 1e-12 / np.maximum(ref["sep"][live], 0.0)
    if err.size:
        print(tag, "worst error / bar", float((err / bar).max()), "worst error", float(err.max()))
    assert np.all(err <= bar), tag
    assert np.abs(np.swapaxes(R, 1, 2) @ R - np.eye(3)).max() <= 1e-14, tag
    assert np.abs(np.linalg.det(R) - 1).max() <= 1e-14, tag


@pytest.mark.parametrize("N", SIZES)
def test_rounding_on_synthetic_blocks(ctx, N):
    M, kinds = sr.synthetic_blocks(N)
    prob = _empty_problem(ctx, N)
    # --- the point form ---
    ref = sr.round_blocks(M)
    assert np.all((np.nan_to_num(ref["sep"], nan=1.0) >= 0.05) | (kinds == 2))
    Mv = ctx.upload(M.ravel())
    Rv, info = prob.project(Mv)
    R = Rv.numpy().reshape(N, 3, 3)
    _check_rounding(R, ref, "project N %d" % N)
    # an exact reflection: the distance to the nearest rotation is 2 whichever of them was taken
    for i in np.flatnonzero(kinds == 2):
        assert abs(np.linalg.norm(R[i] - M[i]) - 2.0) <= 1e-13
    for i in np.flatnonzero(kinds == 1):
        assert np.abs(R[i] - M[i]).max() <= 1e-14
    live = ~ref["degenerate"]
    G = np.swapaxes(M[live], 1, 2) @ M[live] - np.eye(3)
    defect = float(np.linalg.norm(G.reshape(-1, 9), axis=1).max()) if live.any() else 0.0
    assert info["degenerate"] == int(ref["degenerate"].sum()) == int((kinds == 3).sum())
    assert info["negative"] == int(ref["negative"].sum())
    assert abs(info["defect"] - defect) <= 1e-12 * max(defect, 1.0)
    inplace, info2 = prob.project(Mv, Mv)
    assert np.array_equal(inplace.numpy(), Rv.numpy()) and info2 == info
    # --- the panel form: V[3i .. 3i+2, :] = M_i' ---
    V = np.swapaxes(M, 1, 2).reshape(3 * N, 3)
    pref = sr.round_panel(V)
    Rp, pinfo = prob.round(_up(ctx, V))
    _check_rounding(Rp.numpy().reshape(N, 3, 3), pref, "round N %d" % N)
    assert pinfo["flipped"] == pref["flipped"] and pinfo["negative"] == int(pref["negative"].sum())
    assert pinfo["degenerate"] == int(pref["degenerate"].sum())
    if (~pref["degenerate"]).any():
        assert abs(pinfo["min_separation"] - float(np.nanmin(pref["sep"]))) <= 1e-13
    Rq, none = prob.round(_up(ctx, V), info=False)
    assert none is None and np.array_equal(Rq.numpy(), Rp.numpy())


def test_global_sign_rule(ctx):
    N = 65
    M, kinds = sr.synthetic_blocks(N, seed=1)
    keep = np.arange(N) % 6 == 0                            # 11 blocks keep their sign, the others are made negative
    sgn = np.sign(np.linalg.det(M))
    M = np.where(((sgn > 0) & ~keep)[:, None, None], -M, M)
    V = np.swapaxes(M, 1, 2).reshape(3 * N, 3)
    ref = sr.round_panel(V)
    assert ref["flipped"] and ref["sign_sum"] < 0
    prob = _empty_problem(ctx, N)
    Ra, ia = prob.round(_up(ctx, V))
    Rb, ib = prob.round(_up(ctx, -V))
    assert ia["flipped"] and not ib["flipped"]
    assert ia["negative"] == int(ref["negative"].sum()) and ib["negative"] == N - 1 - ia["negative"]   # (one zero block)
    assert np.array_equal(Ra.numpy(), Rb.numpy())           # -(-V) = V: the same bits are rounded
    _check_rounding(Ra.numpy().reshape(N, 3, 3), ref, "flipped panel")
    # a tie does not flip
    tie = np.stack([np.eye(3), np.diag([1.0, 1.0, -1.0])])
    _, it = _empty_problem(ctx, 2).round(_up(ctx, np.swapaxes(tie, 1, 2).reshape(6, 3)))
    assert not it["flipped"] and it["negative"] == 1


@pytest.mark.parametrize("name", ("isolated_1500", 257, 65, 2))
def test_lap_jacobi_is_x_over_degw_bit_for_bit(ctx, name):
    if isinstance(name, str):
        c = sc.case(name)
        N, ei, ej, Rt, w = c.N, c.ei, c.ej, c.Rt, c.w
    else:
        N, ei, ej, Rt, w, _ = _graph(name)
    degw = np.zeros(N)
    for e in range(len(ei)):                                # per node in edge order: the slot order
        degw[ei[e]] += w[e]
        degw[ej[e]] += w[e]
    if isinstance(name, str):
        assert degw[0] == 0 and degw[N - 1] == 0 and np.all(degw[128:192] == 0)
    k, m = 5, 3 * N
    X = np.random.Generator(np.random.PCG64(N)).normal(size=(m, k))
    d3 = np.repeat(np.where(degw != 0, degw, 1.0), 3)
    prob = ctx.so3n(N, ei, ej, Rt, w)
    Xv = _up(ctx, X)
    Z = prob.lap_jacobi(k, Xv)
    assert np.array_equal(_panel(Z, m, k), X / d3[:, None])
    prob.lap_jacobi(k, Xv, Xv)                              # in place
    assert np.array_equal(Xv.numpy(), Z.numpy())
    from optimization_amd import capi
    with pytest.raises(capi.MiError):
        prob.lap_jacobi(k + 1, Xv)                          # X too small
    with pytest.raises(capi.MiError):
        prob.lap_jacobi(0, Xv)


# ---- spectral_initialization through the template layer ------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness():
    from harness_spectral_so3n_py import SpectralSo3nHarness
    return SpectralSo3nHarness()


def _projector_distance(Va, Vb):
    Qa, Qb = np.linalg.qr(Va)[0], np.linalg.qr(Vb)[0]
    return float(np.linalg.norm(Qa @ Qa.T - Qb @ Qb.T, 2))


@pytest.mark.parametrize("case", sr.RING_CASES + sr.WINDING_CASES, ids=str)
def test_spectral_initialization_against_eigh(harness, case):
    N, ei, ej, Rt, w, _ = sr.problem(case)
    ref = _spectral_reference(case)
    r = harness.run(N, ei, ej, Rt, w, tau=TAU)
    assert r["rc"] == 0, r["err"]
    dist = _projector_distance(r["V"], ref["V"])
    print(case, {k: r[k] for k in ("iterations", "f", "lower_bound", "flipped", "min_separation")}, "eigenvalues",
          r["eigenvalues"], "subspace distance", dist, "bar", ref["bar"], "f(truth)", ref["f_truth"], "f(ref R0)", ref["f"])
    assert r["converged"] and r["degenerate"] == 0
    assert dist <= ref["bar"]
    assert np.abs(r["eigenvalues"] - ref["lam"][:3]).max() <= 2 * TAU * ref["L2"]
    # R against the numpy rounding of the device's own panel: identical inputs
    own = sr.round_panel(r["V"])
    assert r["flipped"] == own["flipped"]
    _check_rounding(r["R0"].reshape(N, 3, 3), own, "R0 of %s" % (case,))
    assert abs(r["min_separation"] - float(np.nanmin(own["sep"]))) <= 1e-13
    assert abs(r["f"] - sr.objective(ei, ej, Rt, w, r["R0"])) <= 1e-12 * ref["sum_w"]
    noise_free = isinstance(case, int) or case[2] == 0.0
    if noise_free:
        print(case, "f(R0)", r["f"], "derived bar", 32 * N * ref["sum_w"] * ref["bar"] ** 2)
        assert r["f"] <= 32 * N * ref["sum_w"] * ref["bar"] ** 2
        assert r["lower_bound"] <= r["f"] + 1e-300
    else:
        assert r["lower_bound"] <= r["f"] <= ref["f_truth"]
    # without the preconditioner: the same subspace within the same bar
    q = harness.run(N, ei, ej, Rt, w, tau=TAU, precondition=False)
    assert q["rc"] == 0, q["err"]
    distq = _projector_distance(q["V"], ref["V"])
    print(case, "unpreconditioned: iterations", q["iterations"], "subspace distance", distq)
    assert q["converged"] and distq <= ref["bar"]


@pytest.mark.parametrize("N", sr.WINDING_CASES)
def test_tnt_from_the_spectral_point_is_certified_on_the_cycle(harness, N):
    n, ei, ej, Rt, w, _ = cr.winding(N)
    r = harness.run(n, ei, ej, Rt, w, run_tnt=True)
    assert r["rc"] == 0, r["err"]
    print("cycle", N, {k: r[k] for k in ("iterations", "f", "f_final", "tnt_gradnorm", "tnt_iterations", "cert_lambda_min",
                                          "cert_eta", "cert_iterations")})
    assert r["converged"] and r["cert_converged"] and r["certified"]
    assert r["f_final"] <= 1e-12


@pytest.mark.parametrize("case", [c for c in sr.RING_CASES if c[2] == 0.2], ids=str)
def test_tnt_from_the_spectral_point_is_certified_at_noise_0_2(harness, case):
    N, ei, ej, Rt, w, _ = sr.problem(case)
    r = harness.run(N, ei, ej, Rt, w, run_tnt=True)
    assert r["rc"] == 0, r["err"]
    print(case, {k: r[k] for k in ("iterations", "f", "f_final", "lower_bound", "tnt_gradnorm", "tnt_iterations",
                                   "cert_lambda_min", "cert_eta", "cert_iterations", "tnt_status")})
    assert r["converged"] and r["cert_converged"] and r["certified"]
    assert r["f_final"] <= r["f"]


def test_without_edges_and_on_a_single_edge(harness):
    c = sc.case("tiny_1")
    r = harness.run(c.N, c.ei, c.ej, c.Rt, c.w)
    assert r["rc"] == 0, r["err"]
    assert r["iterations"] == 0 and r["converged"] and r["V"] is None and r["f"] == 0.0
    assert np.array_equal(r["R0"], np.eye(3).ravel())
    # N = 2: solved densely on the host (3N <= 96); a single edge is fitted exactly
    c = sc.case("tiny_2")
    r = harness.run(c.N, c.ei, c.ej, c.Rt, c.w)
    assert r["rc"] == 0, r["err"]
    print("tiny_2", r["f"], r["eigenvalues"], r["lower_bound"])
    assert r["iterations"] == 0 and r["converged"] and r["f"] <= 1e-24 * float(np.sum(np.abs(c.w)))
