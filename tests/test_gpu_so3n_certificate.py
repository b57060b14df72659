"""GPU tests of the SO(3)^N global-optimality certificate (k_so3_cert_diag, k_so3_cert_panel, mi_so3n_certificate /
mi_so3n_cert_apply[_blocks], MI355::RotationAveraging::certify) against tests/so3n_certificate_reference.py.

Operator bar: |Z - Z_ref| on rows 3i .. 3i+2 of column c <= 1e-12 (sum_inc |w| + |degw_i|) max |X_c| over node i and its
neighbours, against the longdouble restatement (a row is at most 3 (deg + 1) products plus the rounding of C_i;
test_cpu_so3n_certificate.py holds float64 numpy inside it up to degree 1499).  Bit contracts are exact."""
import contextlib
import functools

import numpy as np
import pytest

import so3_cases as sc
import so3n_certificate_reference as cr

pytestmark = pytest.mark.gpu

WIDTHS = (1, 3, 8, 9, 24)
KMAX = max(WIDTHS)
# (case, form): every graph and weight pattern in the default form, every creation switch on a multigraph with the
# rotations Shepperd's branch turns on and on the twelve-decade hub, and the 9-component form a non-rotation forces
PARITY = [(n, "default") for n in ("tiny_1", "tiny_2", "isolated_1500", "hub_first_linspace", "hub_last_spread",
                                   "hub_first_some_zero", "multigraph_linspace", "multigraph_negative",
                                   "ring_chords_1024_node_zero", "ring_chords_2049_some_zero", "nonrot_perturbed",
                                   "winding_130")] + \
         [(n, f) for n in ("multigraph_linspace", "hub_last_spread") for f in ("no_quat", "no_rquat", "no_quat_no_rquat")]


@functools.lru_cache(maxsize=None)
def _problem(name):
    """(N, ei, ej, Rt, w, R) of a tests/so3_cases.py case or of a cycle at its winding"""
    if name.startswith("winding_"):
        return cr.winding(int(name.split("_")[1]))
    c = sc.case(name)
    return c.N, c.ei, c.ej, c.Rt, c.w, c.R


@functools.lru_cache(maxsize=None)
def _reference(name):
    """the longdouble restatement at the case's point, a 3N x 24 panel, S X and the bar, once per case"""
    N, ei, ej, Rt, w, R = _problem(name)
    ref = cr.CertRef(N, ei, ej, Rt, w, R, cr.LD)
    X = np.random.Generator(np.random.PCG64(N + 5)).normal(size=(3 * N, KMAX))
    X[:, 1] *= 1e6                                        # (columns of different size: the bar is per column)
    X[:, 2] *= 1e-6
    Z = ref.apply(X)
    for a in (X, Z):
        a.setflags(write=False)
    return ref, X, Z, ref.row_bar(X)


@contextlib.contextmanager
def _ctx_of(form):
    from optimization_amd import capi
    c = capi.Context(0)
    try:
        for k, v in sc.FORMS[form].items():
            c.set_option(k, v)
        yield c
    finally:
        c.close()


def _panel(Zvec, m, k):
    return Zvec.numpy()[:m * k].reshape(k, m).T           # column-major m x k


def _up(ctx, X):
    return ctx.upload(np.ascontiguousarray(np.asarray(X, dtype=np.float64).T).ravel())


@pytest.mark.parametrize("name,form", PARITY)
def test_certificate_operator_parity_symmetry_and_info(name, form):
    N, ei, ej, Rt, w, R = _problem(name)
    ref, X, Zref, bar = _reference(name)
    m = 3 * N
    with _ctx_of(form) as ctx:
        prob = ctx.so3n(N, ei, ej, Rt, w)
        info = prob.info()
        if form == "default":
            assert info["sinc_quat"] == (not name.startswith("nonrot")) and info["gather_quat"]
        else:
            assert info["sinc_quat"] == ("no_quat" not in form.replace("no_rquat", "")) and \
                info["gather_quat"] == ("no_rquat" not in form)
        Rv = ctx.upload(np.asarray(R).ravel())
        cert, inf = prob.certificate(Rv)
        # info: f with the bits of mi_so3n_objective, |skew Q|_F and sum tr C against longdouble
        assert inf["f"] == prob.objective(Rv)
        scale = float(2 * ref.abs_degw().sum()) or 1.0
        print(name, form, "stationarity", inf["stationarity"], float(ref.stationarity()), "trace_C", inf["trace_C"])
        assert abs(inf["stationarity"] - float(ref.stationarity())) <= 1e-12 * scale
        assert abs(inf["trace_C"] - float(ref.trace_C())) <= 1e-12 * scale
        Yd = _panel(cert.null_panel(), m, 3)
        assert np.array_equal(Yd, ref.Y().astype(np.float64))
        Z24 = None
        for k in WIDTHS:
            Z = _panel(cert.apply(k, _up(ctx, X[:, :k])), m, k)
            err = np.abs((Z.astype(cr.LD) - Zref[:, :k]).astype(np.float64))
            print(name, form, "k", k, "worst error / bar", float((err / np.maximum(bar[:, :k], 1e-300)).max()))
            assert np.all(err <= bar[:, :k]), (name, form, k)
            if k == KMAX:
                Z24 = Z
            else:
                Zk = Z
        # bit contract: a column is the same whatever the width and the pass that produced it
        assert np.array_equal(Zk, _panel(cert.apply(KMAX, _up(ctx, X)), m, KMAX)[:, :Zk.shape[1]])
        for c in (0, 7, 8, 23):
            assert np.array_equal(_panel(cert.apply(1, _up(ctx, X[:, c:c + 1])), m, 1)[:, 0], Z24[:, c]), c
        # symmetry: X' (S X2) == (S X)' X2 inside the same bar (summed over the rows)
        X2 = np.random.Generator(np.random.PCG64(3)).normal(size=(m, 3))
        Z2 = _panel(cert.apply(3, _up(ctx, X2)), m, 3)
        A, B = X[:, :3].T @ Z2, Z24[:, :3].T @ X2
        bar2 = ref.row_bar(X2)
        tol = np.abs(X[:, :3]).T @ bar2 + bar[:, :3].T @ np.abs(X2)
        assert np.all(np.abs(A - B) <= tol + 1e-15 * (np.abs(X[:, :3]).T @ np.abs(Z2)))
        # S Y: its norm is the stationarity defect
        SY = _panel(cert.apply(3, cert.null_panel()), m, 3)
        assert abs(np.linalg.norm(SY) - inf["stationarity"]) <= 1e-12 * scale


@pytest.mark.parametrize("name", ("multigraph_linspace", "winding_130", "tiny_2"))
def test_three_block_panel_has_the_bits_of_the_assembled_one(ctx, name):
    N, ei, ej, Rt, w, R = _problem(name)
    _, X, _, _ = _reference(name)
    m = 3 * N
    prob = ctx.so3n(N, ei, ej, Rt, w)
    cert, _ = prob.certificate(ctx.upload(np.asarray(R).ravel()))
    Z = _panel(cert.apply(KMAX, _up(ctx, X)), m, KMAX)
    # blocks cut from two different panels, not adjacent and not in storage order: columns [0, 5) | [5, 14) | [14, 24)
    P1, P2 = _up(ctx, X[:, 14:24]), _up(ctx, np.hstack([X[:, 5:14], X[:, 0:5]]))
    blocks = [(P2.view(9 * m, 5 * m), 5), (P2.view(0, 9 * m), 9), (P1, 10)]
    assert np.array_equal(_panel(cert.apply_blocks(blocks), m, KMAX), Z)
    assert np.array_equal(_panel(cert.apply_blocks(blocks[:2]), m, 14), Z[:, :14])
    assert np.array_equal(_panel(cert.apply_blocks(blocks[1:2]), m, 9), Z[:, 5:14])


def test_certificate_is_bound_to_a_copy_of_its_point(ctx):
    """trial steps, model calls, an Armijo trial and an in-place overwrite of R leave the certificate's product as it is"""
    c = sc.case("ring_chords_1025_spread")
    _, X, _, _ = _reference("ring_chords_1025_spread")
    m = 3 * c.N
    prob = ctx.so3n(c.N, c.ei, c.ej, c.Rt, c.w)
    R = ctx.upload(c.R.ravel())
    cert, inf = prob.certificate(R)
    Xd = _up(ctx, X[:, :9])
    before = cert.apply(9, Xd).numpy()
    Y0 = cert.null_panel().numpy()
    g, H, P = prob.model(R)
    h = g.scaled(-1e-3)
    Rt1, _ = prob.trial(R, h, g)
    g2, _, _ = prob.model(Rt1)
    prob.armijo_trial(Rt1, g2, 1e-3)
    other = sc.case("ring_chords_1025_spread")._replace()  # (same graph)
    R.set(np.roll(other.R, 7, axis=0).ravel())             # R overwritten in place with other rotations
    prob.model(R)
    assert np.array_equal(cert.apply(9, Xd).numpy(), before)
    assert np.array_equal(cert.null_panel().numpy(), Y0)
    # ... and the next call rebinds the same handle to the new point
    cert2, inf2 = prob.certificate(R)
    assert cert2.h.value == cert.h.value and inf2["f"] != inf["f"]
    assert not np.array_equal(cert.apply(9, Xd).numpy(), before)


def test_certificate_at_a_noise_free_ground_truth_is_stationary(ctx):
    N, ei, ej, Rt, w, Rgt = cr.ring_with_chords(70, 40, 0.0, 1)
    prob = ctx.so3n(N, ei, ej, Rt, w)
    cert, inf = prob.certificate(ctx.upload(Rgt.ravel()))
    scale = 2 * float(np.abs(w).sum()) * 2
    SY = cert.apply(3, cert.null_panel()).numpy()
    print("f", inf["f"], "stationarity", inf["stationarity"], "|SY|", np.linalg.norm(SY))
    assert inf["stationarity"] <= 1e-12 * scale and np.linalg.norm(SY) <= 1e-12 * scale and inf["f"] <= 1e-24 * scale


def test_no_edges_and_bad_arguments(ctx):
    c = sc.case("tiny_1")
    prob = ctx.so3n(c.N, c.ei, c.ej, c.Rt, c.w)
    cert, inf = prob.certificate(ctx.upload(c.R.ravel()))
    assert inf["f"] == 0.0 and inf["stationarity"] == 0.0
    assert np.all(cert.apply(2, ctx.upload(np.arange(6.0))).numpy() == 0.0)
    from optimization_amd import capi
    X = ctx.upload(np.arange(6.0))
    with pytest.raises(capi.MiError):
        cert.apply(2, X, X)                                # aliasing
    with pytest.raises(capi.MiError):
        cert.apply(3, X)                                   # X too small
    with pytest.raises(capi.MiError):
        cert.apply(0, X)


# ---- certify through the template layer ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness():
    from harness_certify_so3n_py import CertifySo3nHarness
    return CertifySo3nHarness()


@pytest.mark.parametrize("N", (8, 130))
def test_certify_refuses_the_winding(harness, N):
    n, ei, ej, Rt, w, R = cr.winding(N)
    tau = 1e-8
    S2 = np.abs(np.linalg.eigvalsh(cr.CertRef(n, ei, ej, Rt, w, R).dense())).max()
    r = harness.certify(n, ei, ej, Rt, w, R, tau=tau, max_iterations=4000)
    assert r["rc"] == 0, r["err"]
    print("winding", N, {k: r[k] for k in ("lambda_min", "lambda_min_safe", "f", "lower_bound", "iterations", "converged",
                                             "eta", "norm_estimate", "stationarity")}, "closed form", cr.winding_lambda_min(N))
    assert r["converged"] and not r["certified"]
    assert abs(r["lambda_min"] - cr.winding_lambda_min(N)) <= 2 * tau * S2 + 1e-12 * S2
    assert r["lower_bound"] <= 0
    assert abs(r["f"] - cr.winding_f(N)) <= 1e-12 * N
    v = r["eigenvector"]
    Sv = cr.CertRef(n, ei, ej, Rt, w, R).apply(v[:, None])[:, 0]
    assert np.linalg.norm(Sv - r["lambda_min"] * v) <= 2 * tau * S2 * np.linalg.norm(v) * 1.01


def test_certify_tagged_plain_and_block_forms_agree(harness):
    n, ei, ej, Rt, w, R = cr.winding(8)
    runs = [harness.certify(n, ei, ej, Rt, w, R, op_mode=mode) for mode in (0, 1, 2)]
    for r in runs:
        assert r["rc"] == 0, r["err"]
    assert runs[0]["iterations"] == runs[1]["iterations"] == runs[2]["iterations"] > 1
    assert runs[0]["lambda_min"] == runs[1]["lambda_min"] == runs[2]["lambda_min"]
    S2 = 4.0
    assert 0 <= runs[2]["blocks_residual"] <= 2e-8 * S2 * np.linalg.norm(runs[2]["eigenvector"]) * 1.01


def test_certify_accepts_a_noise_free_ground_truth(harness):
    N, ei, ej, Rt, w, Rgt = cr.ring_with_chords(70, 40, 0.0, 1)
    r = harness.certify(N, ei, ej, Rt, w, Rgt)
    assert r["rc"] == 0, r["err"]
    print({k: r[k] for k in ("lambda_min", "lambda_min_safe", "eta", "iterations", "stationarity", "lower_bound", "f")})
    assert r["certified"] and r["converged"] and abs(r["lambda_min"]) <= r["eta"]
    assert r["lower_bound"] <= r["f"] + 1e-300 and r["lower_bound"] >= -1.5 * N * r["eta"]


def test_certify_accepts_what_tnt_reaches_at_noise_0_2(harness):
    N, ei, ej, Rt, w, Rgt = cr.ring_with_chords(70, 40, 0.2, 3)
    r = harness.certify(N, ei, ej, Rt, w, Rgt, run_tnt=True, tnt_gradient_tolerance=1e-9)
    assert r["rc"] == 0, r["err"]
    print({k: r[k] for k in ("lambda_min", "lambda_min_safe", "eta", "iterations", "stationarity", "lower_bound", "f",
                             "tnt_gradnorm", "tnt_iterations", "tnt_status")})
    assert r["tnt_gradnorm"] < 1e-9
    # numpy on the point the device reached: three eigenvalues at 0, the fourth far from it
    ev = np.linalg.eigvalsh(cr.CertRef(N, ei, ej, Rt, w, r["R"]).dense())
    assert np.abs(ev[:3]).max() <= 1e-8 and ev[3] > 0.05
    assert r["certified"] and r["converged"] and abs(r["lambda_min"]) <= r["eta"]
    assert r["lower_bound"] <= r["f"] and r["f"] - r["lower_bound"] <= 1.5 * N * 2 * r["eta"]


def test_certify_without_edges_needs_no_solve(harness):
    c = sc.case("tiny_1")
    r = harness.certify(c.N, c.ei, c.ej, c.Rt, c.w, c.R)
    assert r["rc"] == 0, r["err"]
    assert r["certified"] and r["lambda_min"] == 0.0 and r["iterations"] == 0
