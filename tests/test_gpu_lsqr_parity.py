"""mi_lsqr pass by pass against a long-double restatement of the reference's LSQR (tests/lsqr_reference.py) over the case
table of tests/lsqr_cases.py: every exit rule told apart, the result scalars and what the observer is handed, the
beta == 0 branch, n_x != n_y, tails, the grid cap, windows at odd offsets.

Operator paths.  callback: mi_op_create_callback(_rect) -- the product in numpy on the host for the rectangular shapes,
the device Csr.spmm for the square ones -- which is what runs k_lsqr_u / k_lsqr_v.  csr (square shapes): op_csr(A, 1) and
op_csr(A', 1), the SpMV-with-epilogue path, on three matrices that take its three single-GPU forms:
  few_values  < 256 distinct values: streamed with the packed value table   (format_info()["packed"])
  generic     streamed without one                                          (not packed)
  gather      the plain gather kernel                                        (not packed, NO_SPMM_STREAM for the solve)
mi_debug_csr_format_info reads out `packed` only.  That `generic` streams and `gather` does not rests on the switch alone
(csr_spmv_sub_scaled reads it at launch, and its other criterion, sell_stream_ok, depends on the size only at n = 4097):
no debug read-out tells the two apart.

Tolerance: BASELINE's 1e-10, or 3 x the floor of the case where that is larger (conftest.floor_or) -- the floor being
how far the float64 RESTATEMENT moves from the long-double one under the orders of its sums that lsqr_cases.floor_orders lists; it
never comes from the device run.  Every test prints the measured device error next to the floor."""
import numpy as np
import pytest

import lsqr_cases as lc
import lsqr_reference as ref
from conftest import floor_or

pytestmark = pytest.mark.gpu

LSQR_TOL = 1e-10  # BASELINE.json
RULE_EXITS = (ref.EXIT_S1, ref.EXIT_S2, ref.EXIT_S3, ref.EXIT_S4)


@pytest.fixture(scope="module")
def ctx():
    from optimization_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def _paths():
    out = []
    for c in lc.CASES:
        out.append((c.id, "callback"))
        if lc.is_square(c):
            out.append((c.id, "csr"))
    return out


_device_matrices = {}


def _csr_pair(ctx, case_id):
    """(A, A') of the case on the device, kept until another case asks: the two operator paths of a case, which run
    one after the other, share one upload"""
    if case_id not in _device_matrices:
        A = lc.inputs(case_id)[0]
        At = A.T.tocsr()
        At.sort_indices()
        _device_matrices.clear()  # (one case at a time: the largest pair is 2 x 100 MB)
        # 2 I has one value and would be packed in every family: the table is switched off where the family has none
        unpacked = lc.BY_ID[case_id].kind == "beta0" and lc.BY_ID[case_id].matrix != "few_values"
        if unpacked:
            ctx.set_option("NO_PACKED", 1)
        try:
            _device_matrices[case_id] = tuple(ctx.csr(M.shape[0], M.indptr, M.indices, M.data) for M in (A, At))
        finally:
            if unpacked:
                ctx.set_option("NO_PACKED", 0)
    return _device_matrices[case_id]


def _operators(ctx, case, path):
    A = lc.inputs(case.id)[0]
    if path == "csr":
        dA, dAt = _csr_pair(ctx, case.id)
        packed = dA.format_info()["packed"], dAt.format_info()["packed"]
        assert packed == ((True, True) if case.matrix == "few_values" else (False, False)), packed
        return ctx.op_csr(dA, 1), ctx.op_csr(dAt, 1)
    if lc.is_square(case):
        dA, dAt = _csr_pair(ctx, case.id)
        ops = [ctx.op_callback(case.nx, (lambda M: lambda vin, vout: M.spmm(1, vin, vout))(M)) for M in (dA, dAt)]
        ops[0].n_in = case.nx
        return ops
    At = A.T.tocsr()
    return (ctx.op_callback_rect(case.nx, case.ny, lambda vin, vout: vout.set(A @ vin.numpy())),
            ctx.op_callback_rect(case.ny, case.nx, lambda vin, vout: vout.set(At @ vin.numpy())))


class _Worst:
    def __init__(self):
        self.e = 0.0

    def rel(self, what, got, want, tol):
        want = np.longdouble(want)
        if want == 0:
            assert got == 0, (what, got)
            return
        e = float(abs(np.longdouble(got) - want) / abs(want))
        self.e = max(self.e, e)
        assert e <= tol, f"{what}: {got!r} against {float(want)!r}, {e:.2e} > {tol:.1e}"

    def vec(self, what, got, want, tol):
        scale = np.abs(want).max()
        if scale == 0:
            assert not got.any(), what
            return
        e = float(np.abs(got.astype(np.longdouble) - want).max() / scale)
        self.e = max(self.e, e)
        assert e <= tol, f"{what}: max-norm {e:.2e} > {tol:.1e}"

    def scalars(self, what, got, want, tol):
        """got, want: mappings with xnorm, rbar_norm, Arnorm, Anorm, Acond"""
        for key in ("xnorm", "rbar_norm", "Anorm", "Acond"):
            self.rel(f"{what} {key}", got[key], want[key], tol)
        # |A' r| is legitimately rounding noise at an S2 exit: in units of |A| |r|
        scale = np.longdouble(want["Anorm"]) * np.longdouble(want["rbar_norm"])
        if scale == 0:
            assert got["Arnorm"] == 0, (what, got["Arnorm"])
        else:
            e = float(abs(np.longdouble(got["Arnorm"]) - want["Arnorm"]) / scale)
            self.e = max(self.e, e)
            assert e <= tol, f"{what} Arnorm: {e:.2e} of Anorm rbar_norm > {tol:.1e}"


def _check_result(case, r, x, e, kw, tol, worst, what):
    assert (r["exit_reason"], r["iterations"]) == (e["exit_reason"], e["iterations"]), \
        f"{what}: exit {r['exit_reason']} after {r['iterations']}, restatement: exit {e['exit_reason']} after {e['iterations']}"
    worst.vec(f"{what} x", x, e["x"], tol)
    worst.scalars(what, r, e, tol)
    passes = e["iterations"] + (e["exit_reason"] in RULE_EXITS)
    assert r["operator_applications"] >= 1 + 2 * passes
    if case.kind == "s4":
        assert r["xnorm"] == kw["Delta"]  # by assignment (:793): bitwise
        worst.rel(f"{what} |x|", np.sqrt(np.sum(x.astype(np.longdouble) ** 2)), kw["Delta"], tol)
    if case.kind == "beta0":
        assert r["iterations"] == 0 and r["exit_reason"] == ref.EXIT_S1 and r["Anorm"] == 0 and r["rbar_norm"] == 0
        assert np.abs(x[:min(case.ny, case.nx)] - 0.5).max() <= tol and not x[min(case.ny, case.nx):].any()


def _solve_and_check(ctx, case, path, b, x_out=None):
    """the un-observed and (where the context offers it) the observed solve of the case on one operator path against the
    long-double restatement; returns (worst device error, floor, tolerance)"""
    _, _, kw = lc.inputs(case.id)
    e = lc.expected(case.id)
    fl, _ = lc.floor(case.id)
    tol = floor_or(LSQR_TOL, fl)
    worst = _Worst()
    gather = path == "csr" and case.matrix == "gather"
    A, At = _operators(ctx, case, path)
    if gather:
        ctx.set_option("NO_SPMM_STREAM", 1)
    try:
        r = ctx.lsqr(A, At, b, x_out=x_out, **kw)
        _check_result(case, r, r["x"].numpy(), e, kw, tol, worst, "result")
        if ctx.lsqr_observer_available()[0]:
            last = e["iterations"] - 1
            seen, xs = [], {}

            def observer(k, x, xnorm, rbar_norm, Arnorm, Anorm, Acond):
                seen.append(dict(k=k, xnorm=xnorm, rbar_norm=rbar_norm, Arnorm=Arnorm, Anorm=Anorm, Acond=Acond))
                if k in (0, last):
                    xs[k] = x.numpy()
                return False
            ro = ctx.lsqr(A, At, b, x_out=x_out, observer=observer, **kw)
            _check_result(case, ro, ro["x"].numpy(), e, kw, tol, worst, "observed result")
            assert [s["k"] for s in seen] == list(range(e["iterations"]))
            for s in seen:
                worst.scalars(f"observer at pass {s['k']}", s, e["trace"][s["k"]], tol)
            assert sorted(xs) == sorted({0, last} if last >= 0 else set())
            for k, xk in xs.items():
                worst.vec(f"observed x at pass {k}", xk, e["iterates"][k], tol)
    finally:
        if gather:
            ctx.set_option("NO_SPMM_STREAM", 0)
    print(f"{case.id} [{path}]: device error {worst.e:.2e}, floor {fl:.2e}, tolerance {tol:.1e}")
    return worst.e, fl, tol


@pytest.mark.parametrize("case_id,path", _paths())
def test_lsqr_matches_the_restatement(ctx, case_id, path):
    case = lc.BY_ID[case_id]
    _solve_and_check(ctx, case, path, ctx.upload(lc.inputs(case_id)[1]))


@pytest.mark.parametrize("path", ["callback", "csr"])
def test_lsqr_on_windows_at_an_odd_offset(ctx, path):
    """b and x_out as views [1, 1 + n) of longer vectors: the double2 walks of k_lsqr_xw are 16-byte aligned on v and w
    and 8-byte aligned on x (mi_vec_view documents that as served); nothing outside the windows is written"""
    case = lc.VIEW_CASE
    n = case.nx
    b = lc.inputs(case.id)[1]
    bbase = ctx.upload(np.concatenate([[7.5], b, [-7.5]]))
    xbase = ctx.upload(np.full(n + 2, 3.25))
    _solve_and_check(ctx, case, path, bbase.view(1, n), x_out=xbase.view(1, n))
    xb, bb = xbase.numpy(), bbase.numpy()
    assert (xb[0], xb[-1]) == (3.25, 3.25)
    assert (bb[0], bb[-1]) == (7.5, -7.5) and np.array_equal(bb[1:-1], b)
    assert np.abs(xb[1:-1].astype(np.longdouble) - lc.expected(case.id)["x"]).max() <= \
        floor_or(LSQR_TOL, lc.floor(case.id)[0]) * np.abs(lc.expected(case.id)["x"]).max()
