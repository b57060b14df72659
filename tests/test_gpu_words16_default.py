"""The 16-bit window words are the default of the one-pass Stiefel Hessian (Config::words16; stiefel.hip st_hess_traits):
a context created with MI355OPT_WORDS16 unset takes them wherever st_hess_plan allows them -- the matrix has them (at most
32 table values, 0.0 included), its far columns are computed and none is a halo column -- and computes the bits of the
4-byte words (MI355OPT_WORDS16=0), which is what MI355OPT_WORDS16=1 always did.  Which kernel a context's pass takes is
read from the library itself (mi_debug_stiefel_hess_form_of: the plan for THIS matrix on THIS context; FAR = 2 is the
16-bit form).

The grids: 12x10x9, 70x3x5 (plane smaller than a tile) and 9x9x40 (slab thinner than a run) keep every entry inside a
window of two or four chunks (sparse.hip build_window's 90 % rule), so they have no far column to compute and the plan
gives them the loaded-far kernel (FAR = 0) whatever the switch says: on them the three contexts must agree and take
that one kernel.  17x16x5 and 33x9x7 (planes of 272 and 297 rows, outside a one-chunk window; n = 1360 and 2079, no
multiple of a tile) are the small grids on which the default does reach the 16-bit kernel."""
import numpy as np
import pytest

import window_cases as wcs
from optimization_amd import workloads as wl

pytestmark = pytest.mark.gpu

FAR = 6  # index of FAR in the plan's numbers: 0 loaded far columns, 1 computed, 2 computed + 16-bit words
SETTINGS = (("unset", None), ("off", "0"), ("on", "1"))


def _solve(monkeypatch, words16, n, rowptr, col, val, p, X, two_kernel=False, **kw):
    """one fused STPCG solve on a fresh context created under MI355OPT_WORDS16 = words16 (None: unset)"""
    from optimization_amd import capi
    monkeypatch.delenv("MI355OPT_WORDS16", raising=False)
    monkeypatch.delenv("MI355OPT_TWO_KERNEL_STEP", raising=False)
    if words16 is not None:
        monkeypatch.setenv("MI355OPT_WORDS16", words16)
    if two_kernel:  # (one rank only: the multi-rank rehearsal switches keep the three kernels)
        monkeypatch.delenv("MI355OPT_FORCE_SLOT_PATH", raising=False)
        monkeypatch.delenv("MI355OPT_FORCE_UNIFORM_GRID", raising=False)
        monkeypatch.setenv("MI355OPT_TWO_KERNEL_STEP", "1")
    c = capi.Context(0)
    try:
        A = c.csr(n, rowptr, col, val)
        prob = c.stiefel_rq(A, n, p)
        g, H = prob.model(c.upload(X))
        for k in ("stiefel_hess_fused", "cg_pupdate"):
            c.ktime_enable(k, True)
        c.ktime_reset()
        plan = A.stiefel_hess_form(p)
        r = c.stpcg(g, H, **kw)
        return dict(s=r["s"].numpy().copy(), rest=(r["iterations"], r["exit_reason"], r["M_norm"]), plan=plan,
                    window=A.window_info(), wk16=A.format_info()["wk16"],
                    hess=c.ktime_read("stiefel_hess_fused")[0], pupdates=c.ktime_read("cg_pupdate")[0])
    finally:
        c.close()


def _same_bits(a, b):
    return np.array_equal(a["s"].view(np.uint64), b["s"].view(np.uint64)) and a["rest"] == b["rest"]


@pytest.mark.parametrize("p", [1, 2, 3])
@pytest.mark.parametrize("grid,sixteen", [((12, 10, 9), False), ((70, 3, 5), False), ((9, 9, 40), False),
                                          ((17, 16, 5), True), ((33, 9, 7), True)])
def test_default_has_the_bits_of_both_settings_on_laplacian_grids(monkeypatch, grid, sixteen, p):
    """25 STPCG iterations next to the minimiser under MI355OPT_WORDS16 unset, = 0 and = 1, a context each: s, the
    iteration count, the exit reason and |s|_M identical to the bit; the unset context's plan is that of = 1."""
    nx, ny, nz = grid
    n = nx * ny * nz
    rowptr, col, val = wl.laplacian_3d(nx, ny, nz)
    Xb, _ = wl.stiefel_bench_iterate(nx, ny, nz, p, eps=1e-2, seed=3 + p)
    res = {name: _solve(monkeypatch, v, n, rowptr, col, val, p, Xb, Delta=1e3, max_iterations=25, kappa_fgr=1e-10,
                        theta=1.0) for name, v in SETTINGS}
    u, off, on = res["unset"], res["off"], res["on"]
    assert u["rest"][0] > 3 and all(r["hess"] > 0 for r in res.values())   # the solve ran through the one-pass kernel
    assert _same_bits(u, off) and _same_bits(u, on)
    # the matrix is what the docstring says: 16-bit words exist; computed far columns on the last two grids only
    assert u["wk16"] and u["window"][0] > 0 and (u["window"][2] > 0) == sixteen
    assert u["plan"][FAR] == on["plan"][FAR] == (2 if sixteen else 0)
    assert off["plan"][FAR] == (1 if sixteen else 0)
    assert u["plan"] == on["plan"]


@pytest.mark.parametrize("p", [1, 3])
@pytest.mark.parametrize("name", ["two_offset_pure_32", "two_offset_pure_33"])
def test_default_at_the_table_size_where_the_16_bit_words_end(monkeypatch, name, p):
    """32 table values: the words exist and the default takes them; 33: they do not, and the default runs the 4-byte
    words' kernel -- the same bits as = 0 either way."""
    n, rowptr, col, val, e = wcs.case(name)
    X = wcs.near_minimiser(name, p)
    res = {s: _solve(monkeypatch, v, n, rowptr, col, val, p, X, Delta=1e6, max_iterations=25, kappa_fgr=1e-10, theta=1.0)
           for s, v in SETTINGS}
    u, off, on = res["unset"], res["off"], res["on"]
    assert u["rest"][0] > 3 and all(r["hess"] > 0 for r in res.values())
    assert _same_bits(u, off) and _same_bits(u, on)
    assert u["wk16"] == e.wk16 == (name == "two_offset_pure_32") and u["window"][2] == e.pure_D > 0
    assert u["plan"][FAR] == on["plan"][FAR] == (2 if e.wk16 else 1)
    assert off["plan"][FAR] == 1


def test_two_kernel_step_keeps_its_4_byte_words_under_the_default(monkeypatch):
    """MI355OPT_TWO_KERNEL_STEP=1 with MI355OPT_WORDS16 unset: the experiment's Hessian pass exists for 4-byte words
    only, so the context keeps them (FAR = 1), the merged kernel replaces both CG kernels (no cg_pupdate launch), and
    the solve has the bits of the same solve with MI355OPT_WORDS16=0."""
    nx, ny, nz, p = 17, 16, 5, 3
    n = nx * ny * nz
    rowptr, col, val = wl.laplacian_3d(nx, ny, nz)
    Xb, _ = wl.stiefel_bench_iterate(nx, ny, nz, p, eps=1e-2, seed=4)
    kw = dict(Delta=1e3, max_iterations=25, kappa_fgr=1e-10, theta=1.0)
    u = _solve(monkeypatch, None, n, rowptr, col, val, p, Xb, two_kernel=True, **kw)
    off = _solve(monkeypatch, "0", n, rowptr, col, val, p, Xb, two_kernel=True, **kw)
    three = _solve(monkeypatch, None, n, rowptr, col, val, p, Xb, **kw)
    assert u["rest"][0] > 3 and u["hess"] > 0 and off["hess"] > 0
    assert u["pupdates"] == 0 and off["pupdates"] == 0 and three["pupdates"] > 0
    assert u["plan"][FAR] == off["plan"][FAR] == 1 and three["plan"][FAR] == 2
    assert _same_bits(u, off)
