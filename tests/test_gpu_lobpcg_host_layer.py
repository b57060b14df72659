"""The owners of lobpcg.hip's host half on their success path: after one warm-up call, five more identical calls of
every public entry point of that file leave the context's pool as large as it was (mi_ctx_pool_bytes) -- whatever a
call takes from the pool goes back to it.  Shapes: m = 4100 (the one-pass kernels) and m = 4099 (their fall-backs, which
hold assembled copies), k = 24; a matrix with and without the window form."""
import ctypes as C

import numpy as np
import pytest

from optimization_amd import workloads as wl

pytestmark = pytest.mark.gpu

K, NX = 24, 8


def _pool_bytes(ctx):
    n = C.c_size_t(0)
    assert ctx.L.mi_ctx_pool_bytes(ctx.h, C.byref(n)) == 0
    return n.value


def _steady(ctx, call):
    call()
    before = _pool_bytes(ctx)
    for _ in range(5):
        call()
    assert _pool_bytes(ctx) == before


def _blocks(panel, m):
    """[X | W(:, 3:) | P(:, 3:)] of a panel of 3 NX columns: three column blocks that are not adjacent"""
    return [(panel.view(0, m * NX), NX), (panel.view((NX + 3) * m, (NX - 3) * m), NX - 3),
            (panel.view((2 * NX + 3) * m, (NX - 3) * m), NX - 3)]


PANEL_CALLS = ("gram", "gram_same", "gram_split", "gram_pair", "gram_pair_sym", "gram_pair_sym_blocks",
               "gram_pair_sym_tblocks", "gram_pair_gen_blocks", "update", "update2", "update2_blocks", "update_48",
               "residual", "rowscale")


@pytest.mark.parametrize("m", [4100, 4099])
@pytest.mark.parametrize("name", PANEL_CALLS)
def test_panel_entry_points_leave_the_pool_as_it_was(ctx, name, m):
    rng = np.random.default_rng(m)
    S, T, B = (ctx.upload(rng.normal(size=m * K)) for _ in range(3))
    T1, T2 = ctx.upload(rng.normal(size=m * 8)), ctx.upload(rng.normal(size=m * (K - 8)))
    d = ctx.upload(rng.uniform(0.5, 2.0, size=m))
    sb, tb, bb = _blocks(S, m), _blocks(T, m), _blocks(B, m)
    ns = sum(c for _, c in sb)
    Cm, C48 = rng.normal(size=(K, K)), rng.normal(size=(K, 48))
    calls = {
        "gram": lambda: ctx.lobpcg_gram(m, S, K, T, K),
        "gram_same": lambda: ctx.lobpcg_gram(m, S, K, S, K),
        "gram_split": lambda: ctx.lobpcg_gram_split(m, S, K, T1, 8, T2),
        "gram_pair": lambda: ctx.lobpcg_gram_pair(m, S, K, T1, 8, T2, S, K, None),
        "gram_pair_sym": lambda: ctx.lobpcg_gram_pair_sym(m, S, K, T1, 8, T2),
        "gram_pair_sym_blocks": lambda: ctx.lobpcg_gram_pair_sym_blocks(m, sb, T, ns, None),
        "gram_pair_sym_tblocks": lambda: ctx.lobpcg_gram_pair_sym_tblocks(m, sb, tb),
        "gram_pair_gen_blocks": lambda: ctx.lobpcg_gram_pair_gen_blocks(m, sb, tb, bb),
        "update": lambda: ctx.lobpcg_update(m, S, K, Cm),
        "update2": lambda: ctx.lobpcg_update2(m, S, K, Cm, 8),
        "update2_blocks": lambda: ctx.lobpcg_update2_blocks(m, sb, Cm[:ns], 8),
        "update_48": lambda: ctx.lobpcg_update(m, S, K, C48),      # the matrix-pipe form (6 steps)
        "residual": lambda: ctx.lobpcg_residual(m, K, T, S, S, np.linspace(0.5, 2.0, K)),
        "rowscale": lambda: ctx.panel_rowscale(m, K, d, S),
    }
    _steady(ctx, calls[name])


@pytest.mark.parametrize("weights", ["stencil", "random"])
@pytest.mark.parametrize("name", ["spmm", "spmm_blocks", "spmm_residual"])
def test_panel_product_entry_points_leave_the_pool_as_it_was(ctx, name, weights):
    gx, gy, gz = 41, 10, 10
    m = gx * gy * gz
    rowptr, col, val = wl.laplacian_3d(gx, gy, gz)
    if weights == "random":   # real-valued weights: no window form, the gather kernels and the assembled copy
        val = val * np.random.default_rng(5).uniform(0.5, 1.5, size=val.shape)
    A = ctx.csr(m, rowptr, col, val)
    X = ctx.upload(np.random.default_rng(m).normal(size=m * K))
    xb = _blocks(X, m)
    calls = {
        "spmm": lambda: A.spmm_colmajor(K, X),
        "spmm_blocks": lambda: A.spmm_colmajor_blocks(xb),
        "spmm_residual": lambda: A.spmm_colmajor_residual(K, X, np.linspace(0.5, 2.0, K)),
    }
    _steady(ctx, calls[name])
