"""The launch plan of the Stiefel one-pass Hessian (stiefel.hip st_hess_plan through mi_debug_stiefel_hess_form): which
of the five kernel forms runs, with which template selectors.  Host-only.

The expected table below is the ladder of `if`s the plan replaced, written out once more by hand; it does not call
the library."""
import ctypes as C
import itertools

from optimization_amd import capi

PLAIN, WINDOW, WIDEWIN, WIDE, WIDEQ = range(5)
WIN_BLOCK, WIDE_BLOCK, BLOCK = 256, 256, 1024   # kWinBlock, kWideBlock, kBlock
WIN_WAVES, FAR_ROWS = 4, 4 * 2 * 64              # kWinWaves, kWinFarRows


def expected(p, gc, T, S):
    """(form, FROM_SLOTS, HALO, RECUR, PK, HW, FAR, TWOK, block, lds bytes, run table, exchange, Gram reduction), or
    None where the library answers with an internal error"""
    pk, wk, wk16, chunks, head, pure, stride, halo, row_sharded = T
    no_window, no_far, words16, wide_quad, wide_window, no_bounds, uniform, slot_mode, twok_r = S
    fard = 0 < pure < 2 ** 31 and not no_far
    hw = 7 if head <= 7 else 8
    wide_window_form = bool((p <= 7 and not wide_quad > 0) if wide_window < 0 else wide_window != 0) and pk and wk and \
        0 < chunks <= 2 and not halo and not uniform and not no_window and not row_sharded
    if p > 4 or (p == 4 and gc == -1 and wide_window_form):
        if gc >= 0:
            return None
        if wide_window_form:
            lds = ((2 * WIN_WAVES + 2 * chunks) * 64 + 1 + FAR_ROWS) * (9 if p == 8 else p) * 8
            return (WIDEWIN, 0, 0, 1, 1, hw, int(fard), 0, WIN_BLOCK, lds, 1, 0, 0)
        quad = p == 8 if wide_quad < 0 else wide_quad != 0
        table = not uniform and stride != 0 and not no_bounds
        return (WIDEQ if quad else WIDE, 0, halo, 1, pk, 0, 0, 0, WIDE_BLOCK, 0, int(table), 1, 0)
    recur = gc < 0
    sharded = slot_mode and not recur
    wc = 0 if (no_window or p > 3 or not wk) else chunks
    win = recur and wc > 0
    w16 = fard and not halo and wk16 and words16
    tail = (WIN_BLOCK if win else BLOCK, 0, int(win and not uniform), 1, int(not recur))
    form = WINDOW if win else PLAIN
    if gc == -2:
        if not (win and fard and not halo and not w16 and p == 3 and twok_r):
            return None
        return (form, 0, 0, 1, 1, hw, 1, 1) + tail
    if win and w16:
        return (form, 0, 0, 1, 1, hw, 2, 0) + tail
    if win and fard and halo:
        return (form, 0, 1, 1, 1, hw, 1, 0) + tail
    if win and fard:
        return (form, 0, 0, 1, 1, hw, 1, 0) + tail
    if win:
        return (form, 0, halo, 1, 1, hw, 0, 0) + tail
    if recur:
        return (form, 0, halo, 1, pk, 0, 0, 0) + tail
    return (form, int(sharded), halo, 0, pk, 0, 0, 0) + tail


def parent_twok(p, T, S):
    """mi_dirgram::twok as mi_stiefel_rq_model spelled it out before the plan existed"""
    pk, wk, wk16, chunks, head, pure, stride, halo, row_sharded = T
    no_window, no_far, words16, wide_quad, wide_window, no_bounds, uniform, slot_mode, twok_r = S
    return bool(p == 3 and not halo and wk and chunks > 0 and pure > 0 and pure < 2 ** 31 and not no_window and
                not no_far and not uniform and not (wk16 and words16))


def test_plan_reproduces_the_ladder_on_every_combination():
    form = capi.stiefel_hess_form_fn()
    tr, sw, out = (C.c_size_t * 9)(), (C.c_int * 9)(), (C.c_int * 14)()
    forms, errors, n = set(), 0, 0
    for i, (pk, chunks, head, pure, halo, words16, wide_quad, wide_window, no_window, no_far, uniform, slot_mode) in \
            enumerate(itertools.product((0, 1), (0, 1, 2, 3), (7, 8), (0, 10_000), (0, 1), (0, 1), (-1, 0, 1),
                                        (-1, 0, 1), (0, 1), (0, 1), (0, 1), (0, 1))):
        # facts that ride along: window words with the window, their 16-bit form and the far stride on every second /
        # third matrix, a pure stride beyond 32 bits now and then, a row shard with and without a halo buffer
        wk = int(chunks > 0)
        if pure and i % 7 == 3:
            pure = 2 ** 31
        T = (pk, wk, int(wk and i % 2 == 0), chunks, head, pure, pure or (300 if i % 3 == 0 else 0), halo,
             int(halo or i % 5 == 0))
        S = (no_window, no_far, words16, wide_quad, wide_window, int(i % 4 == 1), uniform, slot_mode, int(i % 3 != 1))
        tr[:], sw[:] = T, S
        for p in range(1, 9):
            for gc in (-2, -1, 5):
                st = form(p, gc, tr, sw, out)
                want = expected(p, gc, T, S)
                got = tuple(out[:13]) if st == capi.MI_OK else None
                assert got == (None if want is None else tuple(int(v) for v in want)), (p, gc, T, S, got, want)
                assert st in (capi.MI_OK, 1), st  # (1: MI_ERR_INVALID_ARGUMENT, the code of an internal MI_REQUIRE)
                assert bool(out[13]) == parent_twok(p, T, S), (p, gc, T, S)
                errors += want is None
                n += 1
                if want is not None:
                    forms.add(want[:8])
    # the enumeration reaches every form, with and without its variants, and both kinds of internal error
    assert {f[0] for f in forms} == {PLAIN, WINDOW, WIDEWIN, WIDE, WIDEQ}
    assert {f[6] for f in forms if f[0] == WINDOW} == {0, 1, 2} and any(f[7] for f in forms)
    assert any(f[1] for f in forms) and any(f[0] == WINDOW and f[2] and f[6] == 1 for f in forms)
    assert 0 < errors < n


def test_internal_error_combinations_are_errors_not_forms():
    T = (1, 1, 0, 1, 7, 10_000, 10_000, 0, 0)
    S = [0, 0, 0, -1, -1, 0, 0, 0, 1]
    for p in (5, 6, 7, 8):  # rows wider than 4 doubles exist in the recurrence form only
        assert capi.stiefel_hess_form(p, 5, T, S) is None
        assert capi.stiefel_hess_form(p, -1, T, S) is not None
    assert capi.stiefel_hess_form(8, 5, T, S) is None and b"recurrence form only" in capi.load().mi_last_error()
    # the two-kernel step: p = 3, window form with computed far columns, the residual set -- and nothing else
    assert capi.stiefel_hess_form(3, -2, T, S)[:8] == [WINDOW, 0, 0, 1, 1, 7, 1, 1]
    assert capi.stiefel_hess_form(2, -2, T, S) is None
    assert capi.stiefel_hess_form(3, -2, T, S[:8] + [0]) is None
    assert capi.stiefel_hess_form(3, -2, T[:5] + (0, 0) + T[7:], S) is None       # far columns not computed
    assert capi.stiefel_hess_form(3, -2, T, [1] + S[1:]) is None                   # NO_WINDOW
    assert capi.stiefel_hess_form(3, -2, (1, 1, 1) + T[3:], S[:2] + [1] + S[3:]) is None  # 16-bit words
    assert capi.stiefel_hess_form(0, -1, T, S) is None and capi.stiefel_hess_form(9, -1, T, S) is None


def test_bench_matrix_takes_the_forms_the_profiles_name():
    """the 3-D Laplacian of the bench (packed, window of one chunk, 7 entries per row, pure far stride): p = 3 runs
    k_st_hess_fused<3, false, false, true, true, 7, 1>, p = 4 ... 7 the wide window form, p = 8 the quad layout"""
    T = (1, 1, 1, 1, 7, 10_000, 10_000, 0, 0)
    S = (0, 0, 0, -1, -1, 0, 0, 0, 0)
    assert capi.stiefel_hess_form(3, -1, T, S)[:8] == [WINDOW, 0, 0, 1, 1, 7, 1, 0]
    for p in (4, 5, 6, 7):
        assert capi.stiefel_hess_form(p, -1, T, S)[:8] == [WIDEWIN, 0, 0, 1, 1, 7, 1, 0]
    assert capi.stiefel_hess_form(8, -1, T, S)[:8] == [WIDEQ, 0, 0, 1, 1, 0, 0, 0]
    assert capi.stiefel_hess_form(4, 5, T, S)[:8] == [PLAIN, 0, 0, 0, 1, 0, 0, 0]
