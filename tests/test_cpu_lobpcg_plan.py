"""The plans of the LOBPCG host layer (optimization_amd/csrc/lobpcg_plan.h through the mi_debug_lobpcg_* entries): which
Gram kernel runs with which template selectors and geometry, how the Ritz update is cut into steps or chunks and how its
coefficient matrix is packed, the grid of the plane-sweep product.  Host-only.

The expected values below are the ladders the launch code held before the plans existed, written out once more by
hand; they do not come from calling the library."""
import ctypes as C
import itertools

import numpy as np
import pytest

from optimization_amd import capi

GDH = 1                                   # kGdH: 16-row blocks per pipeline step of k_gram_direct
GRAM_ROWS, GRAM_LD, GRAM_WAVES = 32, 34, 8
SW_ROWS, MAX_ROWS = 512, 1024             # kSwRows, kMaxRows

MS = (1, 15, 16, 31, 1000, 1001, 1004, 100_004)
KS = (1, 15, 16, 17, 48, 49, 80, 81, 96)


def pad16(k):
    return (k + 15) // 16 * 16


def ladder(v, top):
    """switch (v) { case 1: .. case top - 1: ; default: top }"""
    return v if 1 <= v < top else top


def parent_gram(m, ka, kb, same_panel, split, al16, al32, num_cu):
    """gram_impl as it stood: None where it refused ("split panels need the direct Gram kernel")"""
    same = (not split) and same_panel and ka == kb
    aligned = m % 2 == 0 and al16
    kapad, kbpad = pad16(ka), pad16(kb)
    direct = ka == kb and ka <= 80 and m % 4 == 0 and al32 and m >= 16 * GDH
    if split and not direct:
        return None
    mfull = m - m % (16 * GDH)
    if direct:
        occ = 2 if (kapad <= 48 or same) else 1
        nwaves = (min(4 * occ * num_cu, mfull // (16 * GDH)) + 3) // 4 * 4
        return dict(direct=1, same=same, tail=mfull < m, T=ladder(kapad // 16, 5), occ=occ, nwaves=nwaves,
                    nb=nwaves + (1 if mfull < m else 0), mfull=mfull, lds=0)
    nb = max(1, min(3 * num_cu, (m + GRAM_ROWS - 1) // GRAM_ROWS))
    ta, tb = kapad // 16, kbpad // 16
    ntiles = ta * (ta + 1) // 2 if same else ta * tb
    return dict(direct=0, same=same, aligned=aligned, tail=False, tpw=ladder((ntiles + GRAM_WAVES - 1) // GRAM_WAVES, 5),
                nb=nb, lds=(kapad if same else kapad + kbpad) * GRAM_LD * 8)


GRAM_OUT = ("ok", "direct", "same", "aligned", "tail", "T", "tpw", "occ", "nwaves", "nb", "mfull", "lds")


def test_gram_plan_reproduces_the_ladder_on_every_combination():
    fn = capi.lobpcg_gram_plan_fn()
    inp, out = (C.c_size_t * 8)(), (C.c_size_t * 12)()
    seen = set()
    for m, ka, kb, same_panel, (al16, al32), split, num_cu in itertools.product(
            MS, KS, KS, (0, 1), ((0, 0), (1, 0), (1, 1)), (0, 1), (1, 256)):
        inp[:] = (m, ka, kb, same_panel, split, al16, al32, num_cu)
        assert fn(0, inp, out) == capi.MI_OK
        got, want = dict(zip(GRAM_OUT, out)), parent_gram(m, ka, kb, same_panel, split, al16, al32, num_cu)
        where = (m, ka, kb, same_panel, split, al16, al32, num_cu, got, want)
        assert bool(got["ok"]) == (want is not None), where
        if want is None:
            seen.add("refused")
            continue
        assert all(got[key] == int(v) for key, v in want.items()), where
        if want["direct"]:
            assert got["nwaves"] % 4 == 0 and got["nwaves"] >= 4, where
        seen.add(("direct", want["T"], want["same"], want["tail"]) if want["direct"] else
                 ("tiled", want["tpw"], want["same"], want["aligned"]))
    # every instantiation of both families is reached, the tail kernel with and without, and the refusal
    assert {s[:3] for s in seen if s[0] == "direct"} == {("direct", T, sm) for T in range(1, 6) for sm in (False, True)}
    assert {s[3] for s in seen if s[0] == "direct"} == {False, True}
    # (S'S of at most 96 columns has 21 tiles: three per wave at the most)
    assert {s for s in seen if s[0] == "tiled"} == {("tiled", w, sm, al) for sm in (False, True)
                                                     for w in range(1, 4 if sm else 6) for al in (False, True)}
    assert "refused" in seen


def test_gram_pair_plan_reproduces_the_ladder_on_every_combination():
    fn = capi.lobpcg_gram_plan_fn()
    inp, out = (C.c_size_t * 5)(), (C.c_size_t * 6)()
    for m, k, pair, no_half, num_cu in itertools.product(MS, KS, (0, 1), (0, 1), (1, 256)):
        inp[:] = (m, k, pair, no_half, num_cu)
        assert fn(1, inp, out) == capi.MI_OK
        T, half, pair_out, occ, nwaves, mfull = out
        kpad, want_mfull = pad16(k), m - m % 16
        want_occ = 2 if kpad <= 32 else 1
        assert T == ladder(kpad // 16, 5) and pair_out == pair and mfull == want_mfull, (m, k, pair, no_half, num_cu)
        # the shared last tile column: a property of the pair, exactly when it is at most half full and the switch is off
        assert bool(half) == bool(pair and 1 <= k % 16 <= 8 and not no_half), (m, k, pair, no_half)
        assert occ == want_occ and nwaves == (min(4 * want_occ * num_cu, want_mfull // 16) + 3) // 4 * 4
        assert nwaves % 4 == 0


def test_the_six_eligibility_expressions_are_the_one_predicate():
    fn = capi.lobpcg_gram_plan_fn()
    inp, out = (C.c_size_t * 4)(), (C.c_size_t * 3)()

    def rule(m, k, aligned, min_rows):
        inp[:] = (m, k, int(aligned), min_rows)
        assert fn(2, inp, out) == capi.MI_OK
        return bool(out[0])

    inp[:] = (16, 16, 1, 16)
    assert fn(2, inp, out) == capi.MI_OK
    direct_min, pair_min = out[1], out[2]
    assert direct_min == 16 * GDH and pair_min == 16
    # every pointer of a call site aligned to 32 bytes, or exactly one of them not
    flags = [(1,) * 7] + [tuple(int(i != j) for i in range(7)) for j in range(7)]
    for m, k, f in itertools.product(MS, KS, flags):
        S, T1, T2 = f[:3]
        # `direct` of gram_impl (ka == kb = k; T2 null and T2 given), split_direct_ok, the copy in mi_lobpcg_gram_split
        assert rule(m, k, S and T1, direct_min) == (k <= 80 and m % 4 == 0 and bool(S) and bool(T1) and m >= 16 * GDH)
        old_split = k <= 80 and m % 4 == 0 and bool(S) and bool(T1) and bool(T2) and m >= 16 * GDH
        assert rule(m, k, S and T1 and T2, direct_min) == old_split
        # gram_pair_sym_direct_ok: S as three column blocks, Ta1, Ta2 null or given
        s0, s1, s2, ta1, ta2 = f[:5]
        for have_ta2 in (False, True):
            old = k <= 80 and m % 4 == 0 and bool(s0) and bool(s1) and bool(s2) and bool(ta1) and \
                (not have_ta2 or bool(ta2)) and m >= 16
            assert rule(m, k, all(f[:4]) and (not have_ta2 or ta2), pair_min) == old
        # the `aligned` lambdas of mi_lobpcg_gram_pair_sym_tblocks (two block sets; f[6] stays out) and of
        # mi_lobpcg_gram_pair_gen_blocks (three: nine pointers, the last block set all aligned or its first not)
        assert rule(m, k, all(f[:6]), pair_min) == (k <= 80 and m % 4 == 0 and m >= 16 and all(f[:3]) and all(f[3:6]))
        assert rule(m, k, all(f), pair_min) == (k <= 80 and m % 4 == 0 and m >= 16 and all(f[:3]) and all(f[3:6])
                                                  and bool(f[6]))


WIDTHS = ((72,), (48,), (24, 24, 24), (24, 19, 17), (24, 23, 23), (24, 25, 23), (20,), (24, 3, 24))


def parent_steps(cols):
    """the step table of update2_impl, or None where it gave the matrix-pipe form up"""
    steps, start = [], 0
    for bi, cb in enumerate(cols):
        if cb < 4:
            return None
        for j in range((cb + 3) // 4):
            first = min(4 * j, cb - 4)
            steps.append([bi, first] + [start + first + q if first + q >= 4 * j else -1 for q in range(4)])
        start += cb
    return steps if 6 <= len(steps) <= 18 else None


@pytest.mark.parametrize("cols", WIDTHS)
def test_update_plan_and_packed_coefficients(cols):
    rng = np.random.default_rng(sum(cols) * 7 + len(cols))
    ks = sum(cols)
    forms = set()
    for kc, off, m, pad in itertools.product((32, 33, 40, 48, 49), (False, True), (1000, 15), (0, 5)):
        Cm = np.asfortranarray(rng.standard_normal((ks + pad, 50)))   # (ldc = ks + pad; more columns than kc)
        mfma, steps, chunks, Ct = capi.lobpcg_update_plan(m, cols, kc, Cm, no_update_mfma=off)
        want_steps = parent_steps(cols) if (32 < kc <= 48 and m >= 16 and not off) else None
        assert mfma == (want_steps is not None), (cols, kc, off, m)
        forms.add(mfma)
        if mfma:
            assert steps.tolist() == want_steps and chunks.tolist() == [[0, 48, 0]]
            ids = steps[:, 2:].ravel()
            assert sorted(ids[ids >= 0]) == list(range(ks))          # every basis column in exactly one row
            assert np.all(ids[ids < 0] == -1)
            # a step's rows are consecutive columns of its block: block start + first + q
            starts = np.concatenate(([0], np.cumsum(cols)))
            for b, first, *lg in steps.tolist():
                assert 0 <= first <= cols[b] - 4
                assert all(v in (-1, starts[b] + first + q) for q, v in enumerate(lg))
            rows = Ct.reshape(len(steps) * 4, 48)
            back = np.zeros((ks, 48))
            for r, sidx in enumerate(ids):
                if sidx >= 0:
                    back[sidx] = rows[r]
                else:
                    assert not rows[r].any()
            assert np.array_equal(back[:, :kc], Cm[:ks, :kc]) and not back[:, kc:].any()
        else:
            assert steps.size == 0
            want, c0 = [], 0
            while c0 < kc:                                            # the 48 / 24 / 16 / 8 ladder
                left = kc - c0
                w = 48 if left > 32 else (24 if left > 16 else (16 if left > 8 else 8))
                want.append([c0, w, sum(ks * x[1] for x in want)])
                c0 += w
            assert chunks.tolist() == want and c0 >= kc
            packed = []
            for c0, w, _ in want:
                blk = np.zeros((ks, w))
                blk[:, :min(w, kc - c0)] = Cm[:ks, c0:min(c0 + w, kc)]
                packed.append(blk.ravel())
            assert np.array_equal(Ct, np.concatenate(packed))
    assert forms == ({False, True} if parent_steps(cols) else {False})


def test_update_plan_refusals():
    Cm = np.asfortranarray(np.zeros((97, 97)))
    for m, cols, kc in ((1000, (24, 24, 24, 24), 48), (1000, (24, 0), 24), (1000, (96, 1), 24), (1000, (24,), 0),
                        (1000, (24,), 97)):
        with pytest.raises(capi.MiError):
            capi.lobpcg_update_plan(m, cols, kc, Cm)
    with pytest.raises(capi.MiError):   # ldc < ks
        capi.lobpcg_update_plan(1000, (48, 24), 24, np.asfortranarray(np.zeros((71, 96))))


def parent_sweep(D, n, k, num_cu, zsegs_opt):
    tiles, nst, npass = (D + SW_ROWS - 1) // SW_ROWS, (n + D - 1) // D, (k + 7) // 8
    zsegs = zsegs_opt if zsegs_opt > 0 else (4 * num_cu + tiles * npass - 1) // (tiles * npass)
    zsegs = max(1, min(zsegs, nst // 12 if nst // 12 > 0 else 1, MAX_ROWS // tiles))
    zs = (nst + zsegs - 1) // zsegs
    zsegs = (nst + zs - 1) // zs
    return dict(tiles=tiles, nst=nst, npass=npass, zsegs=zsegs, zs=zs, xgrid=tiles * zsegs)


def test_sweep_plan_and_its_acceptance():
    edge = SW_ROWS * MAX_ROWS
    accepted = 0
    for D in (2 * SW_ROWS, 1600, 126 * 126, 250_000, edge - SW_ROWS, edge - 1, edge, edge + 1, edge + SW_ROWS, 2 ** 22 - 1):
        for nst, k, num_cu, zopt in itertools.product((1, 11, 12, 40, 126, 500), (1, 8, 24, 96), (1, 256), (0, 1, 7, 5000)):
            n = D * nst - (D // 3 if nst % 2 == 0 else 0)
            got = capi.lobpcg_sweep_plan(D, n, k, num_cu, zopt)
            want = parent_sweep(D, n, k, num_cu, zopt)
            assert {key: got[key] for key in want} == want, (D, n, k, num_cu, zopt)
            # the form is taken exactly where the launch's own requirement xgrid <= kMaxRows can hold
            assert bool(got["ok"]) == (want["xgrid"] <= MAX_ROWS) == (D <= edge), (D, n, k, num_cu, zopt, got)
            if got["ok"]:
                accepted += 1
                assert got["xgrid"] == got["tiles"] * got["zsegs"] <= MAX_ROWS
                assert got["zs"] * got["zsegs"] >= got["nst"] and got["zsegs"] >= 1
    assert accepted > 0
    for bad in ((0, 1000, 8), (1024, 2 ** 31, 8), (1024, 1000, 0), (1024, 1000, 97)):
        with pytest.raises(capi.MiError):
            capi.lobpcg_sweep_plan(*bad)


def test_sanitizer_program_of_the_plans():
    """tests/cpp/sanitize_lobpcg_plan.cpp: the update plans and the packing above, the other plans on a grid and the
    refused shapes, with its own main, built with g++ -fsanitize=address,undefined and run on the CPU; any report fails
    it.  Skipped only where the host has no sanitizer runtime."""
    from optimization_amd import build as b
    try:
        exe = b.build_sanitize_lobpcg_plan(run=True)
    except b.SanitizerUnavailable as e:
        pytest.skip(str(e))
    assert exe
