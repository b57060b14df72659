"""The matrix families of window_cases.py are what they claim to be (no GPU, no library call): symmetric to the bit,
strictly diagonally dominant, sorted -- and every decision sparse.hip build_window has to take on them, re-derived here
from the rules as its comment block and mi_internal.h state them, equals the family's `expect`.  A generator that
drifts off the edge it was built for (a window one chunk wider, a value too many in the table, a far structure that
became pure) fails here, before any GPU test asserts the same `expect` on the library's answer."""
import numpy as np
import pytest

import window_cases as wc_

CHUNK, WIN_WAVES, FAR_CAP, WIN_HEAD = 64, 4, 2, 8     # rows per slice / chunk, kWinWaves, kFarCap, kWinHead


def restate(n, rowptr, col, val):
    """The rules, in words:
    storage   sliced ELL: 64 rows per slice, a slice as wide as its longest row, shorter rows (and the rows behind n in the
              last slice) padded with 0.0; stored slice by slice, entry position by entry position, lane by lane
    packed    at most 256 distinct stored bit patterns, padding included (column offsets within +-2^23: always here)
    wc        the smallest of 1, 2, 4 chunks whose window |col - row| <= 64 wc already holds 90 % of the entries the
              widest holds; no window unless the widest holds at least one off-diagonal entry per row on average
    head      the widest slice, at most 8
    zero      the window words need 0.0 in the table: where it is (first appearance in storage order), else appended
              behind the table if that has fewer than 256 entries, else no window
    far       entries outside the window: at most 2 per row; pure when all of them lie at one distance D; far stride: a
              distance shared by >= 80 % of them
    wk16      table incl. 0.0 <= 32 entries, head <= 8, LDS rows (ring, zero row, far slots) < 2048"""
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    dist = np.abs(col.astype(np.int64) - rows)
    length = np.diff(rowptr)
    nslices = (n + CHUNK - 1) // CHUNK
    padded_len = np.zeros(nslices * CHUNK, dtype=np.int64)
    padded_len[:n] = length
    per_slice = padded_len.reshape(nslices, CHUNK)
    width = per_slice.max(axis=1)
    # the table in order of first appearance
    seen, table = set(), []
    for s in range(nslices):
        for k in range(int(width[s])):
            for lane in range(CHUNK):
                r = s * CHUNK + lane
                v = val[rowptr[r] + k] if r < n and k < length[r] else 0.0
                b = np.float64(v).view(np.uint64).item()
                if b not in seen:
                    seen.add(b)
                    table.append(b)
        if len(table) > 256:
            break
    out = dict(packed=len(table) <= 256, ntable=len(table) if len(table) <= 256 else None, wc=0, head=0, far_max=0,
               pure_D=0, far_stride=0, zidx=None, wk16=False)
    if not out["packed"]:
        return out
    zero_at = table.index(0) if 0 in table else None
    out["zidx"] = zero_at
    held = {c: int((dist <= CHUNK * c).sum()) for c in (1, 2, 4)}
    offdiag_held = int(((dist <= CHUNK * 4) & (dist > 0)).sum())
    # (both readings of "one off-diagonal entry per row on average" must agree, or the family sits on that threshold)
    assert (offdiag_held >= n) == (held[4] >= n + n // 2 + 1)
    if offdiag_held < n:
        return out
    wc = next(c for c in (1, 2, 4) if held[c] * 10 >= held[4] * 9)
    head = int(width.max())
    if head > WIN_HEAD:
        return out
    if zero_at is None:
        if len(table) >= 256:
            return out
        zero_at = len(table)
    far = dist > CHUNK * wc
    far_per_row = np.bincount(rows[far], minlength=n)
    if far_per_row.max(initial=0) > FAR_CAP:
        return out
    strides, counts = np.unique(dist[far], return_counts=True)
    lds_rows = (2 * WIN_WAVES + 2 * wc) * CHUNK + 1 + WIN_WAVES * FAR_CAP * CHUNK
    out.update(wc=wc, head=head, far_max=int(far_per_row.max(initial=0)), zidx=zero_at,
               pure_D=int(strides[0]) if strides.size == 1 else 0,
               far_stride=next((int(s) for s, c in zip(strides, counts) if c * 10 >= counts.sum() * 8), 0),
               wk16=max(len(table), zero_at + 1) <= 32 and head <= 8 and lds_rows < 2048)
    return out


@pytest.mark.parametrize("name", wc_.ALL)
def test_family_is_symmetric_dominant_sorted_and_decided_as_expected(name):
    n, rowptr, col, val, expect = wc_.case(name)
    assert rowptr[0] == 0 and rowptr[-1] == col.size == val.size and rowptr.size == n + 1
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    # sorted, no duplicate, no empty row
    same_row = rows[1:] == rows[:-1]
    assert (np.diff(col.astype(np.int64))[same_row] > 0).all() and (np.diff(rowptr) > 0).all()
    # the transpose has the same bits: the triplets re-sorted by (column, row) are the triplets
    order = np.lexsort((rows, col))
    assert np.array_equal(col[order], rows) and np.array_equal(rows[order], col)
    assert np.array_equal(val[order].view(np.uint64), val.view(np.uint64))
    # strictly diagonally dominant, positive diagonal
    diag = np.zeros(n)
    diag[rows[col == rows]] = val[col == rows]
    off = np.bincount(rows[col != rows], weights=np.abs(val[col != rows]), minlength=n)
    assert (diag > 0).all() and (diag > off).all()
    got = restate(n, rowptr, col, val)
    assert got == expect._asdict(), (name, got)


def test_families_pin_the_decision_points_they_are_named_for():
    """what each family is FOR, beyond its expect tuple"""
    E = {k: wc_.case(k)[4] for k in wc_.ALL}
    assert {E[k].wc for k in wc_.WINDOWED} == {1, 2, 4}
    assert {E[k].head <= 7 for k in wc_.WINDOWED} == {True, False}
    # 0.0 appended (index == table size) with a small and with a full table; found in the table elsewhere
    assert E["circ_full"].zidx == E["circ_full"].ntable and E["circ_full_255"].zidx == 255
    assert all(E[k].zidx < E[k].ntable for k in wc_.WINDOWED if not k.startswith("circ_full"))
    assert E["circ_full_256"].packed and E["circ_full_256"].wc == 0 and not E["circ_full_257"].packed
    assert E["two_offset_pure_32"].wk16 and not E["two_offset_pure_33"].wk16
    assert E["two_offset_pure"].pure_D % 64 != 0
    # matchings: two far entries in every row, both ABOVE the row in 2300 of them, four distances, none dominant
    n, rowptr, col, val, e = wc_.case("matchings")
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    d = col.astype(np.int64) - rows
    far = np.abs(d) > 64
    assert (np.bincount(rows[far], minlength=n) == 2).all()
    assert sorted(np.unique(np.abs(d[far]))) == [700, 1000, 2300, 4000] and e.far_stride == 0 and e.pure_D == 0
    both_above = np.bincount(rows[far & (d > 0)], minlength=n) == 2
    assert both_above.sum() == 2300 and both_above[:1000].all()
    # third_far is matchings + one edge, and only the far cap stands between it and a window
    assert wc_.case("third_far")[2].size == col.size + 2 and E["third_far"].wc == 0 and E["third_far"].packed
    # the plane sweep of the panel product needs D >= 1024
    assert E["stencil_head8"].pure_D >= 1024 > E["two_offset_pure"].pure_D
