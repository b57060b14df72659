"""Matrix families for the LDS-window form of the sparse kernels (a helper module for test_cpu_window_cases.py and
test_gpu_window_forms.py; not a conftest).

sparse.hip build_window decides, once per matrix: the window half-width (1, 2 or 4 chunks of 64 rows), the head width
(widest slice: the HW = 7 or HW = 8 kernels), whether the entries outside the window are all at row +- D ("pure": the
kernels compute those columns, slots by direction) or not (columns loaded, slots in order of appearance), whether a
row has more than two of them (no window), where 0.0 sits in the value table (found, or appended behind it, or no room
for it), and whether the 16-bit words exist.  The 7-point stencil is one point of that space; each family below is
another, and `expect` says which.

Every family is symmetric with bit-equal transposes, strictly diagonally dominant with a positive diagonal (hence
SPD), has sorted column indices and no empty row.  `case(name)` returns (n, rowptr, col, val, expect); the arrays are
shared between the tests and must not be written to.

expect:
  packed      the value-indexed copy exists (<= 256 distinct stored values, padding zeros included)
  ntable      distinct stored values (None where not packed)
  wc          window half-width in chunks; 0: no window form
  head        widest slice
  far_max     most entries outside the window in one row
  pure_D      D when every entry outside the window is at row +- D, else 0
  far_stride  the distance shared by >= 80 % of the entries outside the window, else 0
  zidx        index of 0.0 as the window words use it (== ntable: appended); None where the table has no 0.0 and there
              is no window to append it for
  wk16        the 16-bit words exist
(head, far_max, pure_D, far_stride, wk16 are those of the window form: 0 / False where wc == 0)"""
import functools
from collections import namedtuple

import numpy as np

from optimization_amd import workloads as wl

LD = np.longdouble
Expect = namedtuple("Expect", "packed ntable wc head far_max pure_D far_stride zidx wk16")


def _assemble(n, ei, ej, w, diag):
    """CSR of diag(diag) + sum of w_e (e_i e_j' + e_j e_i') for the unordered edges (ei, ej), each given ONCE: both
    triangles get the same double, so the transpose is bit-equal.  Sorted columns."""
    import scipy.sparse as sps
    ei, ej, w = np.asarray(ei, dtype=np.int64), np.asarray(ej, dtype=np.int64), np.asarray(w, dtype=np.float64)
    assert (ei != ej).all()
    key = np.minimum(ei, ej) * n + np.maximum(ei, ej)
    assert np.unique(key).size == key.size, "an edge given twice would be summed"
    rows = np.concatenate([ei, ej, np.arange(n)])
    cols = np.concatenate([ej, ei, np.arange(n)])
    vals = np.concatenate([w, w, np.broadcast_to(np.asarray(diag, dtype=np.float64), (n,))])
    A = sps.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()
    A.sort_indices()
    assert A.nnz == rows.size
    return n, A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)


def _laplacian(n, ei, ej, shift=0.1):
    """unit-weight graph Laplacian + shift I"""
    deg = np.bincount(np.concatenate([ei, ej]), minlength=n).astype(np.float64)
    return _assemble(n, ei, ej, np.full(len(ei), -1.0), deg + shift)


def _chain_edges(n, offsets):
    ei = np.concatenate([np.arange(n - d) for d in offsets])
    return ei, ei + np.concatenate([np.full(n - d, d) for d in offsets])


def _circulant_edges(n, offsets):
    ei = np.concatenate([np.arange(n) for _ in offsets])
    return ei, (ei + np.concatenate([np.full(n, d) for d in offsets])) % n


def _matchings_edges(n=8000):
    """chain couplings at 1 and 3 plus two involutions of the rows: every row has exactly two entries far from the
    diagonal, at four different distances, and 2300 rows ([0, 1000), [2000, 2700), [3400, 4000)) have BOTH of them
    above the row -- which slots assigned by direction could not hold"""
    ei, ej = _chain_edges(n, (1, 3))
    first = [(0, 1000, 1000), (2000, 2700, 700), (3400, 5700, 2300)]
    second = [(0, 4000, 4000)]
    for lo, hi, d in first + second:
        ei = np.concatenate([ei, np.arange(lo, hi)])
        ej = np.concatenate([ej, np.arange(lo, hi) + d])
    return n, ei, ej


def _head8_edges(n, offsets):
    """the chain couplings + i <-> i + 2 for i % 4 < 2 (n % 4 == 0): one more entry in every row"""
    assert n % 4 == 0 and 2 not in offsets
    ei, ej = _chain_edges(n, offsets)
    i = np.arange(n)
    i = i[i % 4 < 2]
    return np.concatenate([ei, i]), np.concatenate([ej, i + 2])


def _weighted(n, ei, ej, K, seed):
    """constant diagonal 10.0, the weight of every unordered edge drawn once from the K values k / K, k = 1 ... K, every
    one of them used (at most four edges of weight <= 1 per row: strictly dominant)"""
    rng = np.random.default_rng(seed)
    pick = np.concatenate([np.arange(K), rng.integers(0, K, size=len(ei) - K)])
    rng.shuffle(pick)
    return _assemble(n, ei, ej, (pick + 1.0) / K, 10.0)


def _stencil_head8():
    nx, ny, nz = 40, 40, 12
    n = nx * ny * nz
    rowptr, col, val = wl.laplacian_3d(nx, ny, nz)
    # the stencil's own edges (upper triangle) + i <-> i + 2 for i % 4 < 2: nx % 4 == 0, so i % 4 is x % 4 and x + 2 < nx;
    # every row gains exactly one entry (8 per interior row) and one unit of degree
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    up = col > rows
    ei, ej = rows[up], col[up].astype(np.int64)
    i = np.arange(n)
    i = i[i % 4 < 2]
    assert nx % 4 == 0 and ((i % nx) + 2 < nx).all()
    ei, ej = np.concatenate([ei, i]), np.concatenate([ej, i + 2])
    return _assemble(n, ei, ej, np.full(ei.size, -1.0), 7.1)


# name -> (builder, expect).  The expectations were worked out with the restatement of build_window's rules in
# test_cpu_window_cases.py, which re-derives every one of them on every run.
_FAMILIES = {
    # circulant, offsets 1 and 2, 90 full slices of constant width: no padding anywhere, so no 0.0 among the stored
    # values -- it is appended at index ntable.  Rows 0, n - 1 have two far entries (distances n - 1, n - 2), rows 1,
    # n - 2 one
    "circ_full": (lambda: _assemble(5760, *_circulant_edges(5760, (1, 2)), np.full(2 * 5760, -1.0), 4.1),
                  Expect(True, 2, 1, 5, 2, 0, 0, 2, True)),
    "band_wc2": (lambda: _laplacian(6000, *_chain_edges(6000, (1, 70, 100))),
                 Expect(True, 6, 2, 7, 0, 0, 0, 3, True)),
    "band_wc4": (lambda: _laplacian(6000, *_chain_edges(6000, (1, 200))),
                 Expect(True, 5, 4, 5, 0, 0, 0, 3, True)),
    "two_offset_pure": (lambda: _laplacian(12000, *_chain_edges(12000, (1, 300))),
                        Expect(True, 5, 1, 5, 2, 300, 300, 3, True)),
    "matchings": (lambda: _laplacian(*_matchings_edges()),
                  Expect(True, 5, 1, 7, 2, 0, 0, 4, True)),
    "stencil_head8": (_stencil_head8, Expect(True, 3, 1, 8, 2, 1600, 1600, 2, True)),
    # matchings + one more long edge on row 100: three entries outside the window in rows 100 and 6500
    "third_far": (lambda: (lambda n, ei, ej: _laplacian(n, np.append(ei, 100), np.append(ej, 6500)))(*_matchings_edges()),
                  Expect(True, 6, 0, 0, 0, 0, 0, 4, False)),
    # value-table boundaries.  Stored values = the diagonal 10.0 + K weights (+ 0.0 where slices are ragged).
    # 255 values without 0.0: appended at 255, window kept; 256: packed, but no room for 0.0, no window; 257: not packed
    "circ_full_255": (lambda: _weighted(5760, *_circulant_edges(5760, (1, 2)), 254, 1),
                      Expect(True, 255, 1, 5, 2, 0, 0, 255, False)),
    "circ_full_256": (lambda: _weighted(5760, *_circulant_edges(5760, (1, 2)), 255, 2),
                      Expect(True, 256, 0, 0, 0, 0, 0, None, False)),
    "circ_full_257": (lambda: _weighted(5760, *_circulant_edges(5760, (1, 2)), 256, 3),
                      Expect(False, None, 0, 0, 0, 0, 0, None, False)),
    # 10.0 + 30 weights + 0.0 = 32 table entries: the 16-bit words exist; with 31 weights (33 entries) they do not
    "two_offset_pure_32": (lambda: _weighted(12000, *_chain_edges(12000, (1, 300)), 30, 4),
                           Expect(True, 32, 1, 5, 2, 300, 300, 26, True)),
    "two_offset_pure_33": (lambda: _weighted(12000, *_chain_edges(12000, (1, 300)), 31, 5),
                           Expect(True, 33, 1, 5, 2, 300, 300, 26, False)),
    # two more, for the panel product: it has instantiations for a two-chunk window with a pure far structure and
    # with 8 entries per row, which none of the above reaches.  Couplings at 1 and 100 (window of two chunks) + a pure far
    # stride of 1000 (below the 1024 rows the plane sweep needs); the second with i <-> i + 2 for i % 4 < 2 on top
    "band_wc2_pure": (lambda: _laplacian(6000, *_chain_edges(6000, (1, 100, 1000))),
                      Expect(True, 6, 2, 7, 2, 1000, 1000, 3, True)),
    "band_wc2_pure_head8": (lambda: _laplacian(6000, *_head8_edges(6000, (1, 100, 1000))),
                            Expect(True, 6, 2, 8, 2, 1000, 1000, 3, True)),
}
FAMILIES = ("circ_full", "band_wc2", "band_wc4", "two_offset_pure", "matchings", "stencil_head8", "third_far")
EXTRA = ("band_wc2_pure", "band_wc2_pure_head8")
VARIANTS = ("circ_full_255", "circ_full_256", "circ_full_257", "two_offset_pure_32", "two_offset_pure_33")
ALL = FAMILIES + EXTRA + VARIANTS
WINDOWED = tuple(k for k in ALL if _FAMILIES[k][1].wc > 0)


def expect(name):
    """the family's expect without building the matrix"""
    return _FAMILIES[name][1]


@functools.lru_cache(maxsize=None)
def case(name):
    build, expect = _FAMILIES[name]
    n, rowptr, col, val = build()
    for a in (rowptr, col, val):
        a.setflags(write=False)
    return n, rowptr, col, val, expect


@functools.lru_cache(maxsize=None)
def _lowest_modes(name):
    import scipy.sparse as sps
    import scipy.sparse.linalg as sla
    n, rowptr, col, val, _ = case(name)
    A = sps.csr_matrix((val, col, rowptr), shape=(n, n)).tocsc()
    _, U = sla.eigsh(A, k=8, sigma=0.0, which="LM", v0=np.random.default_rng(1).normal(size=n), tol=1e-5)
    U.setflags(write=False)
    return U


def near_minimiser(name, p):
    """a point of St(n, p) 1e-3 away from the span of the p lowest modes.  At a random point the Riemannian Hessian of the
    Rayleigh quotient is indefinite and STPCG leaves along -g before one Hessian product has entered the step; here it
    is positive definite on the tangent space and the solve runs its iterations, every one through the Hessian pass.
    (The modes need not be exact: tolerance 1e-5, computed once per family.)"""
    n = case(name)[0]
    rng = np.random.default_rng(p)
    return wl.thin_qr(_lowest_modes(name)[:, :p] + (1e-3 / np.sqrt(n)) * rng.normal(size=(n, p)))


# ------------------------------------------------------------------------------------------------------------------
# longdouble reference of the product, shared by the tests of one matrix
# ------------------------------------------------------------------------------------------------------------------
def spmm_ld(rowptr, col, val, X):
    """(A X, |A| |X|) with every row's sum accumulated in longdouble, entry after entry; X is n x k.  Every row has an
    entry (the diagonal)."""
    assert (np.diff(rowptr) > 0).all()
    starts = np.asarray(rowptr[:-1], dtype=np.int64)
    prod = val.astype(LD)[:, None] * X.astype(LD)[col]
    return np.add.reduceat(prod, starts, axis=0), np.add.reduceat(np.abs(prod), starts, axis=0)


def sum_bound(head, absAX):
    """A row's sum of m <= head products, each rounded once (u = 2^-53) and added in turn to an accumulator that starts at
    0: a term passes through its product's rounding and at most m - 1 additions' (the first addition, to 0, is exact),
    so |computed - exact| <= ((1 + u)^m - 1) |A| |X| <= (head + 1) u |A| |X| (m u < 1e-14: the second-order terms fit in
    the + 1); with fused multiply-adds it is less.  The reference's own error, (head + 1) 2^-64, is 2000 times smaller."""
    return (head + 1) * 2.0 ** -53 * absAX.astype(np.float64)
