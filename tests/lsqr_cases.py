"""The case table of the LSQR parity tests (tests/test_cpu_lsqr_reference.py asserts its input condition,
tests/test_gpu_lsqr_parity.py runs it on the device).

Every case ends in at most 16 passes, by a NAMED rule, and is well-posed in the pass at which it ends: at every pass
of the long-double restatement the two sides of every comparison that decides a branch (the four stopping rules and
`xnorm <= Delta`) differ by at least MARGIN relative, and the float64 restatement ends at the same pass by the same rule.
(Undamped solves run to full convergence are NOT well-posed in that sense and are not used.)

Kinds:
  maxit  max_iterations = 3, no rule within reach                      -> exit 0, iterations == 3
  s1     b = A xs, btol = 1e-8, Atol = 0, cond(A) <= 3                 -> exit 1
  s2     generic b, lam = 0.3, btol = 0, Atol = 1e-8                   -> exit 2
  s3     btol = Atol = 1e-14, Acond_limit between the estimates of passes 2 and 3       -> exit 3 at pass 3
  s4     Delta between the |x| estimates of passes 1 and 2 of the unbounded solve       -> exit 4 at pass 2, step shortened
  beta0  A = 2 [I 0], b = ones: u is exactly 0 after the first product -> exit 1 at pass 0, iterations == 0, x == 0.5

Which kinds a shape can carry.  The bidiagonalisation of an n_y x n_x matrix ends, in exact arithmetic, after
r = min(n_y, n_x) passes: in pass r - 1 either beta or alpha comes out as pure rounding noise (or as an exact 0), every
quantity of a LATER pass is built on the direction that noise normalises to, and a relative comparison of rbar_norm at
a pass in which the true residual is 0 compares two noises.  So a case must end before or in pass r - 1, and in that
pass by a rule whose outcome the noise cannot change:
  r = 1 with n_y = 1, (1,1) and (1,2): beta of pass 0 is noise, and whether it is exactly 0 decides whether Anorm is
        updated at all.  Only exact data is well-posed there: beta0.
  r = 1 with n_x = 1, (2,1), and r = 2, (3,2) and (2,3): s2 ends in pass r - 1 because Arnorm = alpha |tau| is noise
        against Atol Anorm rbar_norm > 0; every other kind needs more passes than the shape has (maxit and s3 need
        pass 3, s4 needs pass 2) or ends on `noise <= 0` (s1: a consistent b has residual 0 after r passes).
  r = 5, (4097,5) and (5,4097): all five kinds; s1 uses a matrix of condition ~1.01 so that 1e-8 is reached in pass 3.
  2^21 + 4097: maxit only (cost)."""
import functools
from collections import namedtuple

import numpy as np
import scipy.sparse as sps

import lsqr_reference as ref

MARGIN = 1e-6
MAX_PASSES = 16
BIG = 2 ** 21 + 4097

Case = namedtuple("Case", "id ny nx kind matrix seed spread")

KINDS = ("maxit", "s1", "s2", "s3", "s4")
TINY = {(1, 1): ("beta0",), (1, 2): ("beta0",), (2, 1): ("s2",), (3, 2): ("s2",), (2, 3): ("s2",)}
MID = ((63, 65), (4096, 4095), (4097, 5), (5, 4097), (8193, 4099))
# square shapes carry both operator paths; one matrix per single-GPU form of the fused SpMV
SQUARE = 4097
CSR_MATRICES = ("few_values", "generic", "gather")


def band_matrix(ny, nx, seed, spread, few_values=False):
    """row i: 2 + spread cos(i) at column i mod nx, 0.5 spread sin(i) at column (i + 1) mod nx, and a few seeded
    entries of size 0.1 spread elsewhere.  few_values: the angles repeat with period 16 and the seeded entries are
    equal, so that the matrix has fewer than 256 distinct values (the packed value table of the device form).
    With at most 8 columns, column j is scaled by 1 + 0.5 spread j."""
    i = np.arange(ny)
    ang = (i % 16 if few_values else i).astype(np.float64)
    rng = np.random.default_rng(seed)
    extra = max(1, min(ny, nx) // 64)
    er, ec = rng.integers(0, ny, extra), rng.integers(0, nx, extra)
    ev = np.full(extra, 0.1 * spread) if few_values else 0.1 * spread * rng.uniform(0.5, 1.0, extra)
    rows = np.concatenate([i, i, er])
    cols = np.concatenate([i % nx, (i + 1) % nx, ec])
    vals = np.concatenate([2 + spread * np.cos(ang), 0.5 * spread * np.sin(ang), ev])
    if nx <= 8:  # (the wrapped band alone has nearly orthogonal columns of equal length: one singular value)
        vals = vals * (1 + 0.5 * spread * cols)
    A = sps.coo_matrix((vals, (rows, cols)), shape=(ny, nx)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A


def _spread(ny, nx, kind):
    if kind == "s1" and min(ny, nx) <= 5:
        return 0.01
    return 0.2


def _cases():
    out = []

    def add(ny, nx, kind, matrix="generic", seed=None):
        seed = 1000 * len(out) + 17 if seed is None else seed
        tag = "" if matrix == "generic" else "-" + matrix
        out.append(Case(f"{ny}x{nx}-{kind}{tag}", ny, nx, kind, matrix, seed, _spread(ny, nx, kind)))

    for (ny, nx), kinds in TINY.items():
        for kind in kinds:
            add(ny, nx, kind)
    for ny, nx in MID:
        for kind in KINDS:
            add(ny, nx, kind)
    for matrix in CSR_MATRICES:
        for kind in KINDS + ("beta0",):
            add(SQUARE, SQUARE, kind, matrix)
    add(BIG, BIG, "maxit")
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
VIEW_CASE = BY_ID[f"{SQUARE}x{SQUARE}-s2"]


def is_square(case):
    return case.ny == case.nx


@functools.lru_cache(maxsize=None)
def inputs(case_id):
    """(A as scipy CSR, b, keyword parameters of the solve)"""
    c = BY_ID[case_id]
    rng = np.random.default_rng(c.seed + 1)
    if c.kind == "beta0":
        k = min(c.ny, c.nx)
        A = sps.coo_matrix((np.full(k, 2.0), (np.arange(k), np.arange(k))), shape=(c.ny, c.nx)).tocsr()
        return A, np.ones(c.ny), dict(max_iterations=40, btol=1e-8, Atol=0.0)
    A = band_matrix(c.ny, c.nx, c.seed, c.spread, few_values=c.matrix == "few_values")
    b = rng.normal(size=c.ny)
    if c.kind == "maxit":
        return A, b, dict(max_iterations=3, btol=1e-12, Atol=1e-12)
    if c.kind == "s1":
        return A, A @ rng.normal(size=c.nx), dict(max_iterations=40, btol=1e-8, Atol=0.0)
    if c.kind == "s2":
        return A, b, dict(max_iterations=40, lam=0.3, btol=0.0, Atol=1e-8)
    # s3, s4: the threshold lies between two passes of the unbounded long-double solve (geometric mean: the margin to
    # either side is half their distance, which the input condition then checks like any other)
    free = ref.lsqr(A, b, max_iterations=4, btol=0.0, Atol=0.0)["trace"]
    if c.kind == "s3":
        limit = float(np.sqrt(free[2]["Acond"] * free[3]["Acond"]))
        return A, b, dict(max_iterations=40, btol=1e-14, Atol=1e-14, Acond_limit=limit)
    if c.kind == "s4":
        Delta = float(np.sqrt(free[1]["xnorm"] * free[2]["xnorm"]))
        return A, b, dict(max_iterations=40, btol=0.0, Atol=0.0, Delta=Delta)
    raise ValueError(c.kind)


@functools.lru_cache(maxsize=None)
def expected(case_id):
    """the long-double restatement of the case, with its iterates (of the largest shape: the first and the last)"""
    A, b, kw = inputs(case_id)
    keep = (0, kw["max_iterations"] - 1) if BY_ID[case_id].ny == BIG else range(kw["max_iterations"])
    return ref.lsqr(A, b, keep_x=keep, **kw)


def floor_orders(case_id):
    """the reference's own sequential sums and four re-associations; at the largest shape three re-associations (the
    sequential and the permuted sums are cumulative sums over 2 million terms: host time, not coverage)"""
    if BY_ID[case_id].ny == BIG:
        return ref.REASSOCIATIONS[:3]
    return (ref.SEQUENTIAL,) + ref.REASSOCIATIONS


@functools.lru_cache(maxsize=None)
def floor(case_id):
    """how far the float64 restatement moves from the long-double one under the summation orders of floor_orders
    (lsqr_reference.deviation), the maximum; and whether every one of them ended at the same pass by the same rule"""
    A, b, kw = inputs(case_id)
    e = expected(case_id)
    ops = ref.operators(A, np.float64)
    worst, same = 0.0, True
    for order in floor_orders(case_id):
        r = ref.lsqr(ops, b, dtype=np.float64, order=order, **kw)
        agree = r["iterations"] == e["iterations"] and r["exit_reason"] == e["exit_reason"]
        same = same and agree
        if agree:
            worst = max(worst, ref.deviation(r, e))
    return worst, same


def ends_as_named(case_id):
    """None, or what is wrong with how the long-double restatement of the case ended"""
    c, e = BY_ID[case_id], expected(case_id)
    want = dict(maxit=ref.EXIT_MAXIT, s1=ref.EXIT_S1, s2=ref.EXIT_S2, s3=ref.EXIT_S3, s4=ref.EXIT_S4,
                beta0=ref.EXIT_S1)[c.kind]
    if e["exit_reason"] != want:
        return f"exit {e['exit_reason']} instead of {want}"
    if len(e["trace"]) > MAX_PASSES:
        return f"{len(e['trace'])} passes"
    if c.kind == "maxit" and e["iterations"] != 3:
        return f"{e['iterations']} iterations"
    if c.kind == "s3" and e["iterations"] < 3:
        return f"limit crossed at pass {e['iterations']}"
    if c.kind == "s4" and (e["iterations"] < 2 or e["shortened"] != [e["iterations"]]
                           or e["xnorm"] != np.longdouble(inputs(case_id)[2]["Delta"])):
        return f"boundary: pass {e['iterations']}, shortened steps {e['shortened']}"
    if c.kind == "beta0" and (e["iterations"] != 0 or e["trace"][0]["beta"] != 0):
        return f"beta = {e['trace'][0]['beta']} at pass {e['iterations']}"
    if c.kind != "beta0" and min(c.ny, c.nx) <= len(e["trace"]) - 1:
        return f"{len(e['trace'])} passes on a matrix of rank {min(c.ny, c.nx)}"
    return None
