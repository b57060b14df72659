"""The LSQR restatement (tests/lsqr_reference.py) and its case table (tests/lsqr_cases.py), without a GPU:
the input condition of every case, and the restatement against the real reference templates (where oracle/_ref is
built) and against this project's own header on host vectors (tests/cpp/libharness_host.so, where built).

The dense comparisons cover every case of the table except the one at n = 2^21 + 4097, whose dense copy would take
35 TB."""
import os

import numpy as np
import pytest

import lsqr_cases as lc
import lsqr_reference as ref

SMALL = [c.id for c in lc.CASES if c.ny < lc.BIG]


@pytest.mark.parametrize("case_id", [c.id for c in lc.CASES])
def test_case_is_well_posed_and_ends_by_its_rule(case_id):
    """no case is excluded: one that fails gets other inputs (seed, spread, tolerance), not a skip"""
    e = lc.expected(case_id)
    assert lc.ends_as_named(case_id) is None, lc.ends_as_named(case_id)
    m = ref.margin(e["sides"])
    assert m >= lc.MARGIN, f"a comparison is decided by {m:.1e} relative"
    fl, same = lc.floor(case_id)
    assert same, "a float64 restatement ends at another pass or by another rule"
    print(f"{case_id}: exit {e['exit_reason']} after {e['iterations']} iterations, margin {m:.1e}, float64 floor {fl:.1e}")


def test_table_covers_the_shapes_and_kinds():
    shapes = {(c.ny, c.nx) for c in lc.CASES}
    assert shapes >= {(1, 1), (2, 1), (1, 2), (3, 2), (2, 3), (63, 65), (4096, 4095), (4097, 5), (5, 4097),
                      (8193, 4099), (lc.BIG, lc.BIG)}
    # the shapes of rank 1 and 2 carry the kinds lsqr_cases.py reasons out, no fewer
    tiny = {(c.ny, c.nx): set() for c in lc.CASES if min(c.ny, c.nx) <= 2}
    for c in lc.CASES:
        if (c.ny, c.nx) in tiny:
            tiny[(c.ny, c.nx)].add(c.kind)
    assert tiny == {(1, 1): {"beta0"}, (1, 2): {"beta0"}, (2, 1): {"s2"}, (3, 2): {"s2"}, (2, 3): {"s2"}}
    for ny, nx in lc.MID:
        assert {c.kind for c in lc.CASES if (c.ny, c.nx) == (ny, nx)} == set(lc.KINDS)
    for matrix in lc.CSR_MATRICES:
        assert {c.kind for c in lc.CASES if c.matrix == matrix and lc.is_square(c)} >= set(lc.KINDS) | {"beta0"}
    assert {c.id for c in lc.CASES if c.kind == "beta0"} >= {"1x1-beta0", "4097x4097-beta0"}
    assert lc.BIG > 512 * 4096 and lc.BIG % 2 == 1
    assert len(lc.BY_ID) == len(lc.CASES)
    assert all(sum(o is not ref.SEQUENTIAL for o in lc.floor_orders(c.id)) >= 3 for c in lc.CASES)  # re-associations


def test_restatement_special_exits():
    A = np.array([[2.0, 0.0], [0.0, 3.0], [1.0, 1.0]])
    r = ref.lsqr(A, np.zeros(3))
    assert r["exit_reason"] == ref.EXIT_TRIVIAL and r["iterations"] == 0 and not r["x"].any()
    r = ref.lsqr(A, np.ones(3), max_iterations=0)
    assert r["exit_reason"] == ref.EXIT_MAXIT and r["iterations"] == 0 and not r["x"].any()
    xs = np.linalg.lstsq(A, np.ones(3), rcond=None)[0]
    r = ref.lsqr(A, np.ones(3), btol=0.0, Atol=1e-12)
    assert np.abs(r["x"].astype(float) - xs).max() < 1e-14


def _dense_parity(solver, case_id):
    A, b, kw = lc.inputs(case_id)
    e = lc.expected(case_id)
    r = solver.lsqr_dense(A.toarray(), b, **kw)
    assert r["rc"] == 0
    assert r["iterations"] == e["iterations"]
    xs = np.abs(e["x"]).max()
    ex = float(np.abs(r["x"] - e["x"]).max() / xs)
    en = float(abs(r["xnorm"] - e["xnorm"]) / e["xnorm"])
    print(f"{case_id}: x {ex:.1e}, xnorm {en:.1e}")
    assert ex <= 1e-12 and en <= 1e-12, (ex, en)
    if lc.BY_ID[case_id].kind == "s4":
        assert r["xnorm"] == kw["Delta"]


@pytest.mark.parametrize("case_id", SMALL)
def test_restatement_matches_the_reference_templates(reference, case_id):
    _dense_parity(reference, case_id)


@pytest.fixture(scope="module")
def host_templates():
    import oracle_py
    if not os.path.exists(oracle_py.TemplateHarness.PATH):
        pytest.skip("tests/cpp/libharness_host.so not built")
    return oracle_py.TemplateHarness()  # (a library that is there and does not load is an error, not a skip)


@pytest.mark.parametrize("case_id", SMALL)
def test_restatement_matches_this_projects_header_on_host_vectors(host_templates, case_id):
    _dense_parity(host_templates, case_id)
