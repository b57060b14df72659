"""The fp64 oracle of SO(3)^N (oracle/problems.c) against the longdouble reference of tests/so3_cases.py, on every edge
case the GPU tests run (tests/test_gpu_so3n_edges.py): two independent statements of the same formulas -- the oracle's
Hessian shares nothing with the reference's but the operator formula -- so that what the device is compared with is
itself checked, and so that the distance between the two is a measured floor for the device comparisons.  Bars: those of
test_gpu_so3n.py::test_so3n_pieces_vs_oracle, norm-wise (conftest.rel_err)."""
import numpy as np
import pytest

import so3_cases as sc


def test_longdouble_is_wider_than_double():
    assert np.finfo(np.longdouble).eps < 1e-18


def test_special_rotations_reach_every_branch_and_tie():
    """the set is what its names say: rotations to rounding; every branch of the device's and of the host's Shepperd
    selection, as a point and (host) as a measurement and its transpose; trace exactly 0 and to either side; exact ties of
    the two largest diagonal entries"""
    sp = dict(sc.special_rotations())
    for name, S in sp.items():
        assert np.abs(S.T @ S - np.eye(3)).max() < 4e-16 and np.linalg.det(S) > 0, name
    assert {sc.device_branch(S) for S in sp.values()} == {0, 1, 2, 3}
    assert {sc.host_branch(S) for S in sp.values()} | {sc.host_branch(S.T) for S in sp.values()} == {0, 1, 2, 3}
    tr = {k: S[0, 0] + S[1, 1] + S[2, 2] for k, S in sp.items()}
    assert tr["perm"] == 0 and tr["perm_t"] == 0 and tr["pi_x"] == -1 and tr["identity"] == 3
    assert max(abs(tr[k]) for k in ("t23", "t23_below", "t23_above")) < 4e-15    # 2 pi / 3 and one ulp to either side
    assert tr["t23_below"] >= tr["t23"] >= tr["t23_above"] and tr["t23_below"] > tr["t23_above"]
    for a, br in (("x", 1), ("y", 2), ("z", 3)):     # a trace of a few ulps on either side of 0, each diagonal entry largest
        lo, hi = sp[f"t23_{a}_lo"], sp[f"t23_{a}_hi"]
        assert 0 < tr[f"t23_{a}_lo"] < 1e-14 and -1e-14 < tr[f"t23_{a}_hi"] < 0
        assert sc.device_branch(lo) == 0 and sc.device_branch(hi) == br and sc.host_branch(hi) == br
    assert sp["pi_110"][0, 0] == sp["pi_110"][1, 1] and sp["pi_111"][0, 0] == sp["pi_111"][1, 1] == sp["pi_111"][2, 2]
    for k, (a, b, c) in (("tie_xy", (0, 1, 2)), ("tie_yz", (1, 2, 0)), ("tie_xz", (0, 2, 1))):
        S = sp[k]
        assert S[a, a] == S[b, b] > S[c, c] and tr[k] < 0, k
    # where the two selections differ, the tests see both
    assert any(sc.device_branch(S) != sc.host_branch(S) for S in sp.values())


def test_cases_are_what_they_claim():
    for name in sc.CASE_NAMES:
        c = sc.case(name)
        E = c.ei.size
        assert c.ei.dtype == np.int32 and c.Rt.shape == (E, 9) and c.w.shape == (E,) and c.R.shape == (c.N, 9)
        assert np.all(c.ei != c.ej) and (E == 0 or (c.ei.min() >= 0 and max(c.ei.max(), c.ej.max()) < c.N))
        Rb = c.R.reshape(-1, 3, 3)
        assert np.abs(np.einsum("nji,njk->nik", Rb, Rb) - np.eye(3)).max() < 5e-16, name
        Sb = c.Rt.reshape(-1, 3, 3)
        defect = np.abs(np.einsum("nji,njk->nik", Sb, Sb) - np.eye(3)).reshape(E, -1).max(axis=1) if E else np.zeros(0)
        if name in sc.NONROT_CASES:      # exactly one measurement beyond the library's 1e-13 test for a rotation
            assert (defect > 1e-13).sum() == 1 and defect.max() > 1e-6
        else:
            assert defect.max(initial=0) < 5e-16, name
    deg = lambda c: np.bincount(np.concatenate([c.ei, c.ej]), minlength=c.N)
    d = deg(sc.case("hub_first_linspace"))
    assert d[0] == 1499 + 2 > 1024 and d[1:].max() == 3
    d = deg(sc.case("hub_last_spread"))
    assert d[-1] == 1499 + 2 and d[:-1].max() == 3
    c = sc.case("isolated_1500")
    d = deg(c)
    assert d[0] == 0 and d[-1] == 0 and np.all(d[128:192] == 0) and np.all(d[1:128] > 0) and np.all(d[192:-1] > 0)
    assert sc.singular_nodes(c).sum() == 66
    assert (sc.case("tiny_1").N, sc.case("tiny_1").ei.size) == (1, 0)
    assert (sc.case("tiny_2").N, sc.case("tiny_2").ei.size) == (2, 1)
    d = deg(sc.case("path_300"))
    assert d[0] == 1 and d[-1] == 1 and np.all(d[1:-1] == 2)
    d = deg(sc.case("powerlaw_5000"))
    assert d.min() == 1 and 250 <= d.max() <= 400
    c = sc.case("multigraph_linspace")
    pairs = list(zip(c.ei.tolist(), c.ej.tolist()))
    assert len(set(pairs)) < len(pairs) and any((j, i) in set(pairs) for i, j in pairs)
    assert (pairs[0], pairs[1], pairs[2]) == ((3, 9), (3, 9), (9, 3)) and c.w[0] != c.w[1]
    assert not np.array_equal(c.Rt[0], c.Rt[1])
    assert np.array_equal(c.Rt[3].reshape(3, 3), sc.special_rotations()[1][1])        # exactly the special rotation ...
    assert np.array_equal(c.Rt[5].reshape(3, 3), sc.special_rotations()[1][1].T)      # ... and its transpose
    assert (sc.case("ring_chords_1024_negative").w < 0).sum() == 5
    assert (sc.case("ring_chords_2049_some_zero").w == 0).sum() > 100
    assert sc.singular_nodes(sc.case("ring_chords_1024_node_zero")).tolist().count(True) == 1
    w = sc.case("ring_chords_1025_spread").w
    assert w.min() < 1e-5 and w.max() > 1e5


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_oracle_agrees_with_longdouble_reference(oracle, name):
    d = sc.oracle_vs_reference(oracle, name)
    # a singular block D_i (no edge, or every weight 0): 0 / 0 in the oracle and in the reference -- recorded behaviour
    sing = np.repeat(sc.singular_nodes(sc.case(name)), 3)
    assert np.array_equal(d.pop("precon_finite"), ~sing), name
    assert not np.isfinite(sc.reference_values(name)["precon"][sing].astype(np.float64)).any()
    print(name, {k: f"{v:.2e}" for k, v in d.items()})
    for k, v in d.items():
        assert v < sc.bar_of(k), (name, k, v)


def test_reference_hessian_is_the_derivative_of_its_gradient():
    """the longdouble reference checks itself: its operator-form Hessian against a central difference of its gradient
    along the retraction (longdouble leaves ~1e-10 at step 1e-5), on the case with a non-orthogonal measurement and on
    the multigraph; coordinate Hessian = symmetric part at a non-critical point, so compare <u, H v> symmetrised"""
    for name in ("nonrot_perturbed", "multigraph_negative"):
        c = sc.case(name)
        ref = sc.So3Ref(c)
        rng = np.random.default_rng(3)
        u, v = rng.normal(size=3 * c.N), rng.normal(size=3 * c.N)
        t = np.longdouble(1e-5)

        def f_at(xi):
            return sc.So3Ref(c, R=(ref.R @ sc.exp_ld(xi)).reshape(c.N, 9)).f()
        # second difference of f along u + v and u - v gives <u, H v> for the (symmetric) Riemannian Hessian
        ul, vl = u.astype(sc.LD), v.astype(sc.LD)
        q = lambda z: (f_at(t * z) - 2 * ref.f() + f_at(-t * z)) / (t * t)
        fd = (q(ul + vl) - q(ul - vl)) / 4
        uHv = (ul * ref.hess(v)).sum()
        vHu = (vl * ref.hess(u)).sum()
        assert abs(uHv - vHu) <= 1e-14 * abs(uHv), name
        assert abs(fd - uHv) <= 1e-6 * abs(uHv), (name, float(fd), float(uHv))
