"""The longdouble restatement of the robust reweighting (tests/so3n_robust_reference.py) checked on itself, and the cases of
test_gpu_so3n_robust.py checked for what that test relies on: an unambiguous outlier count and both Huber branches."""
import numpy as np
import pytest

import so3n_robust_reference as rr
from so3_cases import LD


@pytest.mark.parametrize("kind", rr.KINDS)
@pytest.mark.parametrize("c", rr.SCALES)
def test_rho_prime_is_r_phi(kind, c):
    """central differences in longdouble (step h: truncation h^2 rho''' / 6, rounding eps_ld rho / h)"""
    r = np.linspace(LD(0.01), LD(2.8), 57)
    r = r[np.abs(r - LD(c)) > 1e-3]                     # (Huber's rho'' jumps at r = c)
    h = LD(1e-6)
    d = (rr.rho(kind, r + h, c) - rr.rho(kind, r - h, c)) / (2 * h)
    err = np.abs(d - r * rr.phi(kind, r, c)).max()
    scale = max(1.0, 1.0 / c) ** 2
    print(kind, c, float(err))
    assert err <= 1e-10 * scale


def test_l2_is_the_plain_problem():
    r = np.linspace(LD(0), LD(3), 31)
    assert np.all(rr.phi("l2", r, 0.5) == 1) and np.all(rr.rho("l2", r, 0.5) == r * r / 2)


@pytest.mark.parametrize("c", rr.SCALES)
def test_huber_is_continuous_at_c(c):
    lo, hi = np.nextafter(LD(c), LD(0)), np.nextafter(LD(c), LD(10))
    for f in (rr.phi, rr.rho):
        a, m, b = (f("huber", np.array([x]), c)[0] for x in (lo, LD(c), hi))
        assert abs(a - m) <= 4 * np.finfo(LD).eps * max(1, abs(m)) and abs(b - m) <= 4 * np.finfo(LD).eps * max(1, abs(m))


@pytest.mark.parametrize("mu", (16.0, 2.0, 1.0, 0.25))
def test_geman_mcclure_at_c_sqrt_mu_is_the_gnc_weight(mu):
    c = LD(0.3)
    r = np.linspace(LD(0), LD(2.8), 29)
    gnc = (mu * c * c / (r * r + mu * c * c)) ** 2
    assert np.abs(rr.phi("geman_mcclure", r, c * np.sqrt(LD(mu))) - gnc).max() <= 8 * np.finfo(LD).eps


@pytest.mark.parametrize("name", rr.VARIANTS)
def test_cases_have_an_unambiguous_outlier_count_and_both_huber_branches(name):
    c = rr.variant(name)
    r = rr.residual_norms(c)
    assert r.size == c.ei.size and (r.size == 0 or float(r.max()) <= 2 * np.sqrt(2) + 1e-3)
    for kind in rr.KINDS:
        for s in rr.SCALES:
            p = rr.phi(kind, r, s)
            assert np.abs(p - LD(1) / 2).min() >= rr.weight_tol(s), (name, kind, s)
    if name.endswith(":outliers") and c.ei.size >= 2:
        assert (r <= 0.5).any() and (r > 0.5).any(), name
        planted = float((r > 0.5).mean())
        print(name, "share of edges with r > 0.5:", planted)
        assert c.ei.size < 100 or 0.03 <= planted <= 0.25
