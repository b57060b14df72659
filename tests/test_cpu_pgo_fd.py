"""The longdouble restatement of the joint pose-graph problem (tests/pgo_cases.py: PgoRef) against central differences along
the retraction, without a GPU.  This is what the formulas of optimization_amd/csrc/pgo.hip rest on: every GPU comparison of
test_gpu_pgo.py is against this restatement.

Step and bar.  Scanned on these cases and directions (|eta_i| of order one, longdouble arithmetic, s = 1e-1 ... 1e-12): both
differences fall as s^2 (8e-3 ... 1.6e-2 at s = 1e-1, 8e-13 ... 1.6e-12 at s = 1e-6), reach their minimum at s = 1e-7 --
first order 9.1e-14 ... 2.1e-13, second order 1.2e-13 ... 2.3e-13 relative -- and rise again with rounding (1e-12 at
s = 1e-8, 1e-10 at s = 1e-10).  The step is s = 1e-7 and the bar 2.5e-12, a decade above the largest minimum found.

First order: (f(x (+) s eta) - f(x (-) s eta)) / 2s against <g, eta>.  Second order: the gradient of the PULLBACK
v -> f(x (+) (s eta + v)) at v = 0 is J_r(s xi)' g_xi(x (+) s eta) (J_r the right Jacobian of exp on SO(3); delta rows
unchanged); its central difference in s is H eta for the Hessian along the retraction, which is what TNT's model needs and
what the kernel assembles."""
import numpy as np
import pytest

import pgo_cases as pc

LD = np.longdouble
STEP, BAR = LD(10) ** -7, 2.5e-12


def directions(p):
    return [e / 0.3 for e in pc.probes(p)]


@pytest.mark.parametrize("name", pc.FD_CASES)
def test_cases_are_what_they_claim(name):
    p = pc.problem(name)
    ei, ej = p["ei"], p["ej"]
    pairs = set(zip(ei.tolist(), ej.tolist()))
    if name == "fd12":
        assert any((b, a) in pairs for a, b in pairs), "no two-way pair"
        assert len(pairs) < ei.size, "no doubled edge"
    assert np.any(ei < ej) and np.any(ei > ej), "edges in one direction only"
    if name == "hub10":
        assert np.count_nonzero(ei == 0) + np.count_nonzero(ej == 0) >= p["N"] - 1
        assert np.any(ei == 0) and np.any(ej == 0)
    r = np.linalg.norm(pc.PgoRef(p).r.astype(np.float64), axis=1)
    assert 0.1 < np.median(r) < 10, "residuals not of order one"


@pytest.mark.parametrize("name", pc.FD_CASES)
def test_gradient_is_the_derivative_of_the_objective_along_the_retraction(name):
    p = pc.problem(name)
    ref = pc.PgoRef(p)
    g = ref.grad()
    for eta in directions(p):
        e = eta.astype(LD)
        fp, fm = pc.PgoRef(p, ref.retract(STEP * e)).f(), pc.PgoRef(p, ref.retract(-STEP * e)).f()
        want = (g * e).sum()
        err = float(abs((fp - fm) / (2 * STEP) - want) / abs(want))
        print(f"{name}: first order {err:.2e}")
        assert err <= BAR


@pytest.mark.parametrize("name", pc.FD_CASES)
def test_hessian_is_the_derivative_of_the_pullback_gradient(name):
    p = pc.problem(name)
    ref = pc.PgoRef(p)
    for eta in directions(p):
        d = (pc.pullback_grad(p, None, eta, STEP) - pc.pullback_grad(p, None, eta, -STEP)) / (2 * STEP)
        err = pc.rel_ld(d, ref.hess(eta))
        print(f"{name}: second order {err:.2e}")
        assert err <= BAR


@pytest.mark.parametrize("name", pc.FD_CASES)
def test_hessian_is_symmetric_and_its_blocks_reproduce_it(name):
    """<a, H b> = <b, H a>, and the node and slot blocks of PgoRef.blocks (the kernel's layout) applied as k_pgo_hvp applies
    them give H eta of the edge-by-edge form"""
    p = pc.problem(name)
    ref = pc.PgoRef(p)
    a, b = (e.astype(LD) for e in directions(p))
    ab, ba = (a * ref.hess(b)).sum(), (b * ref.hess(a)).sum()
    assert abs(ab - ba) <= 1e-16 * max(abs(ab), abs(ba), np.sqrt((ref.hess(a) ** 2).sum()))
    lay = pc.layout(p)
    B, G, Nsl, _, _ = ref.blocks(lay)
    N = p["N"]
    eta = a.reshape(N, 6)
    h = np.zeros((N, 6), dtype=LD)
    for l, node in enumerate(lay["perm"]):
        if node < 0:
            continue
        s, lane = l // 64, l % 64
        H = Nsl[(s * 19 + np.arange(9)) * 64 + lane].reshape(3, 3)
        K = Nsl[(s * 19 + 9 + np.arange(9)) * 64 + lane].reshape(3, 3)
        dt = Nsl[(s * 19 + 18) * 64 + lane]
        h[node, :3] = H @ eta[node, :3] - K.T @ eta[node, 3:]
        h[node, 3:] = dt * eta[node, 3:] - K @ eta[node, :3]
        for k in range(int(lay["slice_ptr"][s]), int(lay["slice_ptr"][s + 1])):
            slot = k * 64 + lane
            j, first = lay["nbr"][slot], lay["slot"][slot] & 1
            Bk = B[(k * 9 + np.arange(9)) * 64 + lane].reshape(3, 3)
            Gk = G[(k * 9 + np.arange(9)) * 64 + lane].reshape(3, 3)
            h[node, :3] -= Bk @ eta[j, :3]
            h[node, 3:] -= LD(lay["tauinc"][slot]) * eta[j, 3:]
            if first:
                h[node, :3] += Gk @ eta[j, 3:]
            else:
                h[node, 3:] += Gk @ eta[j, :3]
    assert pc.rel_ld(h, ref.hess(a)) <= 1e-16    # (1000 eps of longdouble: rows of up to 40 terms)
