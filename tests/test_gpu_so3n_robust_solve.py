"""A GNC loop through the drop-in header (tests/cpp/harness_robust_so3n.cpp): Riemannian::TNT, then four rounds of
RotationAveraging::reweight (Geman-McClure at c sqrt(mu), mu halved each round) + TNT on a ring-with-chords graph of 300
rotations with 10 % planted outliers.  Every round against a fresh RotationAveraging built from that round's downloaded
weights and run from the same start (iterate to 1e-10, iteration counts exactly); at the end the mean angular error to the
ground truth, global rotation aligned, against that of the single L2 solve (strictly smaller).
Measured on the MI355X (profiles/so3n_robust.md): see there."""
import numpy as np
import pytest

import harness_robust_so3n_py as hr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run():
    p = hr.planted_problem()
    out = hr.RobustSo3nHarness().gnc(p)
    assert out["rc"] == 0, out["err"]
    return p, out


def test_every_round_is_the_solve_of_the_problem_with_the_downloaded_weights(run):
    p, out = run
    for k in range(hr.ROUNDS):
        a, b = out["R_rounds"][k], out["R_fresh"][k]
        err = float(np.abs(a - b).max())
        print("round", k, "outliers", int(out["outliers"][k]), "counts", out["counts"][k].tolist(), "|R - R_fresh|_inf", err)
        assert out["counts"][k][:3].tolist() == out["counts"][k][3:].tolist(), (k, out["counts"][k])
        assert err <= 1e-10, (k, err)
        assert out["W"][k].min() > 0 and out["W"][k].max() <= 1


def test_gnc_is_closer_to_the_ground_truth_than_the_l2_solve(run):
    p, out = run
    e_l2 = hr.mean_angular_error(out["R_l2"], p["truth"])
    e_gnc = hr.mean_angular_error(out["R_rounds"][-1], p["truth"])
    print("mean angular error: L2", e_l2, "GNC", e_gnc)
    assert e_gnc < e_l2
