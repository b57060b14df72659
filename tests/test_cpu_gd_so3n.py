"""GradientDescent on SO(3)^N without a GPU: the fixture's conditions, the compiled forms of the new kernels, the
untouched figures of the existing ones, and no host fall-back of the two new entry points."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from test_cpu_kernel_resources import HIPCC, _resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (TotalSGPRs, VGPRs, compiler's waves/SIMD, scratch bytes per lane) of the SO(3)^N kernels as commit c5433d0 compiles
# them (the parent of the gradient-only pass): the pass is a new kernel next to these
PARENT = "c5433d0"
PARENT_FIGURES = {
    "k_so3_model<false, false, false>": (42, 88, 5, 0),
    "k_so3_model<false, false, true>": (44, 88, 5, 0),
    "k_so3_model<false, true, false>": (42, 92, 5, 0),
    "k_so3_model<false, true, true>": (44, 92, 5, 0),
    "k_so3_model<true, false, false>": (66, 166, 3, 0),
    "k_so3_model<true, false, true>": (68, 166, 3, 0),
    "k_so3_model<true, true, false>": (62, 122, 4, 0),
    "k_so3_model<true, true, true>": (64, 122, 4, 0),
    "k_so3_retract<false>": (78, 64, 8, 0),
    "k_so3_retract<true>": (78, 60, 8, 0),
    "k_so3_quat": (26, 37, 8, 0),
    # the gradient-only pass as commit 109fb61 compiles it (the figures of profiles/gd_so3n_ab.md): the last commit in
    # which it had a body of its own, before k_so3_model and k_so3_grad became two entry names over one body
    "k_so3_grad<false, false>": (44, 106, 4, 0),
    "k_so3_grad<false, true>": (46, 106, 4, 0),
    "k_so3_grad<true, false>": (44, 110, 4, 0),
    "k_so3_grad<true, true>": (46, 110, 4, 0),
}


@pytest.fixture(scope="module")
def so3_resources():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    return _resource_usage("so3.hip")


def test_gd_so3n_fixture_meets_its_conditions():
    """tests/golden/gd_so3n.json (make_golden_gd_so3n.py): both runs stop on the gradient tolerance within 400 iterations,
    with iterations of one line-search trial and iterations of more than one"""
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "gd_so3n.json")))
    assert sorted(g) == ["N150", "N40"] and (g["N40"]["N"], g["N40"]["seed"], g["N150"]["N"]) == (40, 7, 150)
    for key, rec in g.items():
        ls, prm = rec["linesearch_iterations"], rec["params"]
        assert rec["status"] == 0                                            # GradientDescentStatus::Gradient
        assert rec["iterations"] == len(ls) <= 400 and rec["iterations"] < prm["max_iterations"]
        assert rec["gradfx_norm"] < prm["gradient_tolerance"]
        assert any(v > 1 for v in ls) and any(v == 1 for v in ls), (key, sorted(set(ls)))
        assert all(1 <= v < prm["max_ls_iterations"] for v in ls)
        assert len(rec["objective_values"]) == rec["iterations"] and len(rec["x"]) == 9 * rec["N"]
        trace = rec["objective_values"] + [rec["f"]]
        assert all(a > b for a, b in zip(trace, trace[1:]))                  # every accepted step decreases f
        assert prm["alpha"] == rec["alpha_times_max_weighted_degree"] / rec["max_weighted_degree"]
        assert 0 < prm["beta"] < 1 and 0 < prm["sigma"] < 1
        X = np.array(rec["x"]).reshape(-1, 3, 3)                             # the final point is a point of SO(3)^N
        assert np.abs(np.swapaxes(X, 1, 2) @ X - np.eye(3)).max() < 1e-12 and np.all(np.linalg.det(X) > 0)


def test_gradient_only_pass_is_compiled_in_all_four_forms_without_scratch(so3_resources):
    r = so3_resources
    for sq in ("false", "true"):
        for gq in ("false", "true"):
            name = f"k_so3_grad<{sq}, {gq}>"
            assert name in r, (name, sorted(r))
            sg, vg, occ, scratch = r[name]
            msg, mvg, mocc, _ = r[f"k_so3_model<true, {sq}, {gq}>"]
            print(name, "SGPRs", sg, "VGPRs", vg, "waves/SIMD", occ, "scratch", scratch, "| model form VGPRs", mvg,
                  "waves/SIMD", mocc)
            assert scratch == 0, name + " spills"
            assert vg <= mvg and occ >= mocc


def test_existing_so3n_kernels_compile_to_the_parents_figures(so3_resources):
    for name, figures in PARENT_FIGURES.items():
        assert so3_resources.get(name) == figures, (name, so3_resources.get(name), figures, "parent " + PARENT)


def test_new_so3n_entry_points_have_no_cpu_fallback():
    """Without a device both entry points answer MI_ERR_NO_DEVICE (no context, hence no problem object, can exist: the
    contract of test_cpu_oracle_templates.py::test_no_cpu_fallback_without_gpu)."""
    from optimization_amd import capi
    L = capi.load()
    if capi.device_count() > 0:
        pytest.skip("a GPU is present")
    out = (C.c_double * 2)()
    assert L.mi_so3n_gradient(None, None, None) == 4
    assert b"no HIP device" in L.mi_last_error()
    assert L.mi_so3n_armijo_trial(None, None, None, C.c_double(0.5), None, None, out) == 4
    assert out[0] == 0.0 and out[1] == 0.0
