"""CPU side of the extra-argument pack (Args...) work: the new harnesses compile with g++ and pass clang's front end, and the host-vector template with a pack is the host-vector template without one,
bit for bit (the reference itself exports no pack-carrying case through oracle/_ref beyond the sphere problem that
tests/test_cpu_oracle_templates.py already holds against it)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


CLANG = "/opt/rocm/lib/llvm/bin/clang++"
HARNESSES = ("harness_args", "harness_lsqr_observer")


@pytest.mark.parametrize("name", HARNESSES)
def test_the_pack_harness_builds_with_gcc(name):
    from optimization_amd import build
    out = build.build_harness()
    assert any(p.endswith("lib" + name + ".so") and os.path.exists(p) for p in out), name


@pytest.mark.skipif(not os.path.exists(CLANG), reason="no clang front end installed")
@pytest.mark.parametrize("name", HARNESSES)
def test_the_pack_instantiations_pass_the_clang_front_end(name):
    """the translation unit itself through clang -fsyntax-only, here and now (build_harness() runs the same check, but
    only when it rebuilds)"""
    inc = [os.path.join(ROOT, "optimization_amd", "include"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "include")]
    cmd = [CLANG, "-std=c++17", "-fsyntax-only"] + [a for i in inc for a in ("-I", i)] + \
        [os.path.join(ROOT, "tests", "cpp", name + ".cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]


def test_host_template_with_a_pack_equals_the_empty_pack_run():
    import args_py
    import oracle_py
    H = args_py.ArgsHarness()
    pr = oracle_py.stpcg_stop_problem()
    a = H.counting(0, 1, pr["g"], pr["D"], max_iterations=6, pack=0)              # Args = {}
    b = H.counting(0, 1, pr["g"], pr["D"], max_iterations=6)                      # Args = {size_t}
    assert a["rc"] == 0 and b["rc"] == 0
    assert a["iterations"] == b["iterations"] == b["counter"] > 0 and a["counter"] == 0
    assert np.array_equal(a["s"], b["s"]) and a["M_norm"] == b["M_norm"]


def test_host_stpcg_with_a_counting_pack_equals_the_fixture_of_the_reference(golden):
    import args_py
    import oracle_py
    H = args_py.ArgsHarness()
    fx = golden("stpcg_user_stop.json")
    pr = oracle_py.stpcg_stop_problem(fx["n"], fx["seed"])
    for c in fx["cases"]:
        r = H.counting(0, 0, pr["g"], pr["D"], pr["Minv"] if c["precon"] else None, stop_at=c["stop_at"])
        assert r["rc"] == 0 and (r["iterations"], r["counter"]) == (c["iterations"], c["calls"])
        assert np.array_equal(r["s"], np.array(c["s"])) and r["M_norm"] == c["M_norm"]
