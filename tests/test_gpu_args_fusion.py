"""The fused paths survive the reference's extra-argument pack (`Args &...`: a cache, a counter -- Base/Concepts.h:20-38,
the way every Riemannian client of the reference calls TNT and GradientDescent).  tests/cpp/harness_args.cpp drives each
optimizer through one template over the pack; here the run with a non-empty pack is held against the empty-pack run of
the same process: the tagged callables ignore the pack, so the same kernels run on the same data -- same fusion
counters, same bits -- and against the fixtures of the real reference."""
import numpy as np
import pytest

from optimization_amd import workloads as wl

pytestmark = pytest.mark.gpu

TRACES = ("objective_values", "gradient_norms", "preconditioned_gradient_norms", "trust_region_radius",
          "inner_iterations", "update_step_norms", "update_step_M_norms", "gain_ratios", "x")


@pytest.fixture(scope="module")
def args():
    import args_py
    return args_py.ArgsHarness()


def _stiefel_fixture(golden, oracle):
    g = golden("tnt_stiefel_8x7x6.json")
    nx, ny, nz = g["grid"]
    p, n = g["p"], nx * ny * nz
    rowptr, col, val = wl.laplacian_3d(nx, ny, nz)
    X0 = np.array(g["x0"]).reshape(n, p)
    prm = oracle.default_params(gradient_tolerance=1e-8, relative_decrease_tolerance=0, stepsize_tolerance=0,
                                preconditioned_gradient_tolerance=0, Delta_tolerance=0, max_iterations=200,
                                max_TPCG_iterations=50)
    return g, n, p, rowptr, col, val, X0, prm


def _same_bits(a, b):
    assert (a["status"], a["outer_iterations"], a["accepted"]) == (b["status"], b["outer_iterations"], b["accepted"])
    for k in TRACES:
        assert np.array_equal(a[k], b[k]), k
    assert a["f"] == b["f"] and a["gradfx_norm"] == b["gradfx_norm"]


def test_tnt_stiefel_with_a_pack_keeps_every_fused_path(args, oracle, golden):
    """TNT on the 8x7x6 Laplacian, p = 3, with Args = {int, DeviceVector} through the pack-templated accessors: every
    inner solve in mi_stpcg, every trial step by the fused chain, and the whole result bit-identical to the empty-pack
    run; counts and accept sequence of the real reference (tests/golden/tnt_stiefel_8x7x6.json)."""
    g, n, p, rowptr, col, val, X0, prm = _stiefel_fixture(golden, oracle)
    a = args.tnt_stiefel(n, p, rowptr, col, val, X0, prm, pack=0)
    b = args.tnt_stiefel(n, p, rowptr, col, val, X0, prm, pack=1)
    assert a["rc"] == 0 and b["rc"] == 0, (a.get("err"), b.get("err"))
    ka, kb = a["counters"], b["counters"]
    print("empty pack:", ka, "\n{int, DeviceVector}:", kb)
    outer = b["outer_iterations"]
    assert kb["fused_stpcg_solves"] == outer and kb["generic_stpcg_solves"] == 0
    assert kb["fused_trial_steps"] == outer and kb["generic_trial_steps"] == 0
    assert kb["generic_inner_products"] <= ka["generic_inner_products"]
    assert kb["syncs"] == ka["syncs"] and kb["user_calls"] == outer
    _same_bits(a, b)
    assert (b["status"], outer, b["accepted"]) == (g["status"], g["outer_iterations"], g["accepted"])
    assert list(b["inner_iterations"]) == g["inner_iterations"]
    acc = lambda r: list(np.diff(r) != 0)  # noqa: the objective moves exactly at the accepted steps
    assert acc(b["objective_values"][:-1]) == acc(np.array(g["objective_values"])[:-1])
    assert abs(b["f"] - g["f"]) < 1e-12


def test_tnt_so3n_with_a_pack_and_its_own_preconditioner(args, oracle, golden):
    """RotationAveraging with its block-Jacobi preconditioner on the SO(3)^40 problem, Args = {DeviceVector}"""
    g = golden("tnt_so3n_40.json")["block_jacobi"]
    N = g["N"]
    ei, ej, Rt, w, _, Rinit = wl.pose_graph(N, seed=g["seed"])
    prm = oracle.default_params(gradient_tolerance=1e-8, relative_decrease_tolerance=0, stepsize_tolerance=0,
                                preconditioned_gradient_tolerance=0, Delta_tolerance=0, max_iterations=100)
    a = args.tnt_so3n(N, ei, ej, Rt, w, Rinit, prm, pack=0)
    b = args.tnt_so3n(N, ei, ej, Rt, w, Rinit, prm, pack=1)
    assert a["rc"] == 0 and b["rc"] == 0, (a.get("err"), b.get("err"))
    kb = b["counters"]
    outer = b["outer_iterations"]
    print("empty pack:", a["counters"], "\n{DeviceVector}:", kb)
    assert kb["fused_stpcg_solves"] == outer and kb["generic_stpcg_solves"] == 0
    assert kb["fused_trial_steps"] == outer and kb["generic_trial_steps"] == 0
    assert kb == dict(a["counters"], seconds=kb["seconds"])
    _same_bits(a, b)
    assert (b["status"], outer, b["accepted"]) == (g["status"], g["outer_iterations"], g["accepted"])
    assert list(b["inner_iterations"]) == g["inner_iterations"]


def test_gradient_descent_with_a_pack_keeps_the_fused_armijo_trial(args, golden):
    """GradientDescent on the Stiefel case p = 3 of tests/golden/gd_counts.json with Args = {DeviceVector}: the fixture's
    counts, one host synchronisation per Armijo trial as in the empty-pack run, bit-identical objective trace"""
    g = golden("gd_counts.json")["stiefel_p3"]
    nx, ny, nz = g["grid"]
    p, n = g["p"], nx * ny * nz
    rowptr, col, val = wl.laplacian_3d(nx, ny, nz)
    X0 = wl.random_stiefel(n, p, seed=g["seed"])
    a = args.gd_stiefel(n, p, rowptr, col, val, X0, g["params"], pack=0)
    b = args.gd_stiefel(n, p, rowptr, col, val, X0, g["params"], pack=1)
    assert a["rc"] == 0 and b["rc"] == 0, (a["err"], b["err"])
    assert (b["status"], b["iterations"]) == (g["status"], g["iterations"])
    assert list(b["linesearch_iterations"]) == g["linesearch_iterations"]
    m = len(g["objective_values"])
    assert np.allclose(b["objective_values"][:m], g["objective_values"], rtol=1e-12)
    trials = int(np.sum(b["linesearch_iterations"]))
    print("trials", trials, "syncs: empty pack", a["counters"]["syncs"], "{DeviceVector}", b["counters"]["syncs"])
    assert b["counters"]["syncs"] == a["counters"]["syncs"] <= trials + 4
    assert b["counters"]["fused_trial_steps"] == trials and b["counters"]["generic_trial_steps"] == 0
    assert np.array_equal(a["objective_values"], b["objective_values"]) and np.array_equal(a["x"], b["x"])
    assert a["gradfx_norm"] == b["gradfx_norm"]


def _nonsym_sparse(n, seed):  # (the matrix of tests/golden/lsqr_tnls.json: make_golden.py)
    import scipy.sparse as sps
    rng = np.random.default_rng(seed)
    A = sps.diags([np.full(n - 1, -1.0), np.full(n, 4.0), np.full(n - 1, 2.0)], [-1, 0, 1]).tolil()
    for _ in range(3 * n):
        i, j = rng.integers(0, n, size=2)
        A[i, j] += rng.normal() * .3
    return sps.csr_matrix(A)


def test_lsqr_with_a_pack_stays_in_the_fused_solver(args, golden):
    """LSQR on the damped case of tests/golden/lsqr_tnls.json with Args = {int, DeviceVector}.  (TNLS itself cannot be
    instantiated with a non-empty pack, here as in the reference: its J is declared without the pack and called with
    it, reference TNLS.h:269,422 -- so the pack reaches mi_lsqr through LinearAlgebra::LSQR.)"""
    kw = dict(lam=0.3)
    A = _nonsym_sparse(300, 2)
    b = np.random.default_rng(9).normal(size=300)
    fx = [c for c in golden("lsqr_tnls.json")["lsqr"] if c["kw"] == kw][0]
    assert abs(float(A.sum()) - fx["A_checksum"]) < 1e-9
    r0 = args.lsqr_csr(A, b, pack=0, **kw)
    r1 = args.lsqr_csr(A, b, pack=1, **kw)
    assert r0["rc"] == 0 and r1["rc"] == 0, (r0["err"], r1["err"])
    assert r1["counters"]["fused_lsqr_solves"] == 1 and r1["counters"]["generic_lsqr_solves"] == 0
    assert r1["counters"]["generic_inner_products"] == 0
    assert r1["iterations"] == r0["iterations"] == fx["iterations"]
    assert np.array_equal(r0["x"], r1["x"]) and r0["xnorm"] == r1["xnorm"]
    assert np.abs(r1["x"] - np.array(fx["x"])).max() <= 1e-10 * max(1.0, np.abs(fx["x"]).max())


def test_a_pack_that_user_code_writes(args, golden):
    """Args = {size_t}: a counter of the caller's, incremented by an STPCGUserFunction (observed fused solve) and by a
    TNTUserFunction.  The counters equal those of the same template on the host vector (the reference's statement
    sequence); stopping at the fixture's stop_at returns the fixture's iterations / calls and s to 1e-10
    (tests/golden/stpcg_user_stop.json), on all eight cases of the fixture.
    The TNT part runs a fixed number of outer iterations (max_iterations = 4, fewer than either side needs to converge):
    it shows one call per outer iteration with the caller's own object, on the host and on the device; it does not
    show that an uncapped device run stops after the same number of outer iterations as the reference."""
    import oracle_py
    fx = golden("stpcg_user_stop.json")
    pr = oracle_py.stpcg_stop_problem(fx["n"], fx["seed"])
    for c in fx["cases"]:
        Minv = pr["Minv"] if c["precon"] else None
        h = args.counting(0, 0, pr["g"], pr["D"], Minv, stop_at=c["stop_at"])
        d = args.counting(1, 0, pr["g"], pr["D"], Minv, stop_at=c["stop_at"])
        assert h["rc"] == 0 and d["rc"] == 0, (h["err"], d["err"])
        assert (h["iterations"], h["counter"]) == (c["iterations"], c["calls"])
        assert (d["iterations"], d["counter"]) == (c["iterations"], c["calls"]), c["stop_at"]
        assert d["counters"]["fused_stpcg_solves"] == 1 and d["counters"]["generic_stpcg_solves"] == 0
        # (the never-stopped preconditioned case runs into the 100-iteration limit with the residual stagnating at
        # rounding level 30 iterations earlier; from there on CG amplifies last-bit differences of the inner products:
        # 1e-5 on the iterate there, as tests/test_gpu_stpcg_observer.py and tests/test_gpu_templates.py ask)
        tol = 1e-10 if c["iterations"] < 100 else 1e-5
        es = np.abs(d["s"] - np.array(c["s"])).max() / max(1e-300, np.abs(c["s"]).max())
        em = abs(d["M_norm"] - c["M_norm"]) / max(1e-300, c["M_norm"])
        print("stop_at", c["stop_at"], "precon", c["precon"], "iterations", d["iterations"], "s", es, "|s|_M", em)
        assert es <= tol and em <= tol
    # (4 outer iterations: the host run needs 6 to reach its gradient tolerance, so the count is the cap's on both sides)
    h = args.counting(0, 1, pr["g"], pr["D"], max_iterations=4)
    d = args.counting(1, 1, pr["g"], pr["D"], max_iterations=4)
    assert h["rc"] == 0 and d["rc"] == 0, (h["err"], d["err"])
    print("TNT with a counting pack: host", h["counter"], "device", d["counter"], d["counters"])
    assert d["counter"] == h["counter"] == h["iterations"] == d["iterations"] == 4
    assert d["counters"]["fused_stpcg_solves"] == d["iterations"] and d["counters"]["generic_stpcg_solves"] == 0
    assert abs(d["M_norm"] - h["M_norm"]) <= 1e-10 * abs(h["M_norm"])


def test_a_wrapped_hessian_stays_generic_with_a_pack(args, oracle, golden, capfd, monkeypatch):
    """With a pack and the Hessian wrapped in a lambda the generic counters rise, and the note names the wrapper, not
    the pack"""
    g, n, p, rowptr, col, val, X0, prm = _stiefel_fixture(golden, oracle)
    monkeypatch.setenv("MI355OPT_WARN_GENERIC", "1")
    capfd.readouterr()
    b = args.tnt_stiefel(n, p, rowptr, col, val, X0, prm, pack=1, wrap_hessian=True)
    err = capfd.readouterr().err
    assert b["rc"] == 0, b.get("err")
    kb, outer = b["counters"], b["outer_iterations"]
    print(kb, "\n", err.strip())
    assert outer == g["outer_iterations"] and abs(b["f"] - g["f"]) < 1e-12
    assert kb["generic_stpcg_solves"] == outer and kb["fused_stpcg_solves"] == 0
    assert kb["generic_trial_steps"] == outer and kb["fused_trial_steps"] == 0
    assert err.count("STPCG on MI355::DeviceVector runs the GENERIC loop") == 1
    assert "MI355::DeviceOperator" in err and "wrapped in a lambda" in err
    assert "Args" not in err and "extra arguments" not in err
