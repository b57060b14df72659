"""Riemannian::TNT on MI355::PoseGraph through the header layer (tests/cpp/harness_pgo.cpp): convergence on a noise-free
graph, the tagged run against TNT's statement sequence, the fusion counters, refine() and the pipeline of
examples/pose_graph_refinement.cpp."""
import functools

import numpy as np
import pytest

import so3_cases as sc
from harness_pgo_py import PIPELINE, PLAIN, REFINE, TAGGED, PgoHarness
from optimization_amd import workloads as wl

pytestmark = pytest.mark.gpu
LD = np.longdouble
GRADIENT_TOLERANCE = 1e-6    # SmoothOptimizerParams' default
STATUS_GRADIENT = 0          # TNTStatus::Gradient


@functools.lru_cache(maxsize=None)
def graph(N, noise):
    """ring with chords; measurements = the truth's relative poses (+ noise: 0.02 rad, 0.02 length units); the start 0.1 rad and
    0.1 length units from the truth: dict(N, ei, ej, Rt, tt, kappa, tau, x0, Rtrue, ttrue)"""
    ei, ej = (a.astype(np.int64) for a in wl.pose_graph(N, seed=N + 1)[:2])
    E = ei.size
    rng = np.random.Generator(np.random.PCG64(100 + N))
    Rtrue = sc.round_orth(sc.exp_ld(rng.normal(size=(N, 3)) * 1.5)).astype(LD)
    ttrue = (rng.normal(size=(N, 3)) * 3.0).astype(LD)
    RiT = np.swapaxes(Rtrue[ei], 1, 2)
    nR = sc.exp_ld(rng.normal(size=(E, 3)) * (0.02 if noise else 0.0))
    Rt = sc.round_orth(RiT @ Rtrue[ej] @ nR)
    tt = (np.einsum("eab,eb->ea", RiT, ttrue[ej] - ttrue[ei]) + rng.normal(size=(E, 3)) * (0.02 if noise else 0.0)).astype(np.float64)
    d = rng.normal(size=(N, 3))
    R0 = sc.round_orth(Rtrue @ sc.exp_ld(0.1 * d / np.linalg.norm(d, axis=1)[:, None]))
    d = rng.normal(size=(N, 3))
    t0 = (ttrue + 0.1 * d / np.linalg.norm(d, axis=1)[:, None]).astype(np.float64)
    return dict(N=N, ei=ei.astype(np.int32), ej=ej.astype(np.int32), Rt=Rt.reshape(E, 9), tt=tt, kappa=np.ones(E), tau=np.ones(E),
                x0=np.concatenate([R0.ravel(), t0.ravel()]), Rtrue=Rtrue, ttrue=ttrue)


def run(mode, g, **kw):
    r = PgoHarness().run(mode, g["N"], g["ei"], g["ej"], g["Rt"], g["tt"], g["kappa"], g["tau"], g["x0"], **kw)
    assert r["rc"] == 0, r["err"]
    return r


def test_tnt_recovers_the_relative_poses_of_a_noise_free_graph():
    g = graph(200, False)
    N, ei, ej = g["N"], g["ei"], g["ej"]
    r = run(TAGGED, g)
    print(f"outer {r['outer']}, inner {r['inner_total']}, f0 {r['f0']:.3e}, f {r['f']:.3e}, |grad| {r['gradient_norm']:.2e}")
    assert r["status"] == STATUS_GRADIENT and r["gradient_norm"] < GRADIENT_TOLERANCE
    R = r["x"][:9 * N].reshape(N, 3, 3).astype(LD)
    t = r["x"][9 * N:].reshape(N, 3).astype(LD)
    RiT = np.swapaxes(R[ei], 1, 2)
    dR = np.abs(RiT @ R[ej] - g["Rt"].reshape(-1, 3, 3).astype(LD)).max()
    dt = np.abs(np.einsum("eab,eb->ea", RiT, t[ej] - t[ei]) - g["tt"].astype(LD)).max()
    print(f"relative rotations {float(dR):.2e}, relative translations {float(dt):.2e}")
    assert dR <= 1e-8 and dt <= 1e-8
    # one fused inner solve and one trial read-back per outer iteration, nothing generic
    assert r["fused_stpcg"] == r["outer"] == r["fused_trials"] and r["generic_stpcg"] == r["generic_trials"] == 0
    assert r["generic_inner_products"] <= 2, "inner products beyond |g| and |M^-1 g| at the start point"
    # host synchronisations: the trial's read-back per outer iteration, plus the start (f(x0) and the two gradient norms)
    assert r["syncs"] <= r["outer"] + 4, (r["syncs"], r["outer"])


def test_tagged_run_equals_the_statement_sequence_on_a_noisy_graph():
    g = graph(200, True)
    a, b = run(TAGGED, g), run(PLAIN, g)
    print(f"tagged: outer {a['outer']}, inner {a['inner']}, syncs {a['syncs']}; plain: outer {b['outer']}, syncs {b['syncs']}")
    assert a["status"] == b["status"] == STATUS_GRADIENT
    assert a["outer"] == b["outer"] and a["inner"] == b["inner"] and a["accepted"] == b["accepted"]
    assert abs(a["f"] - b["f"]) <= 1e-12 * abs(b["f"])
    assert a["fused_trials"] == a["outer"] and a["generic_trials"] == 0 and a["fused_stpcg"] == a["outer"]
    assert b["fused_trials"] == 0 and b["generic_trials"] == b["outer"], "the plain run did not take the statement sequence"
    assert a["syncs"] < b["syncs"]


def test_refine_is_the_explicit_tnt_call():
    g = graph(200, True)
    a, b = run(TAGGED, g), run(REFINE, g)
    assert np.array_equal(a["x"].view(np.uint64), b["x"].view(np.uint64))
    assert (a["f"], a["gradient_norm"], a["outer"], a["inner_total"], a["status"]) == \
           (b["f"], b["gradient_norm"], b["outer"], b["inner_total"], b["status"])


def test_pipeline_ends_no_higher_than_its_chordal_start():
    g = graph(300, True)
    r = run(PIPELINE, g)
    print(f"chordal start f0 {r['f0']:.6e} -> refined f {r['f']:.6e} in {r['outer']} outer iterations")
    assert r["f"] <= r["f0"] and r["status"] == STATUS_GRADIENT
    assert r["fused_trials"] == r["outer"] and r["generic_trials"] == 0
