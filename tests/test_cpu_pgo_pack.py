"""The host-side layout of the joint pose-graph problem (optimization_amd/csrc/pgo_pack.h: pgo_pack) without a GPU, through
the library's host-only debug entry mi_debug_pgo_pack (capi.pgo_pack), against the numpy restatement of
tests/pgo_cases.py and against structural facts that hold whatever the restatement says.  Everything is compared exactly.
Also here: the compiled forms of the new kernels, the untouched kernel sets of the neighbouring units, and the symbols."""
import ctypes as C
import os

import numpy as np
import pytest

import pgo_cases as pc
from optimization_amd import capi
from test_cpu_kernel_resources import HIPCC, _resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = tuple(dict.fromkeys(pc.FD_CASES + pc.GPU_CASES)) + ("ring1025", "hub1500")


def problem(name):
    if name == "ring1025":     # beyond the 1024-node window of the degree sort
        N, (ei, ej) = 1025, pc._ring_chords(1025, seed=3)
    elif name == "hub1500":    # a hub whose degree exceeds the window
        N, (ei, ej) = 1500, pc._hub(1500, True)
    else:
        return pc.problem(name)
    rng = np.random.Generator(np.random.PCG64(N))
    E = ei.size
    return dict(name=name, N=N, ei=ei.astype(np.int32), ej=ej.astype(np.int32), Rt=rng.normal(size=(E, 9)),
                tt=rng.normal(size=(E, 3)), kappa=rng.normal(size=E), tau=np.where(np.arange(E) % 5 == 0, 0.0, np.linspace(0.5, 2, E)))


def pack(p, **over):
    q = dict(p, **over)
    return capi.pgo_pack(q["N"], q["ei"], q["ej"], q["Rt"], q["tt"], q["kappa"], q["tau"])


def refusal(p, **over):
    with pytest.raises(capi.MiError) as e:
        pack(p, **over)
    assert e.value.status == 1
    return str(e.value).split(": ", 1)[1]


@pytest.mark.parametrize("name", CASES)
def test_layout_against_the_restatement(name):
    p = problem(name)
    got, ref = pack(p), pc.layout(p)
    for k in capi.PGO_PACK_COUNTS:
        assert got[k] == ref[k], (k, got[k], ref[k])
    for k, dtype in capi.PGO_PACK_ARRAYS:
        assert got[k].dtype == dtype and got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), k
    # what holds whatever the restatement says: every edge in exactly two slots with opposite direction bits, each carrying
    # the edge's own measurements (the rotation transposed at the first node); zeros on padding
    N, ei, ej, E = p["N"], p["ei"], p["ej"], p["ei"].size
    perm, sp, words, padded = got["perm"], got["slice_ptr"], got["slot"], got["padded"]
    assert padded == 64 * sp[got["nslices"]] and np.array_equal(np.sort(perm[perm >= 0]), np.arange(N))
    owner = np.repeat(perm.reshape(-1, 64), np.diff(sp), axis=0).ravel()
    k = np.concatenate([np.repeat(np.arange(n), 64) for n in np.diff(sp)] + [np.zeros(0, dtype=np.int64)])
    cnt = np.bincount(np.concatenate([ei, ej]).astype(np.int64), minlength=N)
    entry = (owner >= 0) & (k < cnt[np.maximum(owner, 0)])
    seen = np.zeros((E, 2), dtype=np.int64)
    Rt = np.asarray(p["Rt"]).reshape(E, 3, 3)
    for slot in np.flatnonzero(entry):
        e, first = int(words[slot] >> 1), int(words[slot] & 1)
        seen[e, first] += 1
        assert owner[slot] == (ei[e] if first else ej[e]) and got["nbr"][slot] == (ej[e] if first else ei[e])
        assert got["kinc"][slot] == p["kappa"][e] and got["tauinc"][slot] == p["tau"][e]
        kk, lane = slot // 64, slot % 64
        assert np.array_equal(got["tinc"][(kk * 3 + np.arange(3)) * 64 + lane], np.asarray(p["tt"])[e])
        assert np.array_equal(got["rinc"][(kk * 9 + np.arange(9)) * 64 + lane], (Rt[e].T if first else Rt[e]).ravel())
    assert np.all(seen == 1) and got["nnzb"] == 2 * E == int(entry.sum())
    pad = ~entry
    for stream in ("kinc", "tauinc", "slot"):
        assert np.all(got[stream][:padded][pad] == 0)
    for stream, comps in (("rinc", 9), ("tinc", 3)):
        a = got[stream][:comps * padded].reshape(-1, comps, 64)
        assert np.all(a[np.broadcast_to(pad.reshape(-1, 1, 64), a.shape)] == 0)
    assert np.array_equal(got["nbr"][pad], np.where(owner[pad] >= 0, owner[pad], N - 1))


def test_refusals_keep_their_messages():
    p = pc.problem("ring65")
    N, ei, ej, E = p["N"], p["ei"], p["ej"], p["ei"].size
    for e, (a, b) in ((0, (-1, 3)), (5, (2, N)), (E - 1, (N, 2)), (3, (4, -7))):
        bi, bj = ei.copy(), ej.copy()
        bi[e], bj[e] = a, b
        assert refusal(p, ei=bi, ej=bj) == "edge %d has an end point outside [0, N)" % e
    bi, bj = ei.copy(), ej.copy()
    bi[11] = bj[11] = 9
    assert refusal(p, ei=bi, ej=bj) == "edge 11 is a self-loop"
    for bad in (np.inf, -np.inf, np.nan):
        bt = p["tt"].copy()
        bt[17, 2] = bad
        assert refusal(p, tt=bt) == "edge 17 has a non-finite translation"
    for bad in (-1e-300, -1.0, np.inf, np.nan):
        bw = p["tau"].copy()
        bw[E - 2] = bad
        assert refusal(p, tau=bw) == "edge %d has a negative or non-finite weight" % (E - 2)
    none = np.zeros(0, dtype=np.int32)
    for n in (0, 2 ** 31 - 1, 2 ** 40):
        assert refusal(dict(N=n, ei=none, ej=none, Rt=np.zeros((0, 9)), tt=np.zeros((0, 3)), kappa=np.zeros(0),
                            tau=np.zeros(0))) == "bad number of poses"
    # kappa is taken as mi_so3n_create takes w: negative, infinite and NaN values pass through
    bk = p["kappa"].copy()
    bk[:3] = (-1.0, np.inf, np.nan)
    got = pack(p, kappa=bk)
    assert np.isnan(got["kinc"]).sum() == 2 and np.isinf(got["kinc"]).sum() == 2


def test_packer_is_clean_under_asan_and_ubsan():
    """tests/cpp/sanitize_pgo_pack.cpp: the packer on these kinds of graphs and every refused problem, with its own main,
    built with g++ -fsanitize=address,undefined and run on the CPU; any report (a leak on a failure path too) fails it.
    Skipped only where the host has no sanitizer runtime."""
    from optimization_amd import build as b
    try:
        exe = b.build_sanitize_pgo_pack(run=True)
    except b.SanitizerUnavailable as e:
        pytest.skip(str(e))
    assert os.path.exists(exe)


# (TotalSGPRs, VGPRs, compiler's waves/SIMD, scratch bytes per lane) of the new kernels as this commit compiles them,
# recorded (the occupancy is the compiler's figure for the kernel's launch bounds)
PGO_FIGURES = {
    "k_pgo_model<0>": (61, 120, 4, 0),    # objective only
    "k_pgo_model<1>": (79, 210, 2, 0),    # model
    "k_pgo_model<2>": (63, 162, 3, 0),    # gradient only
    "k_pgo_model<3>": (70, 160, 3, 0),    # gradient and inverse blocks
    "k_pgo_hvp<false>": (44, 94, 5, 0),
    "k_pgo_hvp<true>": (48, 114, 4, 0),
    "k_pgo_retract": (78, 60, 8, 0),
    "k_pgo_sum_slots": (14, 3, 8, 0),
}
# the kernels of every other unit as the parent commit d1a4301 compiles them: (count, first 16 hex digits of the SHA-256 of the
# sorted demangled names joined by newlines); pgo_trans.hip's four also by name
PGO_TRANS_KERNELS = ["k_pgo_max_rows", "k_pgo_trans_residual<false>", "k_pgo_trans_residual<true>", "k_pgo_trans_rhs"]
PARENT_KERNELS = {
    "blas1.hip": (18, "f7097ed2df2eb758"), "comm.hip": (20, "5d79d7da715fc496"), "context.hip": (1, "57c412c8379e0d80"),
    "kkt.hip": (11, "9527a63da5758942"), "lobpcg.hip": (109, "3f2be4f9ac0f40a5"), "lsqr.hip": (14, "86ed040c031599ca"),
    "ops.hip": (2, "f195b203be0202c7"), "pgo_trans.hip": (4, "d030b5f6b47551cd"), "so3.hip": (60, "aaeb5f99e91964e8"),
    "sparse.hip": (77, "c8ad20a69b5313c9"), "stiefel.hip": (258, "29b67dda134e04cd"),
    "stiefel_tall.hip": (12, "1f27c4144b509a91"), "stpcg.hip": (91, "9260323a5261b398"),
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_new_kernels_compile_without_scratch_and_the_neighbours_keep_their_kernels():
    r = _resource_usage("pgo.hip")
    want = [f"k_pgo_model<{f}>" for f in range(4)] + ["k_pgo_hvp<false>", "k_pgo_hvp<true>", "k_pgo_retract", "k_pgo_sum_slots"]
    assert sorted(r) == sorted(want), sorted(r)
    for name in want:
        sg, vg, occ, scratch = r[name]
        print(name, "SGPRs", sg, "VGPRs", vg, "waves/SIMD", occ, "scratch", scratch)
        assert scratch == 0, name + " spills"
    assert r == PGO_FIGURES
    # the 1024-thread passes need 4 waves per SIMD to be resident at all, the streaming retraction all 8 within 80 SGPRs
    assert r["k_pgo_hvp<true>"][2] >= 4 and r["k_pgo_hvp<false>"][2] >= 4
    assert r["k_pgo_retract"][0] <= 80 and r["k_pgo_retract"][1] <= 64 and r["k_pgo_retract"][2] == 8
    # the gradient-only and objective-only forms are no heavier than the model form
    for f in (0, 2, 3):
        assert r[f"k_pgo_model<{f}>"][1] <= r["k_pgo_model<1>"][1]
    assert sorted(_resource_usage("pgo_trans.hip")) == PGO_TRANS_KERNELS


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_every_other_unit_keeps_the_kernels_of_the_parent():
    """kernel counts and names of every .hip unit but pgo.hip, unit by unit (compiled side by side)"""
    import concurrent.futures
    import glob
    import hashlib
    csrc = os.path.join(ROOT, "optimization_amd", "csrc")
    units = sorted(os.path.basename(p) for p in glob.glob(os.path.join(csrc, "*.hip")))
    assert units == sorted(list(PARENT_KERNELS) + ["pgo.hip"]), "a unit appeared or went"

    def digest(unit):
        names = sorted(_resource_usage(unit))
        return unit, names, (len(names), hashlib.sha256("\n".join(names).encode()).hexdigest()[:16])
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        for unit, names, got in ex.map(digest, PARENT_KERNELS):
            assert got == PARENT_KERNELS[unit], (unit, got, PARENT_KERNELS[unit])
            if unit == "pgo_trans.hip":
                assert names == PGO_TRANS_KERNELS


def test_header_library_and_binding_agree_on_the_new_entry_points():
    L = capi.load()
    hdr = open(os.path.join(ROOT, "include", "mi355opt.h")).read()
    for name in ("mi_pgo_create", "mi_pgo_destroy", "mi_pgo_objective", "mi_pgo_gradient", "mi_pgo_model", "mi_pgo_retract",
                 "mi_pgo_trial", "mi_debug_pgo_pack", "mi_debug_pgo_blocks"):
        assert ("MI_API int %s(" % name) in hdr and hasattr(L, name), name
    # appended to the kernel enumeration: no earlier value moves
    assert capi.KERNELS[:26] == ["none", "cg_init", "cg_dot3", "cg_scalar_a", "cg_update", "cg_scalar_b", "cg_pupdate", "csr_spmm",
                                 "stiefel_spmm_gram", "stiefel_gram_reduce", "stiefel_finish_dots", "stiefel_retract",
                                 "bsr3_spmv_dots", "blas1", "lobpcg_gram", "lobpcg_update", "lobpcg_residual",
                                 "stiefel_hess_fused", "comm_allreduce", "comm_halo", "so3_grad", "so3_residual", "so3_jac",
                                 "so3_jact", "so3_edge_weight", "so3_inc_reweight"]
    assert capi.KERNELS[26:] == ["pgo_model", "pgo_grad", "pgo_hvp", "pgo_retract"]
    for i, k in enumerate(capi.KERNELS):
        assert L.mi_kernel_name(i) == k.encode()
    assert L.mi_kernel_name(len(capi.KERNELS)) == b"?"
    for meth in ("objective", "gradient", "model", "retract", "trial", "blocks", "info"):
        assert callable(getattr(capi.Pgo, meth))


def test_new_entry_points_have_no_cpu_fallback():
    """Without a device every compute entry point answers MI_ERR_NO_DEVICE (no context, hence no problem, can exist); the
    packer's debug entry is host-only and works."""
    L = capi.load()
    if capi.device_count() > 0:
        pytest.skip("a GPU is present")
    out = (C.c_double * 6)()
    assert L.mi_pgo_create(None, 1, 0, None, None, None, None, None, None, None) == 4
    assert b"no HIP device" in L.mi_last_error()
    assert L.mi_pgo_objective(None, None, out) == 4 and L.mi_pgo_gradient(None, None, None) == 4
    assert L.mi_pgo_model(None, None, None, None, None) == 4 and L.mi_pgo_retract(None, None, None, None) == 4
    assert L.mi_pgo_trial(None, None, None, None, 1, None, out) == 4 and out[0] == 0.0
    assert pack(pc.problem("n2"))["nnzb"] == 4
