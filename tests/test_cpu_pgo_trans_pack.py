"""The host-side layout of the pose-graph translation solve (optimization_amd/csrc/pgo_trans_pack.h: pgo_trans_pack) without
a GPU: the header compiled by g++ on its own behind a small extern "C" shim, against the numpy restatement of
tests/pgo_trans_cases.py and against structural facts that hold whatever the restatement says.

Everything is compared exactly: the integer arrays, the merged Laplacian values (summed in edge order on both sides), dinv
and the slot streams."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pgo_trans_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHIM = r'''
#include "pgo_trans_pack.h"
static mi::PgoTransPack P;
static std::string err;
extern "C" int pack(size_t N, size_t E, const int32_t *ei, const int32_t *ej, const double *tt, const double *tau, long long anchor) {
  P = mi::PgoTransPack();
  err.clear();
  return mi::pgo_trans_pack(N, E, ei, ej, tt, tau, anchor, P, err);
}
extern "C" const char *pack_error() { return err.c_str(); }
extern "C" void pack_counts(size_t *o) {
  o[0] = P.N; o[1] = P.E; o[2] = P.nslices; o[3] = P.nnzb; o[4] = P.padded; o[5] = P.nnz; o[6] = P.anchor;
}
extern "C" size_t pack_array(int which, const void **data) {
  switch (which) {
    case 0: *data = P.rowptr.data(); return P.rowptr.size();
    case 1: *data = P.col.data(); return P.col.size();
    case 2: *data = P.val.data(); return P.val.size();
    case 3: *data = P.dinv.data(); return P.dinv.size();
    case 4: *data = P.slice_ptr.data(); return P.slice_ptr.size();
    case 5: *data = P.perm.data(); return P.perm.size();
    case 6: *data = P.nbr.data(); return P.nbr.size();
    case 7: *data = P.slot.data(); return P.slot.size();
    case 8: *data = P.tinc.data(); return P.tinc.size();
    case 9: *data = P.tauinc.data(); return P.tauinc.size();
    case 10: *data = P.e_ij.data(); return P.e_ij.size();
    case 11: *data = P.e_t.data(); return P.e_t.size();
    default: *data = P.e_tau.data(); return P.e_tau.size();
  }
}
'''
COUNTS = ("N", "E", "nslices", "nnzb", "padded", "nnz", "anchor")
ARRAYS = (("rowptr", np.int32), ("col", np.int32), ("val", np.float64), ("dinv", np.float64), ("slice_ptr", np.int64),
          ("perm", np.int32), ("nbr", np.int32), ("slot", np.uint32), ("tinc", np.float64), ("tauinc", np.float64),
          ("e_ij", np.int32), ("e_t", np.float64), ("e_tau", np.float64))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("pgo_trans_pack")
    src, so = d / "pack_host.cpp", d / "libpack_host.so"
    src.write_text(SHIM)
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", "-I",
                        os.path.join(ROOT, "optimization_amd", "csrc"), str(src), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]
    L = C.CDLL(str(so))
    L.pack.argtypes = [C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong]
    L.pack_error.restype = C.c_char_p
    L.pack_array.restype = C.c_size_t
    return L


def pack(L, N, ei, ej, tt, tau, anchor):
    """(status, message or dict of counts and arrays) of pgo_trans_pack"""
    ei, ej = np.ascontiguousarray(ei, dtype=np.int32), np.ascontiguousarray(ej, dtype=np.int32)
    tt, tau = np.ascontiguousarray(tt, dtype=np.float64), np.ascontiguousarray(tau, dtype=np.float64)
    st = L.pack(N, ei.size, ei.ctypes.data, ej.ctypes.data, tt.ctypes.data, tau.ctypes.data, anchor)
    if st != 0:
        return st, L.pack_error().decode()
    counts = (C.c_size_t * len(COUNTS))()
    L.pack_counts(counts)
    out = dict(zip(COUNTS, (int(c) for c in counts)))
    for which, (name, dtype) in enumerate(ARRAYS):
        p = C.c_void_p()
        n = L.pack_array(which, C.byref(p))
        out[name] = np.ctypeslib.as_array(C.cast(p, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), (n,)).copy() if n else \
            np.zeros(0, dtype)
    return 0, out


def check_structure(got, N, ei, ej, tau, anchor):
    """what holds whatever the restatement says"""
    rowptr, col, val = got["rowptr"], got["col"], got["val"]
    deg = pc.weighted_degree(N, ei, ej, tau)
    unit = deg == 0
    unit[anchor] = True
    A = np.zeros((N, N))
    rows = np.repeat(np.arange(N), np.diff(rowptr))
    A[rows, col] = val
    assert rowptr[0] == 0 and rowptr[N] == col.size == val.size == got["nnz"]
    for i in range(N):    # columns ascending, no duplicates, a diagonal entry in every row
        c = col[rowptr[i]:rowptr[i + 1]]
        assert np.all(np.diff(c) > 0) and i in c
    assert np.array_equal(A, A.T), "L_a is not symmetric entry by entry"
    assert np.all(val[rows != col] != 0), "an explicit zero off the diagonal"
    # unit rows and columns where specified, and only there
    for i in np.flatnonzero(unit):
        assert rowptr[i + 1] - rowptr[i] == 1 and A[i, i] == 1.0 and np.count_nonzero(A[:, i]) == 1
    assert np.array_equal(got["dinv"], np.repeat(1.0 / np.diag(A), 3))
    # L_a 1 = e_anchor + e_zero-degree, up to the anchor's column: a regular row sums to the weight it shares with the anchor
    to_anchor = np.zeros(N)
    np.add.at(to_anchor, ei[ej == anchor], tau[ej == anchor])
    np.add.at(to_anchor, ej[ei == anchor], tau[ei == anchor])
    ones = A @ np.ones(N)
    assert np.all(ones[unit] == 1.0)
    assert np.all(np.abs(ones[~unit] - to_anchor[~unit]) <= 64 * np.finfo(float).eps * deg[~unit])
    # the slot streams: every edge in exactly two slots with opposite direction bits; tauinc = tau but for the unit rows
    perm, sp, words, padded = got["perm"], got["slice_ptr"], got["slot"], got["padded"]
    assert padded == 64 * sp[got["nslices"]] and np.array_equal(np.sort(perm[perm >= 0]), np.arange(N))
    owner = np.repeat(perm.reshape(-1, 64), np.diff(sp), axis=0).ravel()
    k = np.concatenate([np.repeat(np.arange(n), 64) for n in np.diff(sp)] + [np.zeros(0, dtype=np.int64)])
    cnt = np.bincount(np.concatenate([ei, ej]).astype(np.int64), minlength=N)
    entry = (owner >= 0) & (k < cnt[np.maximum(owner, 0)])
    seen = np.zeros((ei.size, 2), dtype=np.int64)
    tt = got["e_t"].reshape(3, -1).T
    for slot in np.flatnonzero(entry):
        e, first = int(words[slot] >> 1), int(words[slot] & 1)
        seen[e, first] += 1
        assert owner[slot] == (ei[e] if first else ej[e]) and got["nbr"][slot] == (ej[e] if first else ei[e])
        assert got["tauinc"][slot] == (0.0 if unit[owner[slot]] else tau[e])
        kk, lane = slot // 64, slot % 64
        assert np.array_equal(got["tinc"][(kk * 3 + np.arange(3)) * 64 + lane], tt[e])
    assert np.all(seen == 1) and got["nnzb"] == 2 * ei.size == int(entry.sum())
    pad = ~entry
    assert np.all(got["tauinc"][:padded][pad] == 0) and np.all(words[:padded][pad] == 0)
    assert np.array_equal(got["nbr"][pad], np.where(owner[pad] >= 0, owner[pad], N - 1))


@pytest.mark.parametrize("kind", pc.TAU_KINDS)
@pytest.mark.parametrize("name", tuple(pc.CASES))
def test_layout_against_the_restatement(lib, name, kind):
    N, ei, ej, tt, tau, _ = pc.problem(name, kind)
    anchors = pc.anchors(name, kind)
    if name in ("isolated_1500",):
        assert any(pc.weighted_degree(N, ei, ej, tau)[a] == 0 for a in anchors), "no zero-degree anchor in this case"
    for anchor in anchors:
        st, got = pack(lib, N, ei, ej, tt, tau, anchor)
        assert st == 0, got
        ref = pc.layout(name, kind, anchor)
        for k in COUNTS:
            assert got[k] == ref[k], (anchor, k, got[k], ref[k])
        for k, _ in ARRAYS:
            assert got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), (anchor, k)
    check_structure(got, N, ei, ej, tau, anchors[-1])


def test_a_node_whose_every_weight_is_zero_gets_the_unit_row(lib):
    N, ei, ej, tt, tau, _ = pc.problem("ring_chords_1025", "linspace")
    tau = tau.copy()
    tau[(ei == 70) | (ej == 70)] = 0.0
    st, got = pack(lib, N, ei, ej, tt, tau, 3)
    assert st == 0, got
    r = got["rowptr"]
    assert r[71] - r[70] == 1 and got["col"][r[70]] == 70 and got["val"][r[70]] == 1.0
    assert np.all(got["dinv"][210:213] == 1.0) and not np.any(got["col"][np.arange(got["nnz"]) != r[70]] == 70)
    check_structure(got, N, ei, ej, tau, 3)


def test_refusals_keep_their_messages(lib):
    N, ei, ej, tt, tau, _ = pc.problem("ring_chords_1023", "linspace")
    E = ei.size
    for anchor in (-1, N, 2 ** 40):
        assert pack(lib, N, ei, ej, tt, tau, anchor) == (1, "anchor %d is outside [0, N)" % anchor)
    for e, (a, b) in ((0, (-1, 3)), (5, (2, N)), (E - 1, (N, 2)), (3, (4, -7))):
        bi, bj = ei.copy(), ej.copy()
        bi[e], bj[e] = a, b
        assert pack(lib, N, bi, bj, tt, tau, 0) == (1, "edge %d has an end point outside [0, N)" % e)
    bi, bj = ei.copy(), ej.copy()
    bi[11] = bj[11] = 9
    assert pack(lib, N, bi, bj, tt, tau, 0) == (1, "edge 11 is a self-loop")
    for bad in (np.inf, -np.inf, np.nan):
        bt = tt.copy()
        bt[17, 2] = bad
        assert pack(lib, N, ei, ej, bt, tau, 0) == (1, "edge 17 has a non-finite translation")
    for bad in (-1e-300, -1.0, np.inf, np.nan):
        bw = tau.copy()
        bw[E - 2] = bad
        assert pack(lib, N, ei, ej, tt, bw, 0) == (1, "edge %d has a negative or non-finite weight" % (E - 2))
    none = np.zeros(0, dtype=np.int32)
    for n in (0, 2 ** 31 - 1, 2 ** 40):
        assert pack(lib, n, none, none, np.zeros((0, 3)), np.zeros(0), 0) == (1, "bad number of poses")


def test_packer_is_clean_under_asan_and_ubsan():
    """tests/cpp/sanitize_pgo_trans_pack.cpp: the packer on these kinds of graphs, every anchor kind and every refused
    problem, with its own main, built with g++ -fsanitize=address,undefined and run on the CPU; any report (a leak on a
    failure path too) fails it.  Skipped only where the host has no sanitizer runtime."""
    from optimization_amd import build as b
    try:
        exe = b.build_sanitize_pgo_trans_pack(run=True)
    except b.SanitizerUnavailable as e:
        pytest.skip(str(e))
    assert os.path.exists(exe)
