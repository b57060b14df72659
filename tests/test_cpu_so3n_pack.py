"""The host-side layout of an SO(3)^N problem (optimization_amd/csrc/so3_pack.h: so3_pack) without a GPU: the header
compiled by g++ on its own behind a small extern "C" shim, against a numpy restatement of the layout comment at the top
of so3.hip and against structural facts that hold whatever the restatement says.

Integer arrays, counts, weights and the 9-component streams are compared exactly; quaternion streams to 4e-16 per
component (unit vectors from correctly rounded operations; the margin allows one contracted multiply-add)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOW = 1024
SIZES = (1, 63, 64, 65, 1025, 2049)
VARIANTS = ("plain", "negative_weight", "reflection", "off_orthogonal")

SHIM = r'''
#include "so3_pack.h"
static mi::So3Pack P;
static std::string err;
extern "C" int pack(size_t N, size_t E, const int32_t *ei, const int32_t *ej, const double *Rt, const double *w, int no_quat,
                    int sort_nbr) {
  P = mi::So3Pack();
  err.clear();
  return mi::so3_pack(N, E, ei, ej, Rt, w, no_quat != 0, sort_nbr != 0, P, err);
}
extern "C" const char *pack_error() { return err.c_str(); }
extern "C" void pack_counts(size_t *o) {
  o[0] = P.N; o[1] = P.E; o[2] = P.nslices; o[3] = P.nnzb; o[4] = P.padded; o[5] = P.sinc_quat; o[6] = P.w_nonneg;
}
extern "C" size_t pack_array(int which, const void **data) {
  switch (which) {
    case 0: *data = P.slice_ptr.data(); return P.slice_ptr.size();
    case 1: *data = P.perm.data(); return P.perm.size();
    case 2: *data = P.nbr.data(); return P.nbr.size();
    case 3: *data = P.sinc.data(); return P.sinc.size();
    case 4: *data = P.winc.data(); return P.winc.size();
    case 5: *data = P.h_ij.data(); return P.h_ij.size();
    case 6: *data = P.h_Se.data(); return P.h_Se.size();
    case 7: *data = P.h_w.data(); return P.h_w.size();
    default: *data = P.h_slot.data(); return P.h_slot.size();
  }
}
'''
ARRAYS = (("slice_ptr", np.int64), ("perm", np.int32), ("nbr", np.int32), ("sinc", np.float64), ("winc", np.float64),
          ("h_ij", np.int32), ("h_Se", np.float64), ("h_w", np.float64), ("h_slot", np.uint32))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("so3_pack")
    src, so = d / "pack_host.cpp", d / "libpack_host.so"
    src.write_text(SHIM)
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-shared", "-fPIC", "-I",
                        os.path.join(ROOT, "optimization_amd", "csrc"), str(src), "-o", str(so)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]
    L = C.CDLL(str(so))
    L.pack.argtypes = [C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.pack_error.restype = C.c_char_p
    L.pack_array.restype = C.c_size_t
    return L


def pack(L, N, ei, ej, Rt, w, no_quat=False, sort_nbr=False):
    """(status, message or dict of counts and arrays) of so3_pack"""
    ei, ej = np.ascontiguousarray(ei, dtype=np.int32), np.ascontiguousarray(ej, dtype=np.int32)
    Rt, w = np.ascontiguousarray(Rt, dtype=np.float64), np.ascontiguousarray(w, dtype=np.float64)
    st = L.pack(N, ei.size, ei.ctypes.data, ej.ctypes.data, Rt.ctypes.data, w.ctypes.data, int(no_quat), int(sort_nbr))
    if st != 0:
        return st, L.pack_error().decode()
    counts = (C.c_size_t * 7)()
    L.pack_counts(counts)
    out = dict(zip(("N", "E", "nslices", "nnzb", "padded", "sinc_quat", "w_nonneg"), (int(c) for c in counts)))
    for which, (name, dtype) in enumerate(ARRAYS):
        p = C.c_void_p()
        n = L.pack_array(which, C.byref(p))
        out[name] = np.ctypeslib.as_array(C.cast(p, C.POINTER(np.ctypeslib.as_ctypes_type(dtype))), (n,)).copy() if n else \
            np.zeros(0, dtype)
    return 0, out


# ---- the problems ----
def rotations(rng, n):
    Q, Rr = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    Q = Q * np.sign(np.diagonal(Rr, axis1=1, axis2=2))[:, None, :]
    Q[:, :, 2] *= np.linalg.det(Q)[:, None]
    return Q


def problem(N, variant="plain"):
    """A ring over every node but one (which stays isolated), about N / 2 random chords, the first edge once more in the
    opposite direction (a pair of parallel edges), one zero weight; weights in [0.5, 2]."""
    rng = np.random.Generator(np.random.PCG64(1000 + N))
    iso = N // 2
    nodes = np.array([i for i in range(N) if i != iso or N < 4], dtype=np.int64)
    n = nodes.size
    ei, ej = [], []
    if n >= 3:
        ei += list(nodes)
        ej += list(np.roll(nodes, -1))
    elif n == 2:
        ei, ej = [int(nodes[0])], [int(nodes[1])]
    if n >= 4:
        a, b = rng.integers(0, n, size=N // 2), rng.integers(0, n, size=N // 2)
        keep = a != b
        ei += list(nodes[a[keep]])
        ej += list(nodes[b[keep]])
        ei.append(ej[0])
        ej.append(ei[0])
    ei, ej = np.array(ei, dtype=np.int32), np.array(ej, dtype=np.int32)
    E = ei.size
    Rt = rotations(rng, E).reshape(E, 9) if E else np.zeros((0, 9))
    w = rng.uniform(0.5, 2.0, size=E)
    if E > 3:
        w[3] = 0.0
    if E and variant == "negative_weight":
        w[E // 2] = -0.25
    if E and variant == "reflection":
        Rt[E // 3] = (Rt[E // 3].reshape(3, 3) @ np.diag([1.0, 1.0, -1.0])).ravel()
    if E and variant == "off_orthogonal":
        Rt[E // 3, 4] += 1e-12
    return ei, ej, Rt, w


# ---- the layout, restated from the comment at the top of so3.hip ----
def to_quat(M):
    """(n, 9) rotations -> (n, 4) unit quaternions (w, x, y, z), Shepperd's choice of the largest of trace, m00, m11, m22"""
    m = M.reshape(-1, 3, 3)
    tr = m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2]
    which = np.argmax(np.stack([tr, m[:, 0, 0], m[:, 1, 1], m[:, 2, 2]], axis=1), axis=1)
    q = np.zeros((m.shape[0], 4))
    a, b, c = m[:, 2, 1] - m[:, 1, 2], m[:, 0, 2] - m[:, 2, 0], m[:, 1, 0] - m[:, 0, 1]
    s01, s02, s12 = m[:, 0, 1] + m[:, 1, 0], m[:, 0, 2] + m[:, 2, 0], m[:, 1, 2] + m[:, 2, 1]
    forms = (np.stack([1 + tr, a, b, c], axis=1),
             np.stack([a, 1 + m[:, 0, 0] - m[:, 1, 1] - m[:, 2, 2], s01, s02], axis=1),
             np.stack([b, s01, 1 - m[:, 0, 0] + m[:, 1, 1] - m[:, 2, 2], s12], axis=1),
             np.stack([c, s02, s12, 1 - m[:, 0, 0] - m[:, 1, 1] + m[:, 2, 2]], axis=1))
    for k, f in enumerate(forms):
        q[which == k] = f[which == k]
    return q / np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])[:, None]


def all_rotations(Rt):
    m = Rt.reshape(-1, 3, 3)
    gram = np.swapaxes(m, 1, 2) @ m - np.eye(3)
    return bool(np.all(np.abs(gram) <= 1e-13) and np.all(np.linalg.det(m) > 0))


def layout(N, ei, ej, Rt, w, no_quat=False, sort_nbr=False):
    E = ei.size
    # the incidences of every node in edge order: (edge, the node is the first node of the edge, neighbour)
    inc = [[] for _ in range(N)]
    for e in range(E):
        inc[ej[e]].append((e, 0, int(ei[e])))
        inc[ei[e]].append((e, 1, int(ej[e])))
    if sort_nbr:
        inc = [sorted(l, key=lambda t: t[2]) for l in inc]   # (stable)
    deg = np.array([len(l) for l in inc], dtype=np.int64)
    nslices = (N + 63) // 64
    perm = np.full(nslices * 64, -1, dtype=np.int32)
    for w0 in range(0, N, WINDOW):
        w1 = min(N, w0 + WINDOW)
        perm[w0:w1] = w0 + np.argsort(-deg[w0:w1], kind="stable")
    width = [max([deg[i] for i in perm[64 * s:64 * s + 64] if i >= 0], default=0) for s in range(nslices)]
    slice_ptr = np.concatenate([[0], np.cumsum(width)]).astype(np.int64)
    padded = 64 * int(slice_ptr[-1])
    quat = (not no_quat) and all_rotations(Rt)
    comps = 4 if quat else 9
    Rt3 = Rt.reshape(-1, 3, 3)
    nbr = np.zeros(padded, dtype=np.int32)
    winc = np.zeros(max(1, padded))
    sinc = np.zeros(max(1, padded * comps))
    h_slot = np.zeros(padded, dtype=np.uint32)
    nnzb = 0
    for s in range(nslices):
        for lane in range(64):
            node = perm[64 * s + lane]
            for k in range(width[s]):
                slot = (slice_ptr[s] + k) * 64 + lane
                nbr[slot] = node if node >= 0 else N - 1
                if node >= 0 and k < deg[node]:
                    e, first, j = inc[node][k]
                    nbr[slot], winc[slot], h_slot[slot] = j, w[e], (e << 1) | first
                    S = (Rt3[e].T if first else Rt3[e]).reshape(1, 9)        # as THIS node uses the measurement
                    S = to_quat(S) if quat else S
                    sinc[((slice_ptr[s] + k) * comps + np.arange(comps)) * 64 + lane] = S[0]
                    nnzb += 1
    h_Se = (to_quat(Rt) if quat else Rt.reshape(E, 9)).T.ravel() if E else np.zeros(0)
    return dict(N=N, E=E, nslices=nslices, nnzb=nnzb, padded=padded, sinc_quat=int(quat), w_nonneg=int(np.all(w >= 0)),
                slice_ptr=slice_ptr, perm=perm, nbr=nbr, sinc=sinc, winc=winc, h_ij=np.stack([ei, ej], axis=1).ravel(),
                h_Se=h_Se, h_w=w.copy(), h_slot=h_slot)


def check(got, ref):
    for k in ("N", "E", "nslices", "nnzb", "padded", "sinc_quat", "w_nonneg"):
        assert got[k] == ref[k], (k, got[k], ref[k])
    for k in ("slice_ptr", "perm", "nbr", "h_slot", "h_ij", "winc", "h_w"):
        assert got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), k
    for k in ("sinc", "h_Se"):
        assert got[k].shape == ref[k].shape, k
        if ref["sinc_quat"]:
            assert np.abs(got[k] - ref[k]).max(initial=0.0) <= 4e-16, (k, float(np.abs(got[k] - ref[k]).max()))
        else:
            assert np.array_equal(got[k], ref[k]), k


def check_structure(got, ei, ej, w):
    """what holds whatever the restatement says"""
    N, E, padded, sp, perm = got["N"], got["E"], got["padded"], got["slice_ptr"], got["perm"]
    assert padded == 64 * sp[got["nslices"]] and sp[0] == 0 and np.all(np.diff(sp) >= 0)
    assert np.array_equal(np.sort(perm[perm >= 0]), np.arange(N)) and np.all(perm[:N] >= 0)
    deg = np.bincount(np.concatenate([ei, ej]).astype(np.int64), minlength=N)
    words = got["h_slot"]
    # the owner of every slot and its position k in the owner's row: a node's first deg slots are its incidences
    owner = np.repeat(perm.reshape(-1, 64), np.diff(sp), axis=0).ravel()
    k = np.concatenate([np.repeat(np.arange(n), 64) for n in np.diff(sp)] + [np.zeros(0, dtype=np.int64)])
    entry = (owner >= 0) & (k < deg[np.maximum(owner, 0)])
    # every edge in exactly two slots with opposite direction bits, at its two end points
    seen = np.zeros((E, 2), dtype=np.int64)
    for slot in np.flatnonzero(entry):
        e, first = int(words[slot] >> 1), int(words[slot] & 1)
        seen[e, first] += 1
        assert owner[slot] == (ei[e] if first else ej[e]) and got["nbr"][slot] == (ej[e] if first else ei[e])
        assert got["winc"][slot] == w[e]
    assert np.all(seen == 1), "an edge is not in exactly two slots with opposite direction bits"
    assert got["nnzb"] == 2 * E == int(entry.sum())
    # padding: weight 0, word 0, neighbour = own node (the last node for the lanes nobody owns)
    pad = ~entry
    assert np.all(got["winc"][:padded][pad] == 0) and np.all(words[pad] == 0)
    assert np.array_equal(got["nbr"][pad], np.where(owner[pad] >= 0, owner[pad], N - 1))
    # degrees non-increasing in perm order inside every window of 1024 nodes
    for w0 in range(0, N, WINDOW):
        d = deg[perm[w0:min(N, w0 + WINDOW)]]
        assert np.all(np.diff(d) <= 0)


@pytest.mark.parametrize("no_quat", (False, True))
@pytest.mark.parametrize("sort_nbr", (False, True))
@pytest.mark.parametrize("N", SIZES)
def test_layout_against_the_restatement(lib, N, sort_nbr, no_quat):
    ei, ej, Rt, w = problem(N)
    st, got = pack(lib, N, ei, ej, Rt, w, no_quat=no_quat, sort_nbr=sort_nbr)
    assert st == 0, got
    assert got["sinc_quat"] == (0 if no_quat else 1)
    check(got, layout(N, ei, ej, Rt, w, no_quat=no_quat, sort_nbr=sort_nbr))
    check_structure(got, ei, ej, w)


@pytest.mark.parametrize("variant", VARIANTS[1:])
@pytest.mark.parametrize("N", (65, 1025))
def test_weights_and_measurements_that_change_the_form(lib, N, variant):
    ei, ej, Rt, w = problem(N, variant)
    st, got = pack(lib, N, ei, ej, Rt, w)
    assert st == 0, got
    assert got["w_nonneg"] == (0 if variant == "negative_weight" else 1)
    # a reflection, and a measurement 1e-12 off orthogonality, switch the problem to the 9-component form
    assert got["sinc_quat"] == (1 if variant == "negative_weight" else 0)
    check(got, layout(N, ei, ej, Rt, w))
    check_structure(got, ei, ej, w)


@pytest.mark.parametrize("N", SIZES)
def test_no_edges(lib, N):
    none = np.zeros(0, dtype=np.int32)
    st, got = pack(lib, N, none, none, np.zeros((0, 9)), np.zeros(0))
    assert st == 0, got
    assert got["padded"] == 0 and got["nnzb"] == 0 and got["sinc_quat"] == 1 and got["w_nonneg"] == 1
    assert np.array_equal(got["perm"][:N], np.arange(N)) and np.all(got["slice_ptr"] == 0)
    assert got["sinc"].size == 1 and got["winc"].size == 1          # (never an empty upload)
    check(got, layout(N, none, none, np.zeros((0, 9)), np.zeros(0)))


def test_invalid_problems_keep_their_messages(lib):
    ei, ej, Rt, w = problem(65)
    for e, (a, b) in ((0, (-1, 3)), (5, (2, 65)), (7, (65, 2)), (ei.size - 1, (9, 9)), (3, (4, -7))):
        bi, bj = ei.copy(), ej.copy()
        bi[e], bj[e] = a, b
        assert pack(lib, 65, bi, bj, Rt, w) == (1, "edge %d has invalid endpoints" % e)
    none = np.zeros(0, dtype=np.int32)
    for N in (0, 2 ** 31 - 1, 2 ** 31, 2 ** 40):
        assert pack(lib, N, none, none, np.zeros((0, 9)), np.zeros(0)) == (1, "bad number of rotations")
    assert pack(lib, 2, [0], [0], np.eye(3).reshape(1, 9), [1.0]) == (1, "edge 0 has invalid endpoints")


def test_packer_is_clean_under_asan_and_ubsan():
    """tests/cpp/sanitize_so3_pack.cpp: the packer on these kinds of graphs and on every refused problem, with its own
    main, built with g++ -fsanitize=address,undefined and run on the CPU; any report (a leak on a failure path too)
    fails it.  Skipped only where the host has no sanitizer runtime."""
    from optimization_amd import build as b
    try:
        exe = b.build_sanitize_so3_pack(run=True)
    except b.SanitizerUnavailable as e:
        pytest.skip(str(e))
    assert os.path.exists(exe)
