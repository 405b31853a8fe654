"""Mel-cepstral distortion along a DTW path (csrc/dtw.h through include/mtts.h: mtts_dtw_*; meta_tts_amd/evaluation.py:
MelCepstralDistortion, ObjectiveEvaluation).  CPU tests run the device code through the SIMT emulator; the `gpu` parameter of the same
tests runs it on the MI355X.

The definition is the project's own (include/mtts.h), restated in float64 numpy in the same summation order in tests/mcd_oracle.py.
Device and oracle are both float64, so the gates are worst-case rounding bounds, not measured figures:
  * cepstra: a sum of n_mel products accumulates at most (n_mel + 1) 2^-53 sum |B m| of rounding error; x 4 for the compiler's freedom to
    contract a multiply-add (which changes single roundings, not the bound's order): 4 (n_mel + 1) 2^-53 sum_n |B[k][n] m[n]| per output.
  * D, MCD, cents RMSE: D is a sum of at most Ta + Tb - 1 distances, each a square root of K squared differences: 4 (Ta + Tb + K) 2^-53
    relative, derived the same way.  L, the counts and the path are exact, which needs every decision of the oracle's path to be
    safe from rounding: the oracle reports its smallest decision margin (best against second-best predecessor along the path,
    relative to D) and every case below asserts it above 1e-9 — seven orders above the gate.  The (7, 7) identical case has margin 0 by
    construction and pins the tie rule instead."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
import mcd_oracle as O
from meta_tts_amd import _lib
from meta_tts_amd import evaluation as E
from meta_tts_amd.engine import MttsError

U = 2.0 ** -53
MARGIN = 4.0
SHOW = bool(os.environ.get("MTTS_SELFTEST_MCD_SHOW"))    # print every measured figure next to its gate (python -m pytest -s)


def show(*a):
    if SHOW:
        print("[mcd]", *a)


@pytest.fixture(scope="module", params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def lib_path(request):
    return ge.build_emulator() if request.param == "emu" else ge.build_device()


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Dev:
    """A raw mtts_dtw handle."""

    def __init__(self, lib_path, n_mel=80, n_coef=13, max_frames=320, max_cells=1 << 24, max_pairs=64, basis=True):
        self.lib = _lib.load(lib_path)
        self.n_mel, self.n_coef = n_mel, n_coef
        self.h = C.c_void_p()
        if self.lib.mtts_dtw_create(n_mel, n_coef, max_frames, max_cells, max_pairs, 0, C.byref(self.h)) != 0:
            raise MttsError(self.lib.mtts_dtw_last_error(None).decode())
        if basis:
            self.check(self.lib.mtts_dtw_load_basis(self.h, _ptr(np.ascontiguousarray(O.dct_basis(n_mel, n_coef)))))

    def check(self, rc):
        if rc != 0:
            assert rc < 0
            raise MttsError(self.lib.mtts_dtw_last_error(self.h).decode())

    def cepstra(self, mels):
        T = np.asarray([len(m) for m in mels], np.int32)
        packed = np.ascontiguousarray(np.concatenate(mels), np.float32)
        out = np.empty((int(T.sum()), self.n_coef))
        self.check(self.lib.mtts_dtw_cepstra(self.h, len(T), _ptr(T), _ptr(packed), _ptr(out)))
        return np.split(out, np.cumsum(T)[:-1])

    def raw(self, Ta, mel_a, Tb, mel_b, fTa=None, f0_a=None, fTb=None, f0_b=None, out=None, L=None, path=None):
        """The entry itself, every argument as given (None = NULL); returns its return code."""
        i32 = lambda v: None if v is None else np.ascontiguousarray(v, np.int32)   # noqa: E731
        Ta, Tb, fTa, fTb = i32(Ta), i32(Tb), i32(fTa), i32(fTb)
        return self.lib.mtts_dtw_mcd_batch(self.h, len(Ta), _ptr(Ta), _ptr(mel_a), _ptr(Tb), _ptr(mel_b), _ptr(fTa), _ptr(f0_a), _ptr(fTb), _ptr(f0_b), _ptr(out),
                                           _ptr(L), _ptr(path))

    def mcd(self, mels_a, mels_b, f0_a=None, f0_b=None):
        """-> (out [n][6], [path (L, 2)]); the unused tail of every path slot must hold -1."""
        Ta, Tb = [len(m) for m in mels_a], [len(m) for m in mels_b]
        pa, pb = (np.ascontiguousarray(np.concatenate(m), np.float32) for m in (mels_a, mels_b))
        fa = fb = fTa = fTb = None
        if f0_a is not None:
            fa, fb = (np.ascontiguousarray(np.concatenate(f), np.float64) for f in (f0_a, f0_b))
            fTa, fTb = [len(f) for f in f0_a], [len(f) for f in f0_b]
        cap = np.asarray(Ta) + np.asarray(Tb) - 1
        out, L, path = np.full((len(Ta), 6), -7.0), np.empty(len(Ta), np.int32), np.empty((int(cap.sum()), 2), np.int32)
        self.check(self.raw(Ta, pa, Tb, pb, fTa, fa, fTb, fb, out, L, path))
        starts = np.concatenate([[0], np.cumsum(cap)[:-1]])
        assert np.array_equal(L, out[:, 1].astype(np.int32))
        for s, n, c in zip(starts, L, cap):
            assert (path[s + n:s + c] == -1).all()
        return out, [path[s:s + n] for s, n in zip(starts, L)]

    def close(self):
        self.lib.mtts_dtw_destroy(self.h)


# ---- inputs and their oracle results, computed once --------------------------------------------------------------------------------------------
B80 = O.dct_basis(80, 13)
# name -> (Ta, Tb, kind, seed).  random: two unrelated sequences; stretch: B is a time-stretched noisy copy of A (the realistic pair).
# Seeds chosen on the CPU so that every case's decision margin is above 1e-9 (asserted in case()); none is skipped.
CASES = {
    "1x1": (1, 1, "random", 0), "1x5": (1, 5, "random", 0), "5x1": (5, 1, "random", 0),
    "7x300": (7, 300, "random", 0), "7x300s": (7, 300, "stretch", 0),                 # a diagonal shorter than a wavefront
    "257x300": (257, 300, "random", 0), "257x300s": (257, 300, "stretch", 0),         # a diagonal longer than one workgroup pass
    "320x320": (320, 320, "random", 0), "320x320s": (320, 320, "stretch", 0),         # max_frames itself
    "300x7": (300, 7, "stretch", 0),                                                  # more rows than columns
    "513x9": (513, 9, "random", 0), "1025x9": (1025, 9, "random", 0),                 # the sweep's 1024- and 2048-row LDS variants
}
_cache = {}


def f0_track(T, seed):
    """Voiced stretches of 3 .. 12 frames at 80 .. 400 Hz with unvoiced gaps of 0 .. 6 frames."""
    r = np.random.default_rng(1000 + seed)
    f = np.zeros(T)
    t = int(r.integers(0, 4))
    while t < T:
        n = int(r.integers(3, 13))
        f[t:t + n] = r.uniform(80.0, 400.0) * np.exp(0.02 * np.cumsum(r.standard_normal(len(f[t:t + n]))))
        t += n + int(r.integers(0, 7))
    return f


def case(name):
    if name not in _cache:
        ta, tb, kind, seed = CASES[name]
        a = O.random_mel(ta, 80, seed=10 * seed + 1)
        b = O.random_mel(tb, 80, seed=10 * seed + 2) if kind == "random" else O.stretched_copy(a, tb, seed=10 * seed + 3)
        fa, fb = f0_track(ta, seed), f0_track(tb, seed + 50)
        out, path, margin = O.mcd(a, b, B80, fa, fb)
        assert margin > 1e-9, (name, margin)
        _cache[name] = dict(a=a, b=b, fa=fa, fb=fb, out=out, path=path, margin=margin, gate=MARGIN * (ta + tb + 13) * U)
    return _cache[name]


def handle_for(lib_path, name):
    return Dev(lib_path, max_frames=2048 if max(CASES[name][:2]) > 320 else 320)


def close_to(got, want, gate):
    return abs(got - want) <= gate * abs(want)


# ---- 1. the oracle ----------------------------------------------------------------------------------------------------------------------------
def test_oracle_basis_is_scipy():
    """Rows 1 .. K of scipy's orthonormal DCT-II to 1e-15 (measured 1.1e-16), and orthonormal rows."""
    fft = pytest.importorskip("scipy.fft")
    for n_mel, k in ((80, 13), (8, 7), (80, 34)):
        ref = fft.dct(np.eye(n_mel), type=2, norm="ortho", axis=0)[1:k + 1]
        got = O.dct_basis(n_mel, k)
        show("basis", n_mel, k, np.abs(got - ref).max())
        assert np.abs(got - ref).max() <= 1e-15
        assert np.abs(got @ got.T - np.eye(k)).max() <= 1e-14


def test_oracle_dp_is_brute_force():
    """The DP's end value is the cheapest of all 129 monotone paths over 4 x 5 frames, and its path's own cost is that value."""
    for seed in range(5):
        a, b = O.cepstra(O.random_mel(4, 80, seed), B80), O.cepstra(O.random_mel(5, 80, 100 + seed), B80)
        d = O.frame_distance(a, b)
        D, frm = O.dtw_tables(d)
        path, _, _ = O.backtrack(D, frm)
        cost, count = O.brute_force(d)
        assert count == 129 and abs(D[-1, -1] - cost) <= 1e-14 * cost
        assert abs(sum(d[i, j] for i, j in path) - cost) <= 1e-14 * cost
        assert path[0] == (0, 0) and path[-1] == (3, 4) and all(0 <= c[0] - p[0] <= 1 and 0 <= c[1] - p[1] <= 1 and c != p for p, c in zip(path, path[1:]))


# ---- 2. cepstra ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mel,n_coef", [(80, 13), (8, 7)])
def test_cepstra(lib_path, n_mel, n_coef):
    """1, 3 and 300 frames, each alone and packed together, against the oracle; gate per output 4 (n_mel + 1) 2^-53 sum_n |B[k][n] m[n]| (a
    worst-case rounding bound of the n_mel-term float64 sum, margin 4 for the compiler's FMA contraction).  A row's cepstra are the same
    bits alone and packed.  Measured: emulator 0 (the same operations in the same order), MI355X at most 0.005 of the gate at n_mel = 80 and 0.05 at n_mel = 8."""
    B = O.dct_basis(n_mel, n_coef)
    mels = [O.random_mel(T, n_mel, seed=T) for T in (1, 3, 300)]
    d = Dev(lib_path, n_mel, n_coef)
    try:
        alone = [d.cepstra([m])[0] for m in mels]
        packed = d.cepstra(mels)
    finally:
        d.close()
    for m, c1, c2 in zip(mels, alone, packed):
        want, gate = O.cepstra(m, B), MARGIN * (n_mel + 1) * U * O.cepstra_scale(m, B)
        show("cepstra", n_mel, len(m), "worst error / gate", float((np.abs(c1 - want) / gate).max()))
        assert c1.shape == (len(m), n_coef) and (np.abs(c1 - want) <= gate).all()
        assert c1.tobytes() == c2.tobytes()


# ---- 3. DTW -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_dtw_against_oracle(lib_path, name):
    """D, MCD and cents RMSE within 4 (Ta + Tb + K) 2^-53 relative of the oracle; L, both counts and the path exactly.  Without F0 the same
    D, L, MCD and path, and NaN in columns 3 .. 5.  Margins of the cases (oracle): 4.2e-6 .. 1.3e-4, see case().  Measured relative error
    of D: emulator 0, MI355X at most 7e-16."""
    c = case(name)
    d = handle_for(lib_path, name)
    try:
        out, paths = d.mcd([c["a"]], [c["b"]], [c["fa"]], [c["fb"]])
        out0, paths0 = d.mcd([c["a"]], [c["b"]])
    finally:
        d.close()
    got, want = out[0], c["out"]
    show(name, "margin", c["margin"], "gate", c["gate"], "rel err D", abs(got[0] - want[0]) / want[0], "cents", got[4], want[4])
    for col in (0, 2, 4):
        assert close_to(got[col], want[col], c["gate"]) or (np.isnan(want[col]) and np.isnan(got[col])), (col, got[col], want[col])
    assert got[1] == want[1] and got[3] == want[3] and got[5] == want[5]
    assert np.array_equal(paths[0], c["path"])
    assert np.array_equal(out0[0, :3], got[:3]) and np.isnan(out0[0, 3:]).all() and np.array_equal(paths0[0], c["path"])
    if min(CASES[name][:2]) >= 7:
        assert want[3] > 0 and want[5] > 0              # the tracks overlap and disagree somewhere


def test_identical_inputs_take_the_diagonal(lib_path):
    """(7, 7), the same frames on both sides: every d(i, i) is 0 and so is every D on the diagonal; off it D > 0, so at each cell the
    diagonal predecessor ties with nothing smaller and the tie rule (diagonal first) must keep the path on it: D = 0, L = 7."""
    a = O.random_mel(7, 80, seed=77)
    flat = np.repeat(a[:1], 7, axis=0)                   # all frames equal: EVERY predecessor ties at 0, only the rule decides
    d = Dev(lib_path)
    try:
        out, paths = d.mcd([a, flat], [a, flat])
    finally:
        d.close()
    for p in range(2):
        assert out[p, 0] == 0.0 and out[p, 1] == 7.0 and out[p, 2] == 0.0
        assert np.array_equal(paths[p], np.stack([np.arange(7), np.arange(7)], axis=1))
    want, path, _ = O.mcd(flat, flat, B80)
    assert want[0] == 0.0 and len(path) == 7


def test_bit_identity(lib_path):
    """One pair alone, as element 0, 2 and 4 of a batch of 5 mixed shapes, and on a handle whose max_cells cuts that batch into 3 chunks:
    the out row and the path are the same bytes everywhere; so are the other pairs' between the one-chunk and the three-chunk call."""
    c = case("257x300s")
    others = [case("7x300"), case("1x5"), case("300x7")]
    alone_h = Dev(lib_path)
    try:
        out1, path1 = alone_h.mcd([c["a"]], [c["b"]], [c["fa"]], [c["fb"]])
        results = {}
        for pos in (0, 2, 4):
            batch = list(others[:2]) + [others[2], others[0]]
            batch.insert(pos, c)
            results[pos] = alone_h.mcd([x["a"] for x in batch], [x["b"] for x in batch], [x["fa"] for x in batch], [x["fb"] for x in batch])
            assert results[pos][0][pos].tobytes() == out1[0].tobytes() and results[pos][1][pos].tobytes() == path1[0].tobytes()
    finally:
        alone_h.close()
    batch = list(others[:2]) + [others[2], others[0]]
    batch.insert(2, c)
    cells = [len(x["a"]) * len(x["b"]) for x in batch]          # 2100, 5, 77100, 2100, 2100
    chunked = Dev(lib_path, max_cells=cells[2] + cells[3])       # -> [0, 1], [2, 3], [4]
    try:
        out3, path3 = chunked.mcd([x["a"] for x in batch], [x["b"] for x in batch], [x["fa"] for x in batch], [x["fb"] for x in batch])
    finally:
        chunked.close()
    assert cells[0] + cells[1] + cells[2] > cells[2] + cells[3]  # pair 2 does not fit behind pairs 0 and 1, nor pair 4 behind 2 and 3
    assert out3.tobytes() == results[2][0].tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(path3, results[2][1]))
    by_pairs = Dev(lib_path, max_pairs=2)                        # the same cut by the pair limit: [0, 1], [2, 3], [4]
    try:
        out2, path2 = by_pairs.mcd([x["a"] for x in batch], [x["b"] for x in batch], [x["fa"] for x in batch], [x["fb"] for x in batch])
    finally:
        by_pairs.close()
    assert out2.tobytes() == out3.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(path2, path3))


# ---- 4. F0 ----------------------------------------------------------------------------------------------------------------------------------
def test_f0_known_figures(lib_path):
    """Identical mels (the path is the diagonal) with tracks built by hand over 40 frames: frames 0 .. 9 unvoiced on both sides, 10 .. 29
    voiced on both with A exactly 100 cents above B, 30 .. 34 voiced on A only, 35 .. 37 on B only, 38 .. 39 unvoiced: 20 voiced steps at
    100 cents RMSE (within the DTW gate: fb is a power of two, so fa / fb is the rounded 2^(1/12) itself), 8 mismatches."""
    T = 40
    a = O.random_mel(T, 80, seed=5)
    fb, fa = np.zeros(T), np.zeros(T)
    fb[10:30] = 128.0
    fa[10:30] = 128.0 * 2.0 ** (100.0 / 1200.0)
    fa[30:35] = 150.0
    fb[35:38] = 210.0
    d = Dev(lib_path)
    try:
        out, paths = d.mcd([a], [a], [fa], [fb])
    finally:
        d.close()
    gate = MARGIN * (T + T + 13) * U
    show("f0 cents", out[0, 4], "gate", gate)
    assert out[0, 0] == 0.0 and out[0, 1] == T and out[0, 3] == 20.0 and out[0, 5] == 8.0
    assert close_to(out[0, 4], 100.0, gate)
    want, _, _ = O.mcd(a, a, B80, fa, fb)
    assert close_to(out[0, 4], want[4], gate) and want[3] == 20.0 and want[5] == 8.0
    # no step with both sides voiced: the counts stand, the RMSE is NaN
    d = Dev(lib_path)
    try:
        out, _ = d.mcd([a], [a], [np.where(np.arange(T) < 5, 100.0, 0.0)], [np.zeros(T)])
    finally:
        d.close()
    assert out[0, 3] == 0.0 and np.isnan(out[0, 4]) and out[0, 5] == 5.0


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals(lib_path):
    """Every refusal returns < 0 with its message, writes nothing to `out` (nothing ran), leaves the handle usable, and destroy after a
    refusal is clean (on the emulator: no allocation survives the handle)."""
    lib = _lib.load(lib_path)
    live = getattr(lib, "emu_live_allocs", None)
    if live is not None:
        live.restype = C.c_longlong
        before = live()
    for kw, msg in ((dict(n_mel=1), "n_mel = 1 outside"), (dict(n_mel=129), "n_mel = 129 outside"), (dict(n_coef=0), "n_coef = 0 outside 1 .. 34"), (dict(n_coef=35), "n_coef = 35 outside"),
                    (dict(n_mel=8, n_coef=8), "n_coef = 8 must be less than n_mel = 8"), (dict(max_frames=2049), "max_frames = 2049 outside 1 .. 2048"),
                    (dict(max_frames=0), "max_frames = 0 outside"), (dict(max_cells=0), "max_cells = 0 outside"), (dict(max_pairs=0), "max_pairs = 0 outside")):
        with pytest.raises(MttsError, match=msg):
            Dev(lib_path, **kw)
    a, b = O.random_mel(7, 80, 1), O.random_mel(9, 80, 2)
    fa, fb = f0_track(7, 1), f0_track(9, 2)
    nobasis = Dev(lib_path, basis=False)
    out = np.full((2, 6), -7.0)
    assert nobasis.raw([7], a, [9], b, out=out) < 0 and "no basis loaded (mtts_dtw_load_basis)" in lib.mtts_dtw_last_error(nobasis.h).decode()
    with pytest.raises(MttsError, match="no basis loaded"):
        nobasis.cepstra([a])
    nobasis.close()                                            # destroy straight after a refusal
    d = Dev(lib_path, max_frames=320, max_cells=1000)
    try:
        two_a, two_b = np.concatenate([a, a]), np.concatenate([b, b])
        long_b = O.random_mel(321, 80, 3)
        wide_a, wide_b = O.random_mel(32, 80, 4), O.random_mel(32, 80, 5)
        bad_a = a.copy()
        bad_a[1, 5] = np.nan
        jobs = [
            (([7, 0], two_a, [9, 9], two_b), "pair 1: frames_a = 0: at least 1 frame"),
            (([7, 7], two_a, [9, -1], two_b), "pair 1: frames_b = -1: at least 1 frame"),
            (([7], a, [321], long_b), "pair 0: frames_b = 321 exceeds the handle's max_frames = 320"),
            (([7, 32], np.concatenate([a, wide_a]), [9, 32], np.concatenate([b, wide_b])), "pair 1: 32 x 32 = 1024 cells exceed the handle's max_cells = 1000"),
            (([7, 7], two_a, [9, 9], two_b, [7, 6], np.concatenate([fa, fa]), [9, 9], np.concatenate([fb, fb])), r"pair 1: f0_frames_a = 6 but frames_a = 7 \(an F0 track has one value per mel frame\)"),
            (([7], a, [9], b, [7], fa, [8], fb), "pair 0: f0_frames_b = 8 but frames_b = 9"),
            (([7], a, [9], b, [7], fa, None, None), r"f0_a given without f0_b \(both F0 tracks or neither\)"),
            (([7], a, [9], b, None, None, [9], fb), "f0_b given without f0_a"),
            (([7], a, [9], b, [7], -fa, [9], fb), "f0_a holds a negative or non-finite value"),
            (([7], bad_a, [9], b), r"mel_a holds a non-finite value \(row 1\)"),
        ]
        for args, msg in jobs:
            out[:] = -7.0
            rc = d.raw(*args, out=out)
            text = lib.mtts_dtw_last_error(d.h).decode()
            assert rc < 0 and (out == -7.0).all(), msg
            assert re.search(msg, text), (msg, text)
            got, _ = d.mcd([a], [b], [fa], [fb])               # the handle is as usable as before
            assert got[0, 1] >= 9
        assert d.raw([7], a, [9], b, out=None) < 0 and "NULL" in lib.mtts_dtw_last_error(d.h).decode()
        with pytest.raises(MttsError, match="utterance 1: n_frames = 321 exceeds the handle's max_frames = 320"):
            d.cepstra([a, long_b])
        assert len(d.cepstra([a])[0]) == 7
    finally:
        d.close()
    d = Dev(lib_path, max_pairs=1)
    try:
        with pytest.raises(MttsError, match="n_utts = 3 exceeds 2 x the handle's max_pairs = 1"):
            d.cepstra([a, a, a])
        assert len(d.cepstra([a, b])) == 2
    finally:
        d.close()
    assert lib.mtts_dtw_mcd_batch(None, 1, *[None] * 11) < 0 and "NULL handle" in lib.mtts_dtw_last_error(None).decode()
    if live is not None:
        assert live() == before


# ---- 6. the host classes ------------------------------------------------------------------------------------------------------------------------
def test_mcd_batch_is_the_raw_entry(lib_path):
    """MelCepstralDistortion over lists of ragged arrays: the raw entry's bytes; its basis is the oracle's; cepstra() is the kernel entry."""
    names = ["7x300", "1x5", "257x300s"]
    cs = [case(n) for n in names]
    d = Dev(lib_path)
    try:
        want, want_paths = d.mcd([c["a"] for c in cs], [c["b"] for c in cs], [c["fa"] for c in cs], [c["fb"] for c in cs])
        want_cep = d.cepstra([cs[0]["a"]])[0]
    finally:
        d.close()
    m = E.MelCepstralDistortion(max_frames=320, lib_path=lib_path)
    try:
        assert m.basis.tobytes() == np.ascontiguousarray(B80).tobytes() and m.COLUMNS[2] == "MCD"
        got, paths = m.mcd_batch([c["a"] for c in cs], [c["b"].tolist() for c in cs], [c["fa"] for c in cs], [c["fb"] for c in cs], return_paths=True)
        assert got.tobytes() == want.tobytes() and all(np.array_equal(p, q) for p, q in zip(paths, want_paths))
        plain = m.mcd_batch([c["a"] for c in cs], [c["b"] for c in cs])
        assert np.array_equal(plain[:, :3], want[:, :3]) and np.isnan(plain[:, 3:]).all()
        assert m.cepstra([cs[0]["a"]])[0].tobytes() == want_cep.tobytes()
        with pytest.raises(ValueError, match=r"mels_a\[0\] has shape \(7, 79\)"):
            m.mcd_batch([cs[0]["a"][:, :79]], [cs[0]["b"]])
        with pytest.raises(MttsError, match="f0_frames_a = 6 but frames_a = 7"):
            m.mcd_batch([cs[0]["a"]], [cs[0]["b"]], [cs[0]["fa"][:6]], [cs[0]["fb"]])
    finally:
        m.close()
    with pytest.raises(MttsError, match="max_frames = 4096 outside"):
        E.MelCepstralDistortion(max_frames=4096, lib_path=lib_path)


SR, HOP = 22050, 256


def _tone(freq, seconds, seed):
    t = np.arange(int(SR * seconds)) / SR
    r = np.random.default_rng(seed)
    return (0.4 * np.sin(2 * np.pi * freq * t) + 0.1 * np.sin(2 * np.pi * 2 * freq * t) + 0.002 * r.standard_normal(len(t))).astype(np.float32)


def _result_tree(tmp_path, n_speaker=2, n_sample=2):
    """A result tree in the reference's layout with empty files; the waveforms live in the returned dict and come through `wav_loader`.
    recon = the real wav itself (MCD 0); the synthesis = another length and pitch."""
    dirs = {k: tmp_path / k for k in ("recon", "real", "meta")}
    wavs, sq = {}, []
    for s in range(n_speaker):
        for k in range(n_sample):
            data_id, qid = s * n_sample + k, f"spk{s:02d}_utt{k}"
            sq.append({"qry_id": [qid]})
            real = dirs["real"] / f"spk{s:02d}" / f"{qid}.wav"
            recon = dirs["recon"] / "audio" / "Testing" / f"test_{data_id:03d}" / f"{qid}.recon.wav"
            syn = dirs["meta"] / "audio" / "Testing" / f"test_{data_id:03d}" / f"{qid}.step_5-FTstep_5.synth.wav"
            for p in (real, recon, syn):
                p.parent.mkdir(parents=True, exist_ok=True)
                p.write_bytes(b"")
            wavs[str(real)] = wavs[str(recon)] = _tone(110.0 * (1 + data_id), 0.3, data_id)
            wavs[str(syn)] = _tone(117.0 * (1 + data_id), 0.34, 100 + data_id)
    (dirs["recon"] / "test_SQids.json").write_text(json.dumps(sq))
    cfg = E.EvalConfig("Toy", {k: str(v) for k, v in dirs.items()}, n_speaker, n_sample, [("meta", [5])], work_dir=str(tmp_path))
    return cfg, wavs


def test_objective_evaluation(lib_path, tmp_path):
    """2 speakers x 2 samples of 0.3 s tones (26 mel frames; the syntheses 30): the tables, the summary file and the reload; recon against
    the identical real wav is MCD 0 with every voiced frame at 0 cents; the synthesis table equals mcd_batch on the same features."""
    from meta_tts_amd.audio.pitch import PitchExtractor
    from meta_tts_amd.audio.stft import TacotronSTFT
    cfg, wavs = _result_tree(tmp_path)
    stft = TacotronSTFT(1024, HOP, 1024, 80, SR, 0.0, 8000.0, max_samples=SR, lib_path=lib_path)
    pitch = PitchExtractor(SR, HOP, lib_path=lib_path, max_samples=SR)
    mcd = E.MelCepstralDistortion(max_frames=64, lib_path=lib_path)
    try:
        ev = E.ObjectiveEvaluation(cfg, mcd, stft, pitch=pitch, wav_loader=lambda p: wavs[p])
        tables = ev.get_mcd()
        assert list(tables) == ["recon", "meta_step5"] and all(t.shape == (4, 6) for t in tables.values())
        rec, syn = tables["recon"], tables["meta_step5"]
        assert (rec[:, 0] == 0).all() and (rec[:, 1] == 26).all() and (rec[:, 2] == 0).all() and (rec[:, 5] == 0).all()
        assert (rec[:, 3] > 0).all() and (rec[:, 4] == 0).all()
        assert (syn[:, 2] > 0).all() and (syn[:, 1] >= 30).all() and np.isfinite(syn[:, :4]).all()
        test, real = ev.mode_filelist("meta_step5")
        mels, f0 = ev.features(test + real)
        assert [len(m) for m in mels] == [30] * 4 + [26] * 4 and all(len(f) == len(m) for f, m in zip(f0, mels))
        assert np.array_equal(mcd.mcd_batch(mels[:4], mels[4:], f0[:4], f0[4:]), syn, equal_nan=True)
        ev.save_mcd()
        lines = open(cfg.path("txt", "mcd.txt")).read().splitlines()
        m, c, v = ev.summarize(syn)
        assert lines[0] == "recon:" and lines[1].startswith("MCD:0.0000\tF0_RMSE_cents:0.00\tVUV_percent:0.00") and lines[2] == "meta_step5:"
        assert lines[3] == f"MCD:{m:.4f}\tF0_RMSE_cents:{c:.2f}\tVUV_percent:{v:.2f}" and m == syn[:, 2].mean()
        assert os.path.exists(cfg.path("npy", "recon_mcd.npy")) and os.path.exists(cfg.path("npy", "meta_step5_mcd.npy"))
        again = E.ObjectiveEvaluation(cfg, mcd, stft, wav_loader=lambda p: pytest.fail("the saved tables are loaded, no file is read"))
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(again.get_mcd().values(), tables.values()))
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(again.load_mcd().values(), tables.values()))
        # without a pitch extractor: MCD only
        os.remove(cfg.path("npy", "recon_mcd.npy"))
        os.remove(cfg.path("npy", "meta_step5_mcd.npy"))
        plain = E.ObjectiveEvaluation(cfg, mcd, stft, wav_loader=lambda p: wavs[p]).get_mcd()
        assert np.array_equal(plain["meta_step5"][:, :3], syn[:, :3]) and np.isnan(plain["meta_step5"][:, 3:]).all()
        assert np.isnan(E.ObjectiveEvaluation.summarize(plain["recon"])[1:]).all()
    finally:
        mcd.close()
        pitch.close()
        stft.close()


def test_objective_evaluation_is_cut_into_calls(lib_path, tmp_path):
    """An evaluation set is more than one front-end call holds, so a mode is scored `pairs_per_call` pairs at a time and a block's files go
    to the front-end `frames_per_call` frames at a time.  The same tree with the default budgets (everything in one call per block), with
    60 frames per call and 3 pairs per block (two 26- or 30-frame files per call, a block boundary inside the mode), and with 10 frames
    per call (every file longer than the budget: each goes alone): more front-end calls, the same tables byte for byte.  Only the real
    files' features are kept.  A test sample without its directory or its wav is an error naming it, not a shorter table."""
    from meta_tts_amd.audio.pitch import PitchExtractor
    from meta_tts_amd.audio.stft import TacotronSTFT
    cfg, wavs = _result_tree(tmp_path)
    stft = TacotronSTFT(1024, HOP, 1024, 80, SR, 0.0, 8000.0, max_samples=SR, lib_path=lib_path)
    pitch = PitchExtractor(SR, HOP, lib_path=lib_path, max_samples=SR)
    mcd = E.MelCepstralDistortion(max_frames=64, lib_path=lib_path)
    load = lambda p: wavs[p]   # noqa: E731
    try:
        whole = E.ObjectiveEvaluation(cfg, mcd, stft, pitch=pitch, wav_loader=load)
        want = {m: whole.compute_mcd(m) for m in whole._modes()}
        assert whole.front_end_calls == 3                      # recon files, real files (once), synthesis files
        assert set(whole._real_features) == set(whole.real_filelist) and len(whole._real_features) == 4
        for kw, calls in ((dict(frames_per_call=60, pairs_per_call=3), 3 * (2 + 1)), (dict(frames_per_call=10), 12)):
            cut = E.ObjectiveEvaluation(cfg, mcd, stft, pitch=pitch, wav_loader=load, **kw)
            got = {m: cut.compute_mcd(m) for m in cut._modes()}
            assert cut.front_end_calls == calls, (kw, cut.front_end_calls)
            assert all(got[m].tobytes() == want[m].tobytes() and got[m].shape == (4, 6) for m in want), kw
            assert set(cut._real_features) == set(cut.real_filelist)
        for bad in (dict(frames_per_call=0), dict(frames_per_call=1 << 23), dict(pairs_per_call=0)):
            with pytest.raises(ValueError, match="frames_per_call|pairs_per_call"):
                E.ObjectiveEvaluation(cfg, mcd, stft, wav_loader=load, **bad)
        test, _ = whole.mode_filelist("meta_step5")
        os.remove(test[2])
        with pytest.raises(MttsError, match=r"mode meta_step5: test sample 2 has no \*FTstep_5.synth.wav in"):
            whole.compute_mcd("meta_step5")
        os.rmdir(os.path.dirname(test[2]))
        with pytest.raises(MttsError, match="mode meta_step5: test sample 2 has no directory"):
            whole.mode_filelist("meta_step5")
    finally:
        mcd.close()
        pitch.close()
        stft.close()
