"""Device pitch extraction (csrc/pitch.h through include/mtts.h: mtts_stft_load_pitch / mtts_stft_f0_batch; meta_tts_amd/audio/pitch.py
and `Preprocessor.f0_batch` / `build_from_path(f0_fn="device")`).  CPU tests run the device code through the SIMT emulator; the `-m gpu`
twins run it on the MI355X.

What is pinned to what:
  * PARITY with pyworld (DIO + StoneMask) is UNPINNED: pyworld is not available and is not restated.  Pinned instead: tests/f0_oracle.py,
    YIN as include/mtts.h states it, in float64 numpy — against the known frequency of synthetic glides and tones.
  * the oracle on the nine test signals (three seeds at (22050, 256), (16000, 200), (8000, 64)): p90 relative error on the glides'
    interior frames <= 2e-2 (measured 2.0e-3 .. 7.3e-3; the glide moves ~170 Hz/s, most of it is window bias), no frame whose span is
    all silence or all noise is voiced, at most 10 % of a signal's frames undecided (margin < 1e-3; measured: at most 2 of 76).
  * device vs oracle: same frame counts; the same voicing decision on every decided frame; on frames voiced on both sides
    max |f0_dev - f0_64| / f0_64 <= 4 E32 + 1e-7, where E32 is the same distance of the float32 numpy restatement (device summation
    order) on the same frames; aperiodicity alike in absolute terms.  Neither side of the bound is the device's own output.
  * bit identity (np.array_equal): an utterance alone, first, last, after an utterance whose length is no multiple of the hop.

Measured (printed by the tests; largest over the three seeds), the same figures from the emulator and from the MI355X:
  rate    E32 (f0)   device (f0)   E32 (ap)   device (ap)
  22050   1.79e-08   1.79e-08      5.31e-08   5.31e-08
  16000   5.56e-09   5.56e-09      5.05e-08   5.05e-08
   8000   9.21e-09   9.21e-09      5.87e-08   5.87e-08
(f0 is refined and divided in float64 on both sides, so E32 only carries the float32 rounding of three d' values; the device's chain
of FMAs and the float32 restatement round alike on these signals.)"""
import functools
import os

import numpy as np
import pytest

import __graft_entry__ as ge
import f0_oracle as O
from meta_tts_amd.audio import PitchExtractor
from meta_tts_amd.audio.pitch import _ptr, yin_window
from meta_tts_amd.engine import MttsError


def _emu():
    return ge.build_emulator()


@functools.lru_cache(maxsize=None)
def _case(sr, hop, seed):
    """(x, truth, segments, float64 result, float32 result) of one test signal: computed once, shared, never written to."""
    x, truth, segs = O.signal(sr, seed)
    res = O.yin(x, sr, hop), O.yin(x, sr, hop, dtype=np.float32)
    for a in (x, truth) + res[0] + res[1]:
        a.setflags(write=False)
    return x, truth, segs, res[0], res[1]


# ---- 1. the oracle against known signals -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,hop", O.CONFIGS)
def test_oracle_on_glides(sr, hop):
    for seed in O.SEEDS:
        x, truth, segs, (f64, _, margin), _ = _case(sr, hop, seed)
        n, T = len(x), len(f64)
        assert T == n // hop + 1
        tr = truth[np.minimum(np.arange(T) * hop, n - 1)]
        interior = O.frames_inside(n, sr, hop, segs, ("tone",))
        quiet = O.frames_inside(n, sr, hop, segs, ("silence", "noise"))
        assert interior.sum() >= 20 and quiet.sum() >= 10
        assert (f64[interior] > 0).all()
        err = np.abs(f64[interior] - tr[interior]) / tr[interior]
        undecided = int((margin < O.UNDECIDED).sum())
        print(f"{sr} seed {seed}: {T} frames, interior error median {np.median(err):.2e} p90 {np.percentile(err, 90):.2e} max {err.max():.2e}; "
              f"{int((f64[quiet] > 0).sum())} of {int(quiet.sum())} silence / noise frames voiced; {undecided} undecided")
        assert np.percentile(err, 90) <= 2e-2
        assert not (f64[quiet] > 0).any()
        assert undecided <= 0.1 * T


def test_oracle_constant_tones():
    """Pure tones of 0.3 s; the oracle's largest relative error over the frames whose span lies inside the signal:
              80 Hz     110 Hz    220 Hz    440 Hz    700 Hz
      22050   5.2e-06   5.4e-06   4.8e-05   2.1e-04   1.4e-04
      16000   1.0e-05   1.2e-05   8.0e-05   2.4e-04   8.5e-04
       8000   6.3e-05   9.2e-05   2.9e-04   1.5e-03   2.3e-03
    (the parabola through d' is a poorer fit the fewer samples a period has).  Asserted: below one semitone, so an octave error fails."""
    for sr, hop in O.CONFIGS:
        for hz in (80, 110, 220, 440, 700):
            x = O.tone(sr, hz)
            f0 = O.yin(x, sr, hop)[0]
            sp = O.spans(len(x), sr, hop)
            inside = (sp[:, 0] >= 0) & (sp[:, 1] <= len(x))
            assert inside.sum() >= 10 and (f0[inside] > 0).all()
            err = float((np.abs(f0[inside] - hz) / hz).max())
            print(f"{sr} Hz, tone {hz} Hz: max relative error {err:.2e}")
            assert err < 5.9e-2


def test_window_sizes():
    assert yin_window(22050) == O.window(22050) == (27, 311, 512, 823)
    assert yin_window(16000) == O.window(16000) == (20, 226, 384, 610)
    assert yin_window(8000) == O.window(8000) == (10, 113, 192, 305)


# ---- 2. device against the oracle ----------------------------------------------------------------------------------------------------------
def _compare(x, sr, hop, f_dev, a_dev, ref=None):
    """The rule of section 2 for one utterance; returns (E32 f0, device f0, E32 ap, device ap) as measured."""
    (f64, a64, margin), (f32, a32, _) = ref if ref is not None else (O.yin(x, sr, hop), O.yin(x, sr, hop, dtype=np.float32))
    assert f_dev.dtype == np.float64 and a_dev.dtype == np.float32 and f_dev.shape == a_dev.shape == f64.shape == (len(x) // hop + 1,)
    assert np.isfinite(f_dev).all() and np.isfinite(a_dev).all()
    decided = margin >= O.UNDECIDED
    assert np.array_equal((f_dev > 0)[decided], (f64 > 0)[decided])
    assert np.all(a_dev[f_dev == 0] == 1)                                             # unvoiced frames carry 1
    both = (f_dev > 0) & (f64 > 0) & (f32 > 0)
    if not both.any():
        return 0.0, 0.0, 0.0, 0.0
    e32 = float((np.abs(f32 - f64)[both] / f64[both]).max())
    dev = float((np.abs(f_dev - f64)[both] / f64[both]).max())
    e32a = float(np.abs(a32.astype(np.float64) - a64)[both].max())
    deva = float(np.abs(a_dev.astype(np.float64) - a64)[both].max())
    assert dev <= 4 * e32 + 1e-7, (dev, e32)
    assert deva <= 4 * e32a + 1e-7, (deva, e32a)
    return e32, dev, e32a, deva


def _check_device_vs_oracle(lib_path, sr, hop):
    pe = PitchExtractor(sr, hop, lib_path=lib_path)
    cases = [_case(sr, hop, seed) for seed in O.SEEDS]
    f0, ap = pe.f0_batch([c[0] for c in cases])
    worst = np.zeros(4)
    for c, f, a in zip(cases, f0, ap):
        worst = np.maximum(worst, _compare(c[0], sr, hop, f, a, ref=(c[3], c[4])))
        assert (f > 0).sum() >= len(f) // 3
    print("%d Hz: f0 relative distance to float64: float32 numpy %.3g, device %.3g; aperiodicity absolute: float32 numpy %.3g, device %.3g" % ((sr,) + tuple(worst)))
    pe.close()


@pytest.mark.parametrize("sr,hop", O.CONFIGS)
def test_device_vs_oracle_emulator(sr, hop):
    _check_device_vs_oracle(_emu(), sr, hop)


@pytest.mark.gpu
@pytest.mark.parametrize("sr,hop", O.CONFIGS)
def test_device_vs_oracle_gpu(sr, hop):
    _check_device_vs_oracle(None, sr, hop)


# ---- 3. bit identity ---------------------------------------------------------------------------------------------------------------------------
def _check_bit_identity(lib_path):
    sr, hop = 22050, 256
    tmin, tmax, W, L = O.window(sr)
    pe = PitchExtractor(sr, hop, lib_path=lib_path)
    a = _case(sr, hop, 0)[0]
    ragged = _case(sr, hop, 1)[0][:9001]                     # 9001 = 35 * 256 + 41
    even = _case(sr, hop, 2)[0][: 20 * hop]
    assert len(ragged) % hop and len(a) % hop
    alone_f, alone_a = pe.f0_batch([a])
    for batch, pos in (([a, ragged], 0), ([ragged, a], 1), ([even, a], 1), ([ragged, even, a, ragged], 2)):
        f, ap = pe.f0_batch(batch)
        assert np.array_equal(f[pos], alone_f[0]) and np.array_equal(ap[pos], alone_a[0]), (len(batch), pos)
    assert np.array_equal(pe.f0(a), alone_f[0])              # a second call
    # a loud tone up to the last sample of the first utterance, silence at the start of the second: no read across the boundary
    loud = (0.9 * np.sin(2 * np.pi * 200 * np.arange(5000) / sr)).astype(np.float32)
    second = np.concatenate([np.zeros(3 * hop + L, np.float32), O.tone(sr, 220, 0.2)])
    f, ap = pe.f0_batch([loud, second])
    quiet = np.arange(len(second) // hop + 1) * hop - L // 2 + L <= 3 * hop + L      # spans inside the leading zeros (and before sample 0)
    assert quiet.sum() >= 4 and np.abs(loud[-200:]).max() > 0.8
    assert np.all(f[1][quiet] == 0) and np.all(ap[1][quiet] == 1)
    fs, aps = pe.f0_batch([second])
    assert np.array_equal(f[1], fs[0]) and np.array_equal(ap[1], aps[0]) and (fs[0] > 0).sum() >= 5
    pe.close()


def test_bit_identity_emulator():
    _check_bit_identity(_emu())


@pytest.mark.gpu
def test_bit_identity_gpu():
    _check_bit_identity(None)


# ---- 4. edges ------------------------------------------------------------------------------------------------------------------------------------
def _check_edges(lib_path):
    sr, hop = 22050, 256
    tmin, tmax, W, L = O.window(sr)
    pe = PitchExtractor(sr, hop, lib_path=lib_path)
    long = _case(sr, hop, 2)[0]                                # 52 frames: four workgroup runs of 16 frames, the last one partial
    wavs = [O.tone(sr, 220, n=100),                            # n < hop: one frame
            O.tone(sr, 220, n=600),                            # n < L: every span padded
            O.tone(sr, 150, n=20 * hop),                       # n an exact multiple of hop
            np.zeros(3000, np.float32),                        # all zero
            long]
    assert [len(w) for w in wavs[:4]] == [100, 600, 20 * hop, 3000] and len(wavs[1]) < L and len(long) // hop + 1 > 48
    f0, ap = pe.f0_batch(wavs)
    assert [len(f) for f in f0] == [1, 3, 21, 12, len(long) // hop + 1]
    for k, (w, f, a) in enumerate(zip(wavs, f0, ap)):
        _compare(w, sr, hop, f, a, ref=(_case(sr, hop, 2)[3], _case(sr, hop, 2)[4]) if k == 4 else None)
    assert not f0[3].any() and np.all(ap[3] == 1)
    assert (f0[2][3:-3] > 0).all() and np.abs(f0[2][3:-3] / 150 - 1).max() < 5.9e-2
    one = pe.f0_batch([wavs[0]])                               # the short ones alone: the same bytes
    assert np.array_equal(one[0][0], f0[0]) and np.array_equal(pe.f0(wavs[1]), f0[1])
    pe.close()
    # 8 kHz, hop 64: 76 frames = five runs; a single sample
    pe = PitchExtractor(8000, 64, lib_path=lib_path)
    x = _case(8000, 64, 0)[0]
    f0, ap = pe.f0_batch([np.full(1, 0.5, np.float32), x])
    assert len(f0[0]) == 1 and f0[0][0] == 0
    _compare(x, 8000, 64, f0[1], ap[1], ref=(_case(8000, 64, 0)[3], _case(8000, 64, 0)[4]))
    pe.close()


def test_edges_emulator():
    _check_edges(_emu())


@pytest.mark.gpu
def test_edges_gpu():
    _check_edges(None)


# ---- 5. through the preprocessor ---------------------------------------------------------------------------------------------------------------
def _check_preprocessor(lib_path, tmp_path):
    import test_preprocess as TP
    trees = {}
    for kind in ("device", "callable"):
        c = TP._Corpus("small", str(tmp_path / kind), lib_path)
        c.write_raw()
        if kind == "device":
            out = c.pp.build_from_path(f0_fn="device", batch_utterances=3)
        else:
            pe = PitchExtractor(c.pp.sampling_rate, c.pp.hop_length, lib_path=lib_path)
            out = c.pp.build_from_path(f0_fn=lambda w, sr, hop: pe.f0(w), batch_utterances=3)
            pe.close()
            with pytest.raises(MttsError, match="nonsense"):
                c.pp.build_from_path(f0_fn="nonsense")
            try:
                import pyworld  # noqa: F401
            except ImportError:
                with pytest.raises(MttsError, match="pitch extraction needs pyworld"):
                    c.pp.build_from_path(batch_utterances=3)
        trees[kind] = (c.pp.out_dir, out)
        one = c.item(*c.utts[0])[2]
        f, a = c.pp.f0_batch([one])
        assert f[0].dtype == np.float64 and a[0].dtype == np.float32 and len(f[0]) == len(one) // c.pp.hop_length + 1
        c.pp.close()
    (da, oa), (db, ob) = trees["device"], trees["callable"]
    assert oa == ob and len(oa["train"]) >= 3
    n_files = 0
    for sub in ("mel", "pitch", "energy", "duration", "."):
        names = sorted(nm for nm in os.listdir(os.path.join(da, sub)) if os.path.isfile(os.path.join(da, sub, nm)))
        assert names == sorted(nm for nm in os.listdir(os.path.join(db, sub)) if os.path.isfile(os.path.join(db, sub, nm))) and names
        for nm in names:
            assert open(os.path.join(da, sub, nm), "rb").read() == open(os.path.join(db, sub, nm), "rb").read(), (sub, nm)
            n_files += 1
    assert {"stats.json", "speakers.json", "train.txt"} <= set(os.listdir(da)) and n_files >= 4 * len(oa["train"]) + 3


def test_through_preprocessor_emulator(tmp_path):
    _check_preprocessor(_emu(), tmp_path)


@pytest.mark.gpu
def test_through_preprocessor_gpu(tmp_path):
    _check_preprocessor(None, tmp_path)


# ---- 6. errors -------------------------------------------------------------------------------------------------------------------------------------
def _check_errors(lib_path):
    from meta_tts_amd.audio.stft import _Handle
    dev = _Handle(256, 256, 1, 4000, 0, lib_path)
    lib = dev.lib
    last = lambda: lib.mtts_stft_last_error(dev.h).decode()   # noqa: E731
    x, n = O.tone(22050, 220, n=1000), np.asarray([1000], np.int32)
    f0, ap = np.full(8, 7.0), np.full(8, 7.0, np.float32)
    assert lib.mtts_stft_f0_batch(dev.h, 1, _ptr(n), _ptr(x), _ptr(f0), _ptr(ap)) < 0 and "no pitch configuration loaded" in last()
    assert lib.mtts_stft_load_pitch(None, 22050, 71.0, 800.0, 0.15, 1e-4) != 0 and lib.mtts_stft_f0_batch(None, 1, _ptr(n), _ptr(x), _ptr(f0), _ptr(ap)) < 0
    assert lib.mtts_stft_load_pitch(dev.h, 22050, 71.0, 71.0, 0.15, 1e-4) != 0 and "f0_ceil <= f0_floor" in last()
    assert lib.mtts_stft_load_pitch(dev.h, 22050, 800.0, 71.0, 0.15, 1e-4) != 0 and "f0_ceil <= f0_floor" in last()
    assert lib.mtts_stft_load_pitch(dev.h, 1000, 71.0, 800.0, 0.15, 1e-4) != 0 and "tau_min" in last() and "< 2" in last()
    assert lib.mtts_stft_load_pitch(dev.h, 22050, 71.0, 800.0, 0.0, 1e-4) != 0 and "bad arguments" in last()
    assert lib.mtts_stft_load_pitch(dev.h, 192000, 20.0, 800.0, 0.15, 1e-4) != 0 and "exceeds what a workgroup stages" in last()
    assert lib.mtts_stft_f0_batch(dev.h, 1, _ptr(n), _ptr(x), _ptr(f0), _ptr(ap)) < 0 and np.all(f0 == 7.0)       # none of the refused loads left a configuration
    pe = PitchExtractor(22050, 256, _handle=dev)
    good = pe.f0(x)
    assert len(good) == 4 and (good > 0).any()
    assert lib.mtts_stft_load_pitch(dev.h, 22050, 71.0, 71.0, 0.15, 1e-4) != 0 and np.array_equal(pe.f0(x), good)  # a refused load keeps the one before
    for bad_n in (0, -1):
        assert lib.mtts_stft_f0_batch(dev.h, bad_n, _ptr(n), _ptr(x), _ptr(f0), _ptr(ap)) < 0 and "n_utts < 1" in last()
    assert lib.mtts_stft_f0_batch(dev.h, 2, _ptr(np.asarray([1000, 0], np.int32)), _ptr(x), _ptr(f0), _ptr(ap)) < 0 and "utterance 1: n_samples < 1" in last()
    assert lib.mtts_stft_f0_batch(dev.h, 1, _ptr(n), None, _ptr(f0), _ptr(ap)) < 0 and lib.mtts_stft_f0_batch(dev.h, 1, _ptr(n), _ptr(x), None, _ptr(ap)) < 0
    assert np.all(f0 == 7.0) and np.all(ap == 7.0)
    assert lib.mtts_stft_f0_batch(dev.h, 1, _ptr(n), _ptr(x), _ptr(f0), None) == 4 and np.array_equal(f0[:4], good)   # aperiodicity is optional
    with pytest.raises(MttsError, match="no waveforms"):
        pe.f0_batch([])
    with pytest.raises(MttsError, match="utterance 1: n_samples < 1"):
        pe.f0_batch([x, np.zeros(0, np.float32)])
    with pytest.raises(MttsError, match="utterance 0: 4500 samples exceed max_samples = 4000"):
        pe.f0_batch([np.zeros(4500, np.float32)])
    with pytest.raises(MttsError, match="hop length is 256, asked for 200"):
        PitchExtractor(16000, 200, _handle=dev)
    with pytest.raises(MttsError, match="tau_min"):
        PitchExtractor(1000, 256, _handle=dev)
    dev.close()


def test_errors_emulator():
    _check_errors(_emu())


@pytest.mark.gpu
def test_errors_gpu():
    _check_errors(None)
