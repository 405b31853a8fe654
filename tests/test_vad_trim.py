"""Device silence trimming (csrc/vad.h through include/mtts.h: mtts_stft_load_vad / mtts_stft_trim_batch,
mtts_dvector_embed_wavs_preprocessed; meta_tts_amd/audio/vad.py and the opt-in wiring in evaluation.py / preprocessor.py / resample.py).
CPU tests run the device code through the SIMT emulator; the `-m gpu` twins run it on the MI355X.

What is pinned to what:
  * PARITY with webrtcvad is UNPINNED (it is not available and not restated); no test rests on the detector's three constants being
    "right".  Pinned instead: the definition of include/mtts.h as tests/vad_oracle.py writes it in float64 numpy.
  * injected flags: the resemblyzer post-processing on the device equals the host `trim_long_silences` and the oracle bit for bit
    (np.array_equal on masks, lengths and samples), and scipy.ndimage.binary_dilation where scipy imports.
  * energy detector: every test input keeps each e[w] at least a relative 1e-9 away from its threshold (asserted on the oracle before
    comparing; no window is left out).  The device's fixed-order float64 sum of W = 480 exact products and numpy's pairwise sum each
    differ from the exact sum by at most about W 2^-53 relative, so the two differ by at most 2 W 2^-53 = 1.1e-13 — far inside 1e-9, so
    masks, lengths and samples are compared with np.array_equal — and that same 2 W 2^-53 gates `energy_out`.
  * bit identity: an utterance's output, mask and energies alone, in a batch, at any position, across two calls; the chained entry
    against embed_utterances(trim_batch(resample_batch(...))) and under another max_partials chunking."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
import vad_oracle as O
from meta_tts_amd import _lib
from meta_tts_amd import evaluation as E
from meta_tts_amd.audio import resample as A
from meta_tts_amd.audio import vad as V
from meta_tts_amd.audio.stft import _Handle
from meta_tts_amd.engine import MttsError
from meta_tts_amd.speaker_encoder import synthetic_state_dict

TINY = dict(hidden=64, emb=32, layers=2)
FULL = dict(hidden=256, emb=256, layers=3)
W = O.W
E_GATE = 2 * W * 2.0 ** -53


def _emu():
    return ge.build_emulator()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _windows(levels, seed, tail=0):
    """One window per entry of `levels`: 1 = a loud tone (0.3), 0 = faint noise (1e-4), a float = noise at that standard deviation."""
    g = np.random.RandomState(seed)
    out = []
    for lv in list(levels) + [0] * (1 if tail else 0):
        if lv == 1:
            out.append(0.3 * np.sin(2 * np.pi * 200 * np.arange(W) / O.SR + g.rand()))
        else:
            out.append((1e-4 if lv == 0 else lv) * g.standard_normal(W))
    x = np.concatenate(out).astype(np.float32)
    return x[: len(levels) * W + tail]


def _pattern(n_w, seed):
    """Voiced stretches of 6 .. 40 windows between pauses of 1 .. 30."""
    g = np.random.RandomState(seed)
    lv = []
    while len(lv) < n_w:
        lv += [0] * g.randint(1, 31) + [1] * g.randint(6, 41)
    return lv[:n_w]


# ---- 1. the host post-processing ---------------------------------------------------------------------------------------------------------
def test_host_post_processing_equals_oracle():
    g = np.random.RandomState(0)
    for ma in (1, 2, 3, 8, 64):
        for ms in (1, 2, 5, 6, 64):
            for _ in range(10):
                f = g.rand(g.randint(1, 90)) < 0.45
                assert np.array_equal(V.smooth_and_dilate(f, ma, ms), O.post(f, ma, ms)), (ma, ms)
    assert np.array_equal(V.moving_average([1, 1, 0, 1], 8), O.moving_average(np.asarray([1.0, 1, 0, 1]), 8))
    # 4 of 8 is 0.5 and rounds to even: 0; 5 of 8 rounds to 1
    assert not V.smooth_and_dilate([0] * 10 + [1] * 4 + [0] * 10).any() and V.smooth_and_dilate([0] * 10 + [1] * 5 + [0] * 10).any()
    x = np.arange(5 * W + 7, dtype=np.float32)
    assert V.trim_long_silences(x, [0] * 5) is not None and np.array_equal(V.trim_long_silences(x, [0] * 5), x)      # nothing kept: as it is
    assert np.array_equal(V.trim_long_silences(x, [1] * 5), x[: 5 * W])
    with pytest.raises(ValueError, match="4 flags for 5 windows"):
        V.trim_long_silences(x, [1] * 4)


def test_oracle_dilation_equals_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    g = np.random.RandomState(1)
    for length in range(1, 12):
        for _ in range(20):
            f = g.rand(g.randint(1, 40)) < 0.2
            assert np.array_equal(O.dilate(f, length), ndimage.binary_dilation(f, np.ones(length))), length


# ---- 2. injected flags: the post-processing on the device ------------------------------------------------------------------------------------
def _flag_cases():
    n_w = 40
    cases = {}
    for run in (4, 5, 8):
        f = np.zeros(n_w, bool)
        f[16:16 + run] = True
        cases[f"run{run}"] = f
    for name, sl in (("first", slice(0, 5)), ("last", slice(n_w - 5, n_w)), ("first4", slice(0, 4)), ("last4", slice(n_w - 4, n_w))):
        f = np.zeros(n_w, bool)
        f[sl] = True
        cases[name] = f
    for gap in range(1, 17):
        f = np.zeros(n_w, bool)
        f[8:14] = True
        f[14 + gap:20 + gap] = True
        cases[f"gap{gap}"] = f
    cases["all"] = np.ones(n_w, bool)
    cases["none"] = np.zeros(n_w, bool)
    cases["one_window"] = np.ones(1, bool)
    cases["seven"] = np.ones(7, bool)
    return cases


def _check_flags(lib_path):
    cases = _flag_cases()
    names = sorted(cases)
    g = np.random.RandomState(2)
    wavs = [g.standard_normal(len(cases[k]) * W + (i * 37) % W).astype(np.float32) for i, k in enumerate(names)]
    t = V.SilenceTrimmer(lib_path=lib_path)
    out, (masks, n_voiced, energies) = t.trim_batch(wavs, flags=[cases[k] for k in names], return_masks=True)
    assert energies is None
    got = {}
    for k, w, o, m, v in zip(names, wavs, out, masks, n_voiced):
        want, want_mask, want_v, _ = O.trim(w, flags=cases[k])
        assert np.array_equal(m, want_mask) and v == want_v == int(m.sum()), k
        assert o.dtype == np.float32 and np.array_equal(o, want) and np.array_equal(o, V.trim_long_silences(w, cases[k])), k
        assert len(o) == (v * W if v else len(w)), k
        got[k] = m
    assert not got["run4"].any() and not got["first4"].any() and not got["none"].any()              # 4 of 8 rounds to 0: the run vanishes
    assert got["run5"].any() and got["run8"].any() and got["all"].all()
    # smooth[w] needs 5 of raw[w - 3 .. w + 4]: the run 16 .. 20 smooths to 16 .. 19, the run 16 .. 23 to 16 .. 22; dilated by 3 each way
    assert np.flatnonzero(got["run5"]).tolist() == list(range(13, 23)) and np.flatnonzero(got["run8"]).tolist() == list(range(13, 26))
    assert np.flatnonzero(got["first"]).tolist() == list(range(0, 7))                                # 0 .. 4 smooths to 0 .. 3: window 0 sees raw[0 .. 4] behind 3 zeros
    assert np.flatnonzero(got["last"]).tolist() == list(range(32, 40))                               # 35 .. 39 smooths to 35 .. 38: window 38 sees raw[35 .. 39] and 3 zeros
    assert not got["one_window"].any() and got["seven"].any()                                        # 1 of 8; 5 .. 7 of 8
    bridged = [gap for gap in range(1, 17) if got[f"gap{gap}"][8:20 + gap].all()]
    print("gaps bridged between two runs of 6:", bridged)
    assert bridged == [gap for gap in range(1, 17) if O.post(cases[f"gap{gap}"])[8:20 + gap].all()] and 1 in bridged and 16 not in bridged
    # another width: even structure, odd average
    t2 = V.SilenceTrimmer(ma_width=3, max_silence=1, _handle=t._dev)
    f = g.rand(57) < 0.4
    w = g.standard_normal(57 * W + 5).astype(np.float32)
    o2, (m2, v2, _) = t2.trim_batch([w], flags=[f], return_masks=True)
    assert np.array_equal(m2[0], O.post(f, 3, 1)) and np.array_equal(o2[0], O.trim(w, flags=f, ma_width=3, max_silence=1)[0])
    assert np.array_equal(t.trim_batch([wavs[0]], flags=[cases[names[0]]])[0], out[0])               # the first configuration is loaded again
    t.close()
    return got, cases


def test_injected_flags_emulator():
    _check_flags(_emu())


def test_injected_flags_match_scipy_emulator():
    ndimage = pytest.importorskip("scipy.ndimage")
    got, cases = _check_flags(_emu())
    for k, m in got.items():
        smooth = np.round(O.moving_average(cases[k].astype(np.float64), 8)).astype(bool)
        assert np.array_equal(m, ndimage.binary_dilation(smooth, np.ones(7))), k


@pytest.mark.gpu
def test_injected_flags_gpu():
    _check_flags(None)


# ---- 3. the energy detector against the oracle -----------------------------------------------------------------------------------------------
def _energy_inputs():
    g = np.random.RandomState(3)
    lv30 = [0] * 5 + [1] * 10 + [0] * 9 + [1] * 6            # (the 10 % quantile must fall on a pause: 3 quiet windows at least)
    return {
        "shorter_than_a_window": _windows([], 5, tail=W - 1),
        "one_window": _windows([1], 6),                                       # n_w = 1: k = 0, the window is its own noise estimate
        "one_window_and_a_sample": _windows([1], 7, tail=1),
        "below_ma_width": _windows([0, 1, 1, 1, 1, 1, 1], 8, tail=W - 1),      # 8 W - 1 samples: 7 windows
        "at_ma_width": _windows([0, 1, 1, 1, 1, 1, 1, 0], 9),                 # 8 W
        "speech": _windows(lv30, 10, tail=100),
        "zeros": np.zeros(10 * W + 3, np.float32),
        "noise_only": _windows([0.01] * 40, 11, tail=17),                     # constant level: nothing is `margin_db` above the 10 % quantile
        "w255": _windows(_pattern(255, 12), 12, tail=3),
        "w256": _windows(_pattern(256, 13), 13),
        "w257": _windows(_pattern(257, 14), 14, tail=W - 1),
        "w4096": _windows(_pattern(4096, 15), 15),
        "loud_tail": _windows([0] * 20 + [1] * 9, 16),
    }, g


def _compare(name, w, o, m, v, e, **cfg):
    want, want_mask, want_v, want_e = O.trim(w, **cfg)
    kw = {k: cfg[k] for k in ("floor_db", "noise_quantile", "margin_db") if k in cfg}
    assert O.margin(want_e, **kw) >= 1e-9, (name, O.margin(want_e, **kw))            # the condition under which the masks must agree
    assert e.shape == want_e.shape and m.shape == want_mask.shape == (len(w) // W,)
    rel = float(np.max(np.abs(e - want_e) / want_e)) if len(e) and want_e.min() > 0 else float(np.max(np.abs(e - want_e))) if len(e) else 0.0
    assert np.all(np.abs(e - want_e) <= E_GATE * want_e), (name, rel)
    assert np.array_equal(m, want_mask) and v == want_v, name
    assert np.array_equal(o, want), name
    return rel


def _check_energy(lib_path):
    inputs, g = _energy_inputs()
    names = sorted(inputs)
    t = V.SilenceTrimmer(lib_path=lib_path, max_samples=4097 * W)
    out, (masks, n_voiced, energies) = t.trim_batch([inputs[k] for k in names], return_masks=True)
    worst = 0.0
    res = {}
    for k, o, m, v, e in zip(names, out, masks, n_voiced, energies):
        worst = max(worst, _compare(k, inputs[k], o, m, v, e))
        res[k] = (o, m, int(v))
    print("max relative difference of the window energies from numpy's: %.3g (gate %.3g)" % (worst, E_GATE))
    for k in ("shorter_than_a_window", "zeros", "noise_only", "one_window", "one_window_and_a_sample"):   # pass-through, tail included
        assert res[k][2] == 0 and not res[k][1].any() and np.array_equal(res[k][0], inputs[k]), k
    for k in ("below_ma_width", "at_ma_width", "speech", "w255", "w256", "w257", "w4096", "loud_tail"):
        assert 0 < res[k][2] and len(res[k][0]) == res[k][2] * W, k
    assert res["speech"][2] < 30 and res["w4096"][2] < 4096                                          # something was trimmed
    # all voiced: a margin below 0 dB puts every window of a constant-level signal above the noise estimate
    loud = _windows([1] * 12, 17, tail=55)
    t2 = V.SilenceTrimmer(margin_db=-3.0, noise_quantile=0.5, floor_db=-60.0, _handle=t._dev)
    o2, (m2, v2, e2) = t2.trim_batch([loud], return_masks=True)
    _compare("all_voiced", loud, o2[0], m2[0], v2[0], e2[0], margin_db=-3.0, noise_quantile=0.5, floor_db=-60.0)
    assert m2[0].all() and np.array_equal(o2[0], loud[: 12 * W])
    # the floor: a quiet signal with structure stays below 10^(floor_db / 10)
    quiet = (_windows(_pattern(30, 18), 18) * np.float32(0.005)).astype(np.float32)
    o3, (m3, v3, e3) = t.trim_batch([quiet], return_masks=True)
    _compare("under_the_floor", quiet, o3[0], m3[0], v3[0], e3[0])
    assert v3[0] == 0 and float(e3[0].max()) < 10 ** -5
    t.close()


def test_energy_detector_emulator():
    _check_energy(_emu())


@pytest.mark.gpu
def test_energy_detector_gpu():
    _check_energy(None)


# ---- 4. bit identity ---------------------------------------------------------------------------------------------------------------------------
def _check_bit_identity(lib_path):
    g = np.random.RandomState(20)
    secs = [0.05, 3.0] + list(g.uniform(0.05, 3.0, 6))
    wavs = [O.speechlike(int(s * O.SR), 30 + i) for i, s in enumerate(secs)] + [_windows(_pattern(n, n), n, tail=n % 7) for n in (255, 256, 257)]
    t = V.SilenceTrimmer(lib_path=lib_path)
    alone = [t.trim_batch([w], return_masks=True) for w in wavs[:3] + wavs[-3:]]                     # small calls first: the workspace grows below
    batch = t.trim_batch(wavs, return_masks=True)
    rev = t.trim_batch(wavs[::-1], return_masks=True)
    again = t.trim_batch(wavs, return_masks=True)

    def item(r, i):
        return r[0][i], r[1][0][i], int(r[1][1][i]), r[1][2][i]

    def same(a, b):
        return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and np.array_equal(a[3], b[3])

    n = len(wavs)
    for i in range(n):
        assert same(item(batch, i), item(rev, n - 1 - i)) and same(item(batch, i), item(again, i)), i
    for j, i in enumerate([0, 1, 2, n - 3, n - 2, n - 1]):
        assert same(item(batch, i), item(alone[j], 0)), i
    assert any(0 < item(batch, i)[2] < len(wavs[i]) // W for i in range(n))                          # not all trivially kept or passed
    t.close()


def test_bit_identity_emulator():
    _check_bit_identity(_emu())


@pytest.mark.gpu
def test_bit_identity_gpu():
    _check_bit_identity(None)


# ---- 5. the chained entry ------------------------------------------------------------------------------------------------------------------------
def _chain_wavs():
    """22 050 Hz: speech-like utterances with pauses, a quiet one (turned up to -30 dBFS), and one of faint noise only (passed through)."""
    lengths = [71000, 22050, 45632, 28000, 56001]
    wavs = [O.speechlike(n, 50 + i, sr=22050) * np.float32(0.02 if i == 2 else 1.0) for i, n in enumerate(lengths)]
    wavs[3] = (1e-4 * np.random.RandomState(9).standard_normal(lengths[3])).astype(np.float32)
    return wavs


def _check_chain(lib_path, dims):
    wavs = _chain_wavs()
    emb = E.SpeakerEmbedder(synthetic_state_dict(3, **dims), lib_path=lib_path, max_partials=6, **dims)
    pre = emb.resampler(22050).resample_batch(wavs, normalize_dbfs=-30)
    trimmed, (masks, n_voiced, energies) = emb.trimmer().trim_batch(pre, return_masks=True)
    for p, t, m, v, e in zip(pre, trimmed, masks, n_voiced, energies):                               # the device trim of the device-resampled signal = the oracle's
        _compare("chain", p, t, m, v, e)
    assert n_voiced[3] == 0 and len(trimmed[3]) == len(pre[3]) and all(0 < v < len(p) // W for i, (v, p) in enumerate(zip(n_voiced, pre)) if i != 3)
    assert sum(len(E.compute_partial_slices(len(p))[1]) for p in trimmed) > 6                        # at least two chunks
    want_vec, want_sl = emb.embed_utterances(trimmed, return_slices=True)
    got_vec, got_sl = emb.embed_utterances(wavs, return_slices=True, source_rate=22050, normalize_dbfs=-30, trim=True)
    assert np.array_equal(emb.last_trimmed_lengths, [len(t) for t in trimmed])
    assert np.array_equal(got_vec, want_vec) and len(got_sl) == len(want_sl)
    for a, b in zip(got_sl, want_sl):
        assert np.array_equal(a, b)
    # 16 kHz input: the identity bank, with and without source_rate; no normalisation
    plain = emb.embed_utterances(emb.trimmer().trim_batch(pre[:2]))
    assert np.array_equal(emb.embed_utterances(pre[:2], trim=True), plain) and np.array_equal(emb.embed_utterances(pre[:2], source_rate=16000, trim=True), plain)
    assert np.array_equal(emb.reference_mel_slices(wavs[0], source_rate=22050, normalize_dbfs=-30, trim=True), want_sl[0])
    assert np.array_equal(emb.embed_utterances(wavs, source_rate=22050, normalize_dbfs=-30), emb.embed_utterances(pre))   # trim off: as before
    # another chunking: one chunk, and one utterance per chunk
    for mp, mu in ((64, 256), (64, 1)):
        other = E.SpeakerEmbedder(synthetic_state_dict(3, **dims), lib_path=lib_path, max_partials=mp, max_utts=mu, **dims)
        assert np.array_equal(other.embed_utterances(wavs, source_rate=22050, normalize_dbfs=-30, trim=True), want_vec), (mp, mu)
        other.close()
    # preprocess_wav(trim="device") is the same three steps, host to host
    dev = A.preprocess_wav(wavs, 22050, trim="device", resampler=emb.resampler(22050))
    assert len(dev) == len(trimmed) and all(np.array_equal(a, b) for a, b in zip(dev, trimmed))
    with pytest.raises(ValueError, match="exclude each other"):
        A.preprocess_wav(wavs, 22050, trim_fn=lambda w: w, trim="device", resampler=emb.resampler(22050))
    emb.close()


def _check_chain_without_resampler(lib_path):
    """The C entry on a handle that holds a VAD configuration and NO resampler: the waveforms are uploaded at the front-end's rate
    straight into the trimmer's staging buffer (the Python layer always loads a bank, so this goes through ctypes)."""
    emb = E.SpeakerEmbedder(synthetic_state_dict(3, **TINY), lib_path=lib_path, max_partials=4, **TINY)
    wavs = [O.speechlike(n, 70 + i) for i, n in enumerate([52000, 16000, 33333])] + [(1e-3 * np.random.RandomState(8).standard_normal(20000)).astype(np.float32)]
    trimmed, (masks, n_voiced, energies) = emb.trimmer().trim_batch(wavs, return_masks=True)
    for w, t, m, v, e in zip(wavs, trimmed, masks, n_voiced, energies):
        _compare("no_resampler", w, t, m, v, e)
    assert n_voiced[3] == 0 and any(0 < v < len(w) // W for v, w in zip(n_voiced, wavs))
    want_vec, want_sl = emb.embed_utterances(trimmed, return_slices=True)
    assert not emb._resamplers and getattr(emb._dev, "_resampler_key", None) is None                 # nothing above loaded a bank
    n = np.asarray([len(w) for w in wavs], np.int32)
    packed = np.ascontiguousarray(np.concatenate(wavs))
    vec, cnt, ntr = np.empty((len(wavs), TINY["emb"]), np.float32), np.empty(len(wavs), np.int32), np.empty(len(wavs), np.int32)
    bound = sum(len(E.compute_partial_slices(len(w))[1]) for w in wavs)
    sl = np.empty((bound, 160, 40), np.float32)
    rc = emb.lib.mtts_dvector_embed_wavs_preprocessed(emb.encoder.h, emb._dev.h, len(wavs), _ptr(n), _ptr(packed), 160, emb.frame_step, 0.75, float("nan"), 0,
                                                      _ptr(vec), _ptr(cnt), _ptr(sl), _ptr(ntr))
    assert rc == 0, emb.lib.mtts_stft_last_error(emb._dev.h).decode()
    assert np.array_equal(ntr, [len(t) for t in trimmed]) and np.array_equal(cnt, [len(s) for s in want_sl]) and cnt.sum() > 4   # two chunks at least
    assert np.array_equal(vec, want_vec) and np.array_equal(sl[: cnt.sum()], np.concatenate(want_sl))
    emb.close()


def test_chain_without_resampler_emulator():
    _check_chain_without_resampler(_emu())


@pytest.mark.gpu
def test_chain_without_resampler_gpu():
    _check_chain_without_resampler(None)


def test_chain_emulator():
    _check_chain(_emu(), TINY)


@pytest.mark.gpu
@pytest.mark.parametrize("dims", [TINY, FULL], ids=["tiny", "full"])
def test_chain_gpu(dims):
    _check_chain(None, dims)


def _chunk_wavs(sr):
    """Five utterances of 0.3 .. 1.2 s at `sr`, in 30 ms windows of tone (1) and faint noise (0), three of them with a ragged tail.  One
    partial each, so max_partials = 2 cuts them into the chunks (0, 1), (2, 3), (4), and the last chunk holds the most samples,
    sum-of-squares slots and VAD windows.  Utterance 2 opens with 12 silent windows, more than smoothing and dilation bridge; utterance
    0 is all tone (the noise quantile is the tone itself: nothing is kept and it passes through)."""
    w, g = sr * 30 // 1000, np.random.RandomState(77)
    out = []
    for levels, tail in (([1] * 10, 0), ([1] * 5 + [0] * 2 + [1] * 4, 7), ([0] * 12 + [1] * 10, 0), ([1] * 10, 123), ([1] * 9 + [0] * 14 + [1] * 16, 5)):
        x = [0.3 * np.sin(2 * np.pi * 200 * np.arange(w) / sr + g.rand()) if lv else 1e-4 * g.standard_normal(w) for lv in levels + [0]]
        out.append(np.concatenate(x).astype(np.float32)[: len(levels) * w + tail])
    n = [len(x) for x in out]
    assert 0.3 * sr <= min(n) and max(n) <= 1.2 * sr and n[4] > n[2] + n[3] > n[0] + n[1]
    return out


def _embed_entry(emb, which, wavs, dbfs):
    """One of the three C entries -> (d-vectors, slices, partial counts, trimmed lengths (-1 where the entry does not trim))."""
    n, packed = np.asarray([len(w) for w in wavs], np.int32), np.ascontiguousarray(np.concatenate(wavs))
    vec, cnt, ntr = np.empty((len(wavs), emb.emb), np.float32), np.full(len(wavs), -1, np.int32), np.full(len(wavs), -1, np.int32)
    sl = np.empty((sum(len(E.compute_partial_slices(len(w))[1]) for w in wavs), 160, 40), np.float32)      # (a bound: no entry lengthens a waveform)
    args = (emb.encoder.h, emb._dev.h, len(wavs), _ptr(n), _ptr(packed), 160, emb.frame_step, 0.75)
    outs = (_ptr(vec), _ptr(cnt), _ptr(sl))
    if which == "plain":
        rc = emb.lib.mtts_dvector_embed_wavs(*args, *outs)
    elif which == "resampled":
        rc = emb.lib.mtts_dvector_embed_wavs_resampled(*args, dbfs, 1, *outs)
    else:
        rc = emb.lib.mtts_dvector_embed_wavs_preprocessed(*args, dbfs, 1, *outs, _ptr(ntr))
    assert rc == 0, emb.lib.mtts_stft_last_error(emb._dev.h).decode()
    return vec, sl[: cnt.sum()].copy(), cnt, ntr


def _check_chunk_tables(lib_path, streams=None):
    """All three entries over three chunks whose largest comes last (every buffer is sized before the first launch, every chunk keeps
    host tables of its own): each utterance's d-vector, slices, partial count and trimmed length equal those of the same entry called
    with that utterance alone."""
    emb = E.SpeakerEmbedder(synthetic_state_dict(3, **TINY), lib_path=lib_path, max_partials=2, **TINY)
    if streams:
        emb.set_streams(*streams)
    emb.trimmer()

    def check(which, wavs, dbfs, rate_ratio):
        vec, sl, cnt, ntr = _embed_entry(emb, which, wavs, dbfs)
        assert np.all(cnt == 1), cnt                                                                 # hence the chunks (0, 1), (2, 3), (4)
        if which == "preprocessed":
            n16 = [-(-len(w) * rate_ratio[0] // rate_ratio[1]) for w in wavs]
            assert ntr[0] == n16[0] and 480 <= ntr[2] <= n16[2] - 6 * 480 and ntr[4] < n16[4], (ntr, n16)   # passed through; the leading silence cut
        for i, w in enumerate(wavs):
            v1, s1, c1, t1 = _embed_entry(emb, which, [w], dbfs)
            assert np.array_equal(v1[0], vec[i]) and np.array_equal(s1[0], sl[i]) and c1[0] == cnt[i] and t1[0] == ntr[i], (which, i)

    w16, w24, nan = _chunk_wavs(16000), _chunk_wavs(24000), float("nan")
    check("plain", w16, nan, (1, 1))
    check("preprocessed", w16, nan, (1, 1))                                                          # no resampler loaded: uploaded into the staging buffer
    assert getattr(emb._dev, "_resampler_key", None) is None
    emb.resampler(24000)
    check("resampled", w24, -30.0, (2, 3))
    check("preprocessed", w24, -30.0, (2, 3))                                                        # through the resampler
    if streams:
        emb.set_streams(0, 0)
    emb.close()


def test_chunk_tables_emulator():
    _check_chunk_tables(_emu())


@pytest.mark.gpu
@pytest.mark.parametrize("two_streams", [False, True], ids=["one_stream", "two_streams"])
def test_chunk_tables_gpu(two_streams):
    import torch
    s = (torch.cuda.Stream(), torch.cuda.Stream()) if two_streams else None
    _check_chunk_tables(None, (s[0].cuda_stream, s[1].cuda_stream) if s else None)


def _check_result_tree(lib_path, tmp_path):
    """WavsToDvector(resample=True, trim=True) over a Saver-shaped result tree at 22 050 Hz, and the preprocessing hook."""
    import json
    import os
    import random
    from scipy.io import wavfile
    from meta_tts_amd.preprocessor import Preprocessor, read_wav
    n_speaker, root, sq = 5, str(tmp_path), []
    raw = os.path.join(root, "raw")

    def write(path, seed):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        wavfile.write(path, 22050, (O.speechlike(18000 + 997 * (seed % 9), seed, sr=22050) * 20000).astype(np.int16))

    for s in range(n_speaker):
        for u in range(4):
            write(os.path.join(raw, f"{100 + s}", f"{100 + s}_{u:02d}.wav"), 10 * s + u)
        sq.append({"sup_id": [f"{100 + s}_03"], "qry_id": [f"{100 + s}_00"]})
    res = os.path.join(root, "result", "m1")
    for data_id, q in enumerate(sq):
        d = os.path.join(res, "audio", "Testing", f"test_{data_id:03d}")
        write(os.path.join(d, f"{q['qry_id'][0]}.recon.wav"), 500 + data_id)
        write(os.path.join(d, f"{q['qry_id'][0]}.step_100000-FTstep_5.synth.wav"), 600 + data_id)
    json.dump(sq, open(os.path.join(res, "test_SQids.json"), "w"))
    dirs = {"recon": res, "m1": res, "real": raw, "enrollment": raw}
    emb = E.SpeakerEmbedder(synthetic_state_dict(3, **TINY), lib_path=lib_path, max_partials=8, **TINY)
    real = [read_wav(os.path.join(raw, f"{100 + s}", f"{100 + s}_00.wav"))[0] for s in range(n_speaker)]
    pre = emb.resampler(22050).resample_batch(real, normalize_dbfs=-30)
    trimmed, (_, n_voiced, _) = emb.trimmer().trim_batch(pre, return_masks=True)
    assert any(0 < v < len(p) // W for v, p in zip(n_voiced, pre))                                   # trimming changes these files
    want = emb.embed_utterances(trimmed)
    walks = {}
    for trim in (False, True):
        cfg = E.EvalConfig("Tiny", dirs, n_speaker, 1, [("m1", [5])], work_dir=os.path.join(root, f"work{int(trim)}"))
        walks[trim] = E.WavsToDvector(cfg, emb, rng=random.Random(3), resample=True, trim=trim).dvector_list_dict["real"]
    assert np.array_equal(walks[True], want) and np.array_equal(walks[False], emb.embed_utterances(pre)) and not np.array_equal(walks[True], walks[False])
    # Preprocessor.speaker_reference_fn(trim=True): -30 dBFS and trimming on the device behind the injected resampler
    pp = Preprocessor.__new__(Preprocessor)
    pp.in_dir, pp.train_set, pp.val_set, pp.test_set = root, "raw", "raw", "raw"
    front = E.SpeakerEmbedder(lib_path=lib_path, encoder=False)
    rs = front.resampler(22050)
    got = pp.speaker_reference_fn(front, resample=rs, trim=True)("100", "100_00")
    plain = pp.speaker_reference_fn(front, resample=rs)("100", "100_00")
    y = rs.resample_batch([real[0]])[0]
    assert np.array_equal(plain, front.reference_mel_slices(y))                                      # the default: as before
    by_hand = front.trimmer().trim_batch(front.resampler(16000).resample_batch([y], normalize_dbfs=-30))[0]
    assert np.array_equal(front.last_trimmed_lengths, [len(by_hand)]) and len(by_hand) < len(y)
    assert np.array_equal(got, front.reference_mel_slices(by_hand)) and got.shape[0] <= plain.shape[0]
    front.close()
    emb.close()


def test_result_tree_and_reference_slices_emulator(tmp_path):
    pytest.importorskip("scipy.io")
    _check_result_tree(_emu(), tmp_path)


@pytest.mark.gpu
def test_result_tree_and_reference_slices_gpu(tmp_path):
    pytest.importorskip("scipy.io")
    _check_result_tree(None, tmp_path)


# ---- 6. refusals: before any launch, outputs untouched ---------------------------------------------------------------------------------------
def _check_errors(lib_path):
    dev = _Handle(16, 4, 1, 4097 * W, 0, lib_path)
    lib = dev.lib
    err = lambda: lib.mtts_stft_last_error(dev.h).decode()                                          # noqa: E731
    x, n = np.full(3 * W, 0.25, np.float32), np.asarray([3 * W], np.int32)
    out, n_out, nv = np.full(3 * W, 7.0, np.float32), np.full(1, -5, np.int32), np.full(1, -5, np.int32)
    mask, en = np.full(4, 9, np.uint8), np.full(4, 9.0)
    untouched = lambda: np.all(out == 7.0) and n_out[0] == -5 and nv[0] == -5 and np.all(mask == 9) and np.all(en == 9.0)   # noqa: E731
    call = lambda h=dev.h, k=1, nn=n, xx=x, oo=out, no=n_out: lib.mtts_stft_trim_batch(h, k, _ptr(nn) if nn is not None else None, _ptr(xx) if xx is not None else None,   # noqa: E731
                                                                                        None, _ptr(oo) if oo is not None else None, _ptr(no) if no is not None else None,
                                                                                        _ptr(nv), _ptr(mask), _ptr(en))
    assert call() < 0 and err() == "mtts_stft_trim_batch: no VAD configuration loaded (mtts_stft_load_vad)" and untouched()
    load = lambda *a: lib.mtts_stft_load_vad(dev.h, *a)                                              # noqa: E731
    good = (16000, 30, 8, 6, -50.0, 0.1, 10.0)
    for bad, msg in (((22050, 30) + good[2:], "window_ms * sampling_rate = 661500 is not a multiple of 1000"),
                     ((16000, 30, 0) + good[3:], "ma_width outside 1 .. 64"), ((16000, 30, 65) + good[3:], "ma_width outside 1 .. 64"),
                     ((16000, 30, 8, 0) + good[4:], "max_silence outside 1 .. 64"), ((16000, 30, 8, 65) + good[4:], "max_silence outside 1 .. 64"),
                     (good[:5] + (-0.1, 10.0), "noise_quantile outside [0, 1]"), (good[:5] + (1.5, 10.0), "noise_quantile outside [0, 1]"),
                     (good[:5] + (float("nan"), 10.0), "noise_quantile outside [0, 1]"),
                     (good[:4] + (float("inf"), 0.1, 10.0), "non-finite threshold"), (good[:6] + (float("nan"),), "non-finite threshold"),
                     ((0, 30) + good[2:], "bad arguments"), ((16000, 0) + good[2:], "bad arguments")):
        assert load(*bad) != 0 and msg in err(), (bad, err())
    assert call() < 0 and "no VAD configuration loaded" in err()                                     # the refused loads loaded nothing
    assert lib.mtts_stft_load_vad(None, *good) != 0 and load(*good) == 0
    assert call(h=None) < 0 and untouched()
    for kw in (dict(nn=None), dict(xx=None), dict(oo=None), dict(no=None), dict(k=0), dict(k=-1)):
        assert call(**kw) < 0 and "bad arguments" in err() and untouched(), kw
    big = np.zeros(65536, np.int32) + 1
    assert call(k=65536, nn=big) < 0 and "more than 65535 utterances" in err() and untouched()
    assert call(nn=np.zeros(1, np.int32)) < 0 and "utterance 0: n_samples < 1" in err() and untouched()
    assert call(nn=np.asarray([4097 * W + 1], np.int32)) < 0 and f"utterance 0: {4097 * W + 1} samples exceed max_samples = {4097 * W}" in err() and untouched()
    assert call(nn=np.asarray([4097 * W], np.int32)) < 0 and "utterance 0: 4097 windows of 480 samples exceed the 4096 a workgroup holds" in err() and untouched()
    assert call() == 3 * W and n_out[0] == 3 * W and nv[0] == 0 and np.array_equal(out, x)           # and a good call after all of them
    dev.close()
    # the Python layer
    with pytest.raises(MttsError, match="not a multiple of 1000"):
        V.SilenceTrimmer(sampling_rate=22050, lib_path=lib_path)
    t = V.SilenceTrimmer(lib_path=lib_path)
    with pytest.raises(MttsError, match="no waveforms"):
        t.trim_batch([])
    with pytest.raises(MttsError, match="flags must hold"):
        t.trim_batch([x], flags=[[1, 1]])
    t.close()
    # the chained entry: both handles carry the reason, nothing is written
    emb = E.SpeakerEmbedder(synthetic_state_dict(3, **TINY), lib_path=lib_path, max_partials=4, **TINY)
    vec, cnt, ntr = np.full((1, 32), 7.0, np.float32), np.full(1, -1, np.int32), np.full(1, -1, np.int32)
    wav = np.zeros(30000, np.float32)
    args = lambda k=30000, w=wav, c=cnt: (1, _ptr(np.asarray([k], np.int32)), _ptr(w) if w is not None else None, 160, 77, 0.75, float("nan"), 0, _ptr(vec),   # noqa: E731
                                          _ptr(c) if c is not None else None, None, _ptr(ntr))
    both = lambda: (lib.mtts_stft_last_error(emb._dev.h).decode(), lib.mtts_dvector_last_error(emb.encoder.h).decode())   # noqa: E731
    clean = lambda: np.all(vec == 7.0) and cnt[0] == -1 and ntr[0] == -1                             # noqa: E731
    assert lib.mtts_dvector_embed_wavs_preprocessed(emb.encoder.h, emb._dev.h, *args()) != 0 and clean()
    assert both()[0] == both()[1] == "mtts_dvector_embed_wavs_preprocessed: no VAD configuration loaded (mtts_stft_load_vad)"
    assert lib.mtts_dvector_embed_wavs_preprocessed(emb.encoder.h, None, *args()) != 0 and "NULL STFT handle" in both()[1] and clean()
    emb.trimmer()
    assert lib.mtts_dvector_embed_wavs_preprocessed(emb.encoder.h, emb._dev.h, *args(w=None)) != 0 and "bad arguments" in both()[1] and clean()
    assert lib.mtts_dvector_embed_wavs_preprocessed(emb.encoder.h, emb._dev.h, *args(c=None)) != 0 and "bad arguments" in both()[1] and clean()
    assert lib.mtts_dvector_embed_wavs_preprocessed(emb.encoder.h, emb._dev.h, *args(k=0)) != 0 and "n_samples < 1" in both()[1] and clean()
    assert lib.mtts_dvector_embed_wavs_preprocessed(emb.encoder.h, emb._dev.h, *args(k=150)) != 0 and "too short for the reflection padding" in both()[1] and clean()
    norm = args()[:6] + (-30.0, 1) + args()[8:]
    assert lib.mtts_dvector_embed_wavs_preprocessed(emb.encoder.h, emb._dev.h, *norm) != 0 and "volume normalisation needs a resampler" in both()[0] and clean()
    long = np.zeros(16000 * 60, np.float32)                                                          # 2000 windows, but more partials than max_partials = 4
    assert lib.mtts_dvector_embed_wavs_preprocessed(emb.encoder.h, emb._dev.h, *args(k=len(long), w=long)) != 0 and "exceed the encoder's max_partials" in both()[1] and clean()
    assert lib.mtts_dvector_embed_wavs_preprocessed(emb.encoder.h, emb._dev.h, *args(k=16000 * 60 + 1)) != 0 and clean()   # (refused before `wav` is read)
    assert both()[0] == both()[1] == "mtts_dvector_embed_wavs_preprocessed: utterance 0: 960001 samples exceed max_samples = 960000"
    many = (65536, _ptr(np.full(65536, 30000, np.int32))) + args()[2:]
    assert lib.mtts_dvector_embed_wavs_preprocessed(emb.encoder.h, emb._dev.h, *many) != 0 and clean()
    assert both()[0] == both()[1] == "mtts_dvector_embed_wavs_preprocessed: more than 65535 utterances in one call"
    V.SilenceTrimmer(window_ms=10, _handle=emb._dev)                                                  # 160 samples <= filter_length / 2 = 200
    assert lib.mtts_dvector_embed_wavs_preprocessed(emb.encoder.h, emb._dev.h, *args()) != 0 and "too short for the reflection padding" in both()[0] and clean()
    # with a resampler the limits hold at the detector's rate, after out_len: 4097 windows of 160 samples from 22 050 Hz input
    rs = emb.resampler(22050)
    k = -(-4097 * 160 * 441 // 320)
    assert rs.output_length(k) // 160 == 4097 and rs.output_length(k) <= 16000 * 60
    assert lib.mtts_dvector_embed_wavs_preprocessed(emb.encoder.h, emb._dev.h, *args(k=k)) != 0 and clean()
    assert both()[0] == both()[1] == "mtts_dvector_embed_wavs_preprocessed: utterance 0: 4097 windows of 160 samples exceed the 4096 a workgroup holds"
    k = 16000 * 60 * 441 // 320 + 2
    assert lib.mtts_dvector_embed_wavs_preprocessed(emb.encoder.h, emb._dev.h, *args(k=k)) != 0 and clean()
    assert both()[0] == both()[1] and f"{rs.output_length(k)} resampled samples exceed max_samples = 960000" in both()[0]
    # the Python layer of the chained entry
    assert emb.last_trimmed_lengths is None
    with pytest.raises(ValueError, match="sampling_rate"):
        emb.trimmer(sampling_rate=8000)
    with pytest.raises(ValueError, match="sampling_rate"):
        emb.embed_utterances([np.zeros(30000, np.float32)], trim=dict(sampling_rate=8000))
    emb.close()


def test_errors_emulator():
    _check_errors(_emu())


@pytest.mark.gpu
def test_errors_gpu():
    _check_errors(None)


# ---- 7. resources ---------------------------------------------------------------------------------------------------------------------------------
def test_a_handle_without_a_vad_allocates_nothing_new():
    lib = _lib.load(_emu())
    for name in ("emu_live_allocs", "emu_alloc_calls", "emu_bad_frees"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = C.c_longlong, []
    live0, bad0 = lib.emu_live_allocs(), lib.emu_bad_frees()
    t = V.SilenceTrimmer(lib_path=_emu())                                                            # create + load_vad
    created = lib.emu_alloc_calls()
    t.load()
    assert lib.emu_alloc_calls() == created                                                          # a configuration is host state: no device memory
    rs = A.Resampler(22050, 16000, _handle=t._dev)
    x = O.speechlike(30000, 1, sr=22050)
    before = lib.emu_alloc_calls()
    rs.resample_batch([x])
    resample_only = lib.emu_alloc_calls() - before
    h2 = _Handle(16, 4, 1, 16000 * 120, 0, _emu())                                                    # the same call on a handle that never loaded a VAD
    rs2 = A.Resampler(22050, 16000, _handle=h2)
    before = lib.emu_alloc_calls()
    rs2.resample_batch([x])
    assert lib.emu_alloc_calls() - before == resample_only
    h2.close()
    before = lib.emu_alloc_calls()
    t.trim_batch([x])
    assert lib.emu_alloc_calls() > before                                                            # the first trim reserves its buffers ...
    before = lib.emu_alloc_calls()
    t.trim_batch([x[:20000]])
    assert lib.emu_alloc_calls() == before                                                           # ... and a smaller one reuses them
    t.close()
    assert lib.emu_live_allocs() == live0 and lib.emu_bad_frees() == bad0                            # destroy returns every block exactly once
