"""Device resampling and volume normalisation (csrc/resample.h through include/mtts.h: mtts_stft_load_resampler / resample_batch,
mtts_dvector_embed_wavs_resampled; meta_tts_amd/audio/resample.py and the opt-in wiring in evaluation.py / preprocessor.py).  CPU tests
run the device code through the SIMT emulator; the `-m gpu` twins run it on the MI355X.

What is pinned to what:
  * PARITY with librosa / resampy / resemblyzer is UNPINNED (none is available).  Pinned instead: tests/resample_oracle.py, the
    resampling sum as written, equals scipy.signal.resample_poly with the same Kaiser window to 1e-13 (five rate pairs x three presets).
  * device vs oracle, every output sample: |y_dev - y_f64| <= (taps + 2) 2^-24 sum |h32| |x| — the a-priori bound of an fp32 dot
    product of `taps` terms plus one rounding of every coefficient; it holds in any summation order and with FMA, so it carries no
    measured margin.  A float32 numpy restatement is held to the same bound.
  * bit identity (np.array_equal): an utterance's output alone, in any batch, at any position, across two calls; the chained entry
    against embed_utterances of resample_batch's host output.
  * volume: gain against the float64 value to n 2^-52 relative (a sum of n squares in another order, then log10 / pow to a few ulp);
    output against fp32(y gain) to 1 ulp.
  * filter quality (float64 oracle, kaiser_best): a 1 kHz sine comes out as the sine at the new rate to 1e-7, 500 samples from either
    edge (measured <= 1.2e-8 over the five pairs); a tone at new Nyquist + 0.6 (old Nyquist - new Nyquist) is suppressed to 8e-7 = 10 x
    the measured residue 7.93e-8 (worst of the four down-sampling pairs: 24000 -> 22050; the others 7.3e-9 .. 2.3e-8).

Measured (printed by the tests; worst ratio of error to bound over all samples of all cases):
  emulator : device 0.201, float32 numpy 0.141 (the largest ratios sit at utterance edges, where few taps contribute); gains: relative
             difference from float64 <= 1.1e-15 against gates of 4.8e-12 .. 6.6e-12; the 24 kHz corpus' feature tree differs from the
             oracle-resampled one by at most 2.5e-7 of the gate's scale
  MI355X   : not measured (the `-m gpu` twins have not been run on the device yet)"""
import json
import os
import random

import numpy as np
import pytest

import __graft_entry__ as ge
import resample_oracle as R
from meta_tts_amd import evaluation as E
from meta_tts_amd.audio import resample as A
from meta_tts_amd.engine import MttsError
from meta_tts_amd.speaker_encoder import synthetic_state_dict

TINY = dict(hidden=64, emb=32, layers=2)
FULL = dict(hidden=256, emb=256, layers=3)
CASES = [(p, "kaiser_best") for p in R.PAIRS] + [((22050, 16000), "scipy"), ((22050, 16000), "kaiser_fast")]


def _emu():
    return ge.build_emulator()


def _ragged(sr, seed, k=8):
    """k utterances of 0.05 .. 3 s at sr: chirps + noise."""
    g = np.random.RandomState(seed)
    secs = [0.05, 3.0] + list(g.uniform(0.05, 3.0, k - 2))
    return [R.chirps(int(s * sr), sr, seed * 100 + i) for i, s in enumerate(secs)]


# ---- 1. the oracle against scipy -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", R.PAIRS)
@pytest.mark.parametrize("preset", sorted(R.PRESETS))
def test_oracle_equals_scipy_resample_poly(pair, preset):
    signal = pytest.importorskip("scipy.signal")
    up, down, H, h = R.design(*pair, preset)
    assert (up, down) == A.ratio(*pair) and np.array_equal(h, A.resample_filter(*pair, preset)[3])
    zeros, beta, rolloff = R.PRESETS[preset]
    g = np.random.RandomState(1)
    for n in (1, 2, 10 * down, 10 * down + 1, 3001, 777):          # multiples of `down` and not, and a single sample
        x = g.standard_normal(n)
        y = R.resample(x, up, down, H, h)
        ys = signal.resample_poly(x, up, down, window=signal.firwin(2 * H + 1, rolloff / max(up, down), window=("kaiser", beta)))
        assert len(y) == len(ys) == A.output_length(n, up, down) == -(-n * up // down)
        assert np.abs(y - ys).max() <= 1e-13, (pair, preset, n, np.abs(y - ys).max())


def test_bank_layout_and_identity():
    up, down, H, h = A.resample_filter(22050, 16000, "kaiser_best")
    bank, lead = A.polyphase_bank(up, down, H, h)
    assert (up, down) == (320, 441) and bank.shape == (178, 320) and bank.dtype == np.float32 and lead == 89
    for p, t in ((0, 0), (7, 88), (319, 177), (100, 89)):
        off = (p * down) % up + (t - lead) * up
        assert bank[t, p] == (np.float32(h[off + H]) if abs(off) <= H else 0.0)
    assert A.resample_filter(16000, 16000) == (1, 1, 0, pytest.approx(np.ones(1)))
    with pytest.raises(ValueError, match="unknown resampling preset"):
        A.resample_filter(22050, 16000, "sinc_best")


# ---- 2. device against the oracle ------------------------------------------------------------------------------------------------------------
def _check_device_vs_oracle(lib_path):
    worst_dev = worst_32 = 0.0
    for k, ((orig, target), preset) in enumerate(CASES):
        rs = A.Resampler(orig, target, preset, lib_path=lib_path)
        up, down, H, h = R.design(orig, target, preset)
        wavs = _ragged(orig, 10 + k)
        got = rs.resample_batch(wavs)
        for w, y in zip(wavs, got):
            y64, scale = R.resample(w, up, down, H, h, return_abs=True)
            y32 = R.resample(w, up, down, H, h, np.float32)
            assert y.dtype == np.float32 and y.shape == y64.shape == (rs.output_length(len(w)),)
            bound = (rs.taps + 2) * 2.0 ** -24 * scale
            live = bound > 0
            assert np.all(np.abs(y - y64) <= bound) and np.all(np.abs(y32 - y64) <= bound), (orig, target, preset, len(w))
            worst_dev = max(worst_dev, float((np.abs(y - y64)[live] / bound[live]).max()))
            worst_32 = max(worst_32, float((np.abs(y32 - y64)[live] / bound[live]).max()))
        rs.close()
    print("max |y - f64| / bound: device %.3g, float32 numpy %.3g" % (worst_dev, worst_32))


def test_device_vs_oracle_emulator():
    _check_device_vs_oracle(_emu())


@pytest.mark.gpu
def test_device_vs_oracle_gpu():
    _check_device_vs_oracle(None)


# ---- 3. bit identity --------------------------------------------------------------------------------------------------------------------------
def _check_bit_identity(lib_path):
    rs = A.Resampler(24000, 22050, lib_path=lib_path)
    wavs = _ragged(24000, 3, 6) + [R.chirps(1, 24000, 5), R.chirps(1500, 24000, 6)]
    alone = [rs.resample_batch([w], normalize_dbfs=-30, return_gains=True) for w in wavs[:3]]      # small calls first: the workspace grows below
    batch, gains = rs.resample_batch(wavs, normalize_dbfs=-30, return_gains=True)
    rev, rev_gains = rs.resample_batch(wavs[::-1], normalize_dbfs=-30, return_gains=True)
    again, again_gains = rs.resample_batch(wavs, normalize_dbfs=-30, return_gains=True)
    pair = rs.resample_batch([wavs[4], wavs[1]], normalize_dbfs=-30)
    for i in range(len(wavs)):
        j = len(wavs) - 1 - i
        assert np.array_equal(batch[i], rev[j]) and np.array_equal(batch[i], again[i]) and gains[i] == rev_gains[j] == again_gains[i], i
        if i < 3:
            assert np.array_equal(batch[i], alone[i][0][0]) and gains[i] == alone[i][1][0], i
    assert np.array_equal(pair[0], batch[4]) and np.array_equal(pair[1], batch[1])
    rs.close()


def test_bit_identity_emulator():
    _check_bit_identity(_emu())


@pytest.mark.gpu
def test_bit_identity_gpu():
    _check_bit_identity(None)


# ---- 4. volume ----------------------------------------------------------------------------------------------------------------------------------
def _check_volume(lib_path):
    rs = A.Resampler(22050, 16000, lib_path=lib_path)
    loud, quiet = R.chirps(30000, 22050, 1), R.chirps(41000, 22050, 2, amp=0.004)
    plain = rs.resample_batch([loud, quiet])
    assert R.gain_of(plain[0]) == 1.0 and R.gain_of(plain[1]) > 1.0        # -30 dBFS lies between the two
    for increase_only in (True, False):
        out, gains = rs.resample_batch([loud, quiet], normalize_dbfs=-30.0, increase_only=increase_only, return_gains=True)
        for y, o, g in zip(plain, out, gains):
            want = R.gain_of(y, -30.0, increase_only)
            print("gain device %.17g, float64 %.17g, relative difference %.3g (gate %.3g)" % (g, want, abs(g - want) / want, len(y) * 2.0 ** -52))
            assert abs(g - want) <= len(y) * 2.0 ** -52 * want
            if want == 1.0:
                assert g == 1.0 and np.array_equal(o, y)                     # left as it is: bit-identical to the plain resample
            else:
                ref = (y.astype(np.float64) * want).astype(np.float32)
                assert np.all(np.abs(o - ref) <= np.spacing(np.abs(ref)))
                assert abs(10 * np.log10(np.mean(o.astype(np.float64) ** 2)) + 30.0) < 1e-5
    assert gains[0] < 1.0                                                    # increase_only off: the loud one is turned down
    host, g_host = A.normalize_volume(plain[1], -30.0, increase_only=True)
    assert g_host == R.gain_of(plain[1]) and A.normalize_volume(plain[0], -30.0, increase_only=True)[1] == 1.0
    silent = rs.resample_batch([np.zeros(500, np.float32)], normalize_dbfs=-30.0, return_gains=True)
    assert not silent[0][0].any() and silent[1][0] == 1.0
    pre = A.preprocess_wav([loud, quiet], 22050, trim_fn=lambda w: w[100:], resampler=rs)                 # resample -> -30 dBFS, increase only -> injected trim
    assert np.array_equal(pre[0], plain[0][100:]) and np.array_equal(pre[1], out[1][100:])
    rs.close()


def test_volume_emulator():
    _check_volume(_emu())


@pytest.mark.gpu
def test_volume_gpu():
    _check_volume(None)


# ---- 5. filter quality (the float64 oracle) ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", R.PAIRS)
def test_filter_quality_oracle(pair):
    orig, target = pair
    up, down, H, h = R.design(orig, target, "kaiser_best")
    t = np.arange(20000) / orig
    y = R.resample(np.sin(2 * np.pi * 1000 * t), up, down, H, h)
    err = np.abs(y - np.sin(2 * np.pi * 1000 * np.arange(len(y)) / target))[500:-500].max()
    print(f"{orig} -> {target}: 1 kHz sine error {err:.3g} (gate 1e-7)")
    assert err <= 1e-7
    if target < orig:                                                        # a tone between the new and the old Nyquist frequency
        f = target / 2 + 0.6 * (orig / 2 - target / 2)
        res = np.abs(R.resample(np.sin(2 * np.pi * f * t), up, down, H, h))[500:-500].max()
        print(f"{orig} -> {target}: residue of a {f:.0f} Hz tone {res:.3g} (gate 8e-7)")
        assert res <= 8e-7


# ---- 6. the chained entry -----------------------------------------------------------------------------------------------------------------------
def _check_chain(lib_path, dims):
    emb = E.SpeakerEmbedder(synthetic_state_dict(3, **dims), lib_path=lib_path, max_partials=6, **dims)
    lengths = [71000, 22050, 45632, 28000, 56001]
    wavs = [R.chirps(n, 22050, 40 + i, amp=(0.01 if i % 2 else 1.0)) for i, n in enumerate(lengths)]
    pre = emb.resampler(22050).resample_batch(wavs, normalize_dbfs=-30)
    assert [len(p) for p in pre] == [-(-n * 320 // 441) for n in lengths]
    assert sum(len(E.compute_partial_slices(len(p))[1]) for p in pre) > 6                          # at least two chunks
    want_vec, want_sl = emb.embed_utterances(pre, return_slices=True)
    got_vec, got_sl = emb.embed_utterances(wavs, return_slices=True, source_rate=22050, normalize_dbfs=-30)
    assert np.array_equal(got_vec, want_vec)
    for n, a, b in zip(lengths, got_sl, want_sl):
        assert np.array_equal(a, b) and len(a) == len(E.compute_partial_slices(-(-n * 320 // 441))[1])
    # no normalisation, and 16 kHz input through the identity bank
    assert np.array_equal(emb.embed_utterances(wavs[:2], source_rate=22050), emb.embed_utterances(emb.resampler(22050).resample_batch(wavs[:2])))
    assert np.array_equal(emb.embed_utterances(pre[:2], source_rate=16000), emb.embed_utterances(pre[:2]))
    assert np.array_equal(emb.embed_utterances(wavs, source_rate=22050, normalize_dbfs=-30), want_vec)   # after the bank was swapped and restored
    with pytest.raises(ValueError, match="needs source_rate"):
        emb.embed_utterances(pre, normalize_dbfs=-30)
    emb.close()


def test_chain_emulator():
    _check_chain(_emu(), TINY)


@pytest.mark.gpu
def test_chain_gpu():
    _check_chain(None, FULL)


# ---- 7. end to end ------------------------------------------------------------------------------------------------------------------------------
def _check_result_tree(lib_path, dims, tmp_path):
    """A Saver-shaped result tree whose wavs are at 22 050 Hz (what Saver, the vocoder and Griffin-Lim write)."""
    from scipy.io import wavfile
    n_speaker, n_sample = 5, 1
    root, raw, sq = str(tmp_path), os.path.join(str(tmp_path), "raw"), []
    g = np.random.RandomState(0)

    def write(path, seed):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        wavfile.write(path, 22050, (R.chirps(int(g.randint(12000, 30000)), 22050, seed) * 20000).astype(np.int16))

    for s in range(n_speaker):
        for u in range(4):
            write(os.path.join(raw, f"{100 + s}", f"{100 + s}_{u:02d}.wav"), 1000 * s + u)
        sq.append({"sup_id": [f"{100 + s}_03"], "qry_id": [f"{100 + s}_00"]})
    res = os.path.join(root, "result", "m1")
    for data_id, q in enumerate(sq):
        d = os.path.join(res, "audio", "Testing", f"test_{data_id:03d}")
        write(os.path.join(d, f"{q['qry_id'][0]}.recon.wav"), 5000 + data_id)
        write(os.path.join(d, f"{q['qry_id'][0]}.step_100000-FTstep_5.synth.wav"), 6000 + data_id)
    json.dump(sq, open(os.path.join(res, "test_SQids.json"), "w"))
    dirs = {"recon": res, "m1": res, "real": raw, "enrollment": raw}
    emb = E.SpeakerEmbedder(synthetic_state_dict(3, **dims), lib_path=lib_path, max_partials=8, **dims)
    cfg = E.EvalConfig("Tiny", dirs, n_speaker, n_sample, [("m1", [5])], work_dir=os.path.join(root, "plain"))
    with pytest.raises(MttsError, match="sampling rate 22050"):
        E.WavsToDvector(cfg, emb, rng=random.Random(3))                                           # resample=False still raises
    cfg = E.EvalConfig("Tiny", dirs, n_speaker, n_sample, [("m1", [5])], work_dir=os.path.join(root, "work"))
    w = E.WavsToDvector(cfg, emb, rng=random.Random(3), resample=True)
    npy = lambda name: np.load(os.path.join(root, "work", "npy", "Tiny", name), allow_pickle=True)   # noqa: E731
    assert npy("real_dvector.npy").shape == npy("recon_dvector.npy").shape == npy("m1_step5_dvector.npy").shape == (n_speaker, dims["emb"])
    assert npy("pair_dvector.npy").shape == (2, 4 * n_speaker, dims["emb"]) and npy("centroid_dvector.npy").shape == (n_speaker, dims["emb"])
    from meta_tts_amd.preprocessor import read_wav
    first = emb.embed_utterances(emb.resampler(22050).resample_batch([read_wav(w.real_filelist[0])[0]], normalize_dbfs=-30))[0]
    assert np.array_equal(first, w.dvector_list_dict["real"][0])                                  # a row of the walk = that file alone, preprocessed on the host side
    assert np.allclose(np.linalg.norm(npy("real_dvector.npy"), axis=1), 1, atol=1e-5)
    emb.close()


def test_result_tree_at_22050_emulator(tmp_path):
    _check_result_tree(_emu(), TINY, tmp_path)


@pytest.mark.gpu
def test_result_tree_at_22050_gpu(tmp_path):
    _check_result_tree(None, FULL, tmp_path)


def _check_corpus_24k(lib_path, tmp_path):
    """The `small` fixture corpus of tests/test_preprocess.py re-recorded at 24 kHz: build_from_path(resample=True) on the 24 kHz files
    against build_from_path(resample=False) on the same files resampled by the float64 oracle (written as float32 wavs)."""
    import test_preprocess as TP
    from scipy.io import wavfile
    trees = {}
    for kind in ("device", "oracle"):
        c = TP._Corpus("small", str(tmp_path / kind), lib_path)
        c.pp.close()
        c.pp = TP.P.Preprocessor(c.cfg, max_samples=22050 * 30, lib_path=lib_path)
        f0_of = c.write_raw()
        sr = c.pp.sampling_rate
        up, down, H, h = R.design(24000, sr, "kaiser_best")
        f0 = {}
        for spk, base in c.utts:                                                                  # a longer 24 kHz recording with the fixture's alignment
            n22 = len(TP.G[f"{c.name}|{base}|wav"])
            w24 = R.chirps(-(-n22 * 24000 // sr) + 240, 24000, len(f0) + 70)
            path = os.path.join(c.pp.in_dir, "train", spk, base + ".wav")
            w22 = R.resample(w24, up, down, H, h).astype(np.float32)
            wavfile.write(path, 24000, w24) if kind == "device" else wavfile.write(path, sr, w22)
            f0[base] = c.item(spk, base)[5]
        order = iter([b for _, b in sorted(c.utts)])
        out = c.pp.build_from_path(f0_fn=lambda wav, rate, hop: f0[next(order)], batch_utterances=3, resample=(kind == "device"))
        trees[kind] = (c.pp.out_dir, out)
        if kind == "device":
            with pytest.raises(MttsError, match="sampling rate 24000 differs"):
                c.pp.build_from_path(f0_fn=lambda *a: None, batch_utterances=3)
        c.pp.close()
    (da, oa), (db, ob) = trees["device"], trees["oracle"]
    assert oa == ob and oa["train"]
    worst = 0.0
    for feat in ("mel", "pitch", "energy", "duration"):
        names = sorted(os.listdir(os.path.join(da, feat)))
        assert names == sorted(os.listdir(os.path.join(db, feat))) and names
        for nm in names:
            a, b = np.load(os.path.join(da, feat, nm)), np.load(os.path.join(db, feat, nm))
            assert a.shape == b.shape and a.dtype == b.dtype
            if feat == "mel":                                                                     # log of a clamped value: compared above the clamp (tests/test_stft.py)
                live = b > np.log(2e-5)
                a, b = np.exp(a[live]), np.exp(b[live])
            worst = max(worst, float(np.abs(a - b).max() / max(1.0, np.abs(b).max())))
            np.testing.assert_allclose(a, b, rtol=0, atol=1e-6 * max(1.0, float(np.abs(b).max())))
    print("feature trees, 24 kHz corpus resampled on the device vs by the float64 oracle: max difference %.3g (gate 1e-6 of the larger of 1 and the file's maximum)" % worst)
    assert json.load(open(os.path.join(da, "speakers.json"))) == json.load(open(os.path.join(db, "speakers.json")))
    sa, sb = json.load(open(os.path.join(da, "stats.json"))), json.load(open(os.path.join(db, "stats.json")))
    for k in sa:
        np.testing.assert_allclose(sa[k], sb[k], rtol=1e-6, atol=1e-6)


def test_corpus_24k_through_preprocessor_emulator(tmp_path):
    _check_corpus_24k(_emu(), tmp_path)


@pytest.mark.gpu
def test_corpus_24k_through_preprocessor_gpu(tmp_path):
    _check_corpus_24k(None, tmp_path)


# ---- 8. errors ----------------------------------------------------------------------------------------------------------------------------------
def _check_errors(lib_path):
    from meta_tts_amd.audio.stft import _Handle
    dev = _Handle(16, 4, 1, 4000, 0, lib_path)
    lib = dev.lib
    x, n = np.zeros(100, np.float32), np.asarray([100], np.int32)
    out = np.full(200, 7.0, np.float32)
    nan = float("nan")
    assert lib.mtts_stft_resample_batch(dev.h, 1, A._ptr(n), A._ptr(x), nan, 0, A._ptr(out), None) != 0
    assert "no resampler loaded" in lib.mtts_stft_last_error(dev.h).decode()
    emb = E.SpeakerEmbedder(lib_path=lib_path, encoder=False)
    cnt, sl = np.full(1, -1, np.int32), np.zeros((4, 160, 40), np.float32)
    args = (1, A._ptr(np.asarray([30000], np.int32)), A._ptr(np.zeros(30000, np.float32)), 160, 77, 0.75, nan, 0, None, A._ptr(cnt), A._ptr(sl))
    assert lib.mtts_dvector_embed_wavs_resampled(None, emb._dev.h, *args) != 0
    assert lib.mtts_stft_last_error(emb._dev.h).decode() == "mtts_dvector_embed_wavs_resampled: no resampler loaded (mtts_stft_load_resampler)"
    assert lib.mtts_dvector_embed_wavs_resampled(None, None, *args) != 0 and cnt[0] == -1           # NULL STFT handle
    emb.resampler(22050)
    short = (1, A._ptr(np.asarray([250], np.int32)), A._ptr(np.zeros(250, np.float32))) + args[3:]
    assert lib.mtts_dvector_embed_wavs_resampled(None, emb._dev.h, *short) != 0                     # 182 samples at 16 kHz
    assert "waveform too short for the reflection padding" in lib.mtts_stft_last_error(emb._dev.h).decode()
    emb.close()
    rs = A.Resampler(24000, 22050, _handle=dev)
    bank = rs.bank
    assert lib.mtts_stft_load_resampler(None, rs.up, rs.down, rs.taps, rs.lead, A._ptr(bank)) != 0      # NULL handle
    assert lib.mtts_stft_resample_batch(None, 1, A._ptr(n), A._ptr(x), nan, 0, A._ptr(out), None) != 0
    for bad in ((0, rs.down, rs.taps, rs.lead), (rs.up, 0, rs.taps, rs.lead), (rs.up, rs.down, 0, 0), (rs.up, rs.down, rs.taps, rs.taps)):
        assert lib.mtts_stft_load_resampler(dev.h, *bad, A._ptr(bank)) != 0 and "bad arguments" in lib.mtts_stft_last_error(dev.h).decode()
    assert lib.mtts_stft_load_resampler(dev.h, 1, 40, 16, 8, A._ptr(np.zeros(16, np.float32))) != 0   # 255 * 40 + 17 input samples per 256 outputs
    assert "exceeds the 4096 samples a workgroup stages" in lib.mtts_stft_last_error(dev.h).decode()
    good = rs.resample_batch([x + 0.5])                                                             # the refused loads left the bank as it was
    with pytest.raises(MttsError, match="no waveforms"):
        rs.resample_batch([])
    with pytest.raises(MttsError, match=r"utterance 1: 4135 resampled samples exceed max_samples = 4000"):
        rs.resample_batch([x, np.zeros(4500, np.float32)])
    assert lib.mtts_stft_resample_batch(dev.h, 0, A._ptr(n), A._ptr(x), nan, 0, A._ptr(out), None) != 0
    assert lib.mtts_stft_resample_batch(dev.h, 1, A._ptr(np.zeros(1, np.int32)), A._ptr(x), nan, 0, A._ptr(out), None) != 0
    assert "utterance 0: n_in < 1" in lib.mtts_stft_last_error(dev.h).decode()
    assert lib.mtts_stft_resample_batch(dev.h, 1, A._ptr(n), None, nan, 0, A._ptr(out), None) != 0 and np.all(out == 7.0)
    with pytest.raises(MttsError, match="converts 24000 Hz -> 22050 Hz"):
        rs(x, 16000)
    assert np.array_equal(rs(x + 0.5, 24000), good[0])
    dev.close()


def test_errors_emulator():
    _check_errors(_emu())


@pytest.mark.gpu
def test_errors_gpu():
    _check_errors(None)
