"""Speaker-similarity evaluation (csrc/speakereval.h through include/mtts.h: mtts_stft_power_mel_batch, mtts_dvector_embed_wavs /
embed_device / cosine_indexed / centroids; meta_tts_amd/evaluation.py).  CPU tests run the device code through the SIMT emulator
(tiny encoder dimensions, the real 400 / 160 / 40 front-end); the `-m gpu` twins run the LSTM(40, 256, 3) encoder on the MI355X.

What is pinned to what:
  * scoring: tests/golden/speaker_eval.npz — the reference's own PairSimilarity / centroid / CentroidSimilarity / get_eer on seeded
    synthetic d-vectors (tests/golden/make_speaker_eval_golden.py).  Similarities and centroids: the arbiter rule element-wise,
    |device - f64| <= 3 |reference_f32 - f64| + 1e-7.  EER, AUC (ratios of counts) and the threshold (one of the scores): EQUAL to the
    reference's values, computed by this project's numpy DET / ROC from the fixture's pair similarities; eer.txt byte for byte.
  * front-end and partial rule: PARITY UNPINNED (resemblyzer / librosa are not available) — tests/spk_oracle.py, a float64
    restatement of the published recipe, plus hand-computed slice cases.  Mel power: per utterance, err(X) = max |X - f64| / m with
    m = the utterance's largest mel value (the power mel spans many decades) — the max-norm form of oracle/arbiter.py's gate, which is
    relative to max |reference| — and err(device) <= 3 err(torch_f32) + 1e-7.  (Element by element the rule cannot hold between two
    independent fp32 roundings: wherever the torch run happens to land within 1e-8 m of float64 it would demand the same of the
    device.)  d-vectors: 1 - cos(device, f64) <= 3 (1 - cos(torch_f32, f64)) + 1e-6.
  * bit-identity (np.array_equal): an utterance's slices and d-vector alone, first / last in a batch, across a chunk boundary, after
    the workspace has grown.

Measured (printed by the tests; max over the utterances):
  emulator : mel err(device) 9.2e-7 against err(torch_f32) 4.9e-7; d-vector 1 - cos 2.8e-14 against 4.7e-15 (tiny encoder); scoring: |device - f64| <= 3.1e-8
             everywhere (one rounding of the float64 result) against |reference_f32 - f64| up to 2.3e-7
  MI355X   : mel err(device) 9.97e-7 against err(torch_f32) 7.64e-7; d-vector 1 - cos 9.8e-14 against 5.8e-15 (LSTM(40, 256, 3)); scoring as above"""
import json
import os
import random

import numpy as np
import pytest

import __graft_entry__ as ge
import spk_oracle as O
from meta_tts_amd import data as D
from meta_tts_amd import evaluation as E
from meta_tts_amd.engine import MttsError
from meta_tts_amd.speaker_encoder import synthetic_state_dict

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "speaker_eval.npz"))
TINY = dict(hidden=64, emb=32, layers=2)
FULL = dict(hidden=256, emb=256, layers=3)
LENGTHS = [52000, 16000, 33111, 48000, 20480, 41000]      # unequal; 16000 and 20480 are shorter than one 25600-sample window


def _emu():
    return ge.build_emulator()


def _embedder(lib_path, dims, **kw):
    return E.SpeakerEmbedder(synthetic_state_dict(3, **dims), lib_path=lib_path, **dims, **kw)


def _wavs():
    """Chirps + noise of unequal lengths, and one white-noise utterance: its energy is spread over every mel bin, so the max-norm gates
    below also see the upper bins, which the chirps leave four decades under their maximum."""
    return [O.chirps(n, 100 + i) for i, n in enumerate(LENGTHS)] + [(0.3 * np.random.RandomState(9).standard_normal(30000)).astype(np.float32)]


# ---- the partial rule ------------------------------------------------------------------------------------------------------------------
def test_partial_slices_hand_computed_cases():
    """frame_step = round(16000 / 1.3 / 160) = 77; a window is 160 frames = 25600 samples."""
    assert E.frame_step_of(1.3) == 77
    sl = lambda *ab: [slice(a, b) for a, b in ab]   # noqa: E731
    # shorter than one window: ceil(16001 / 160) = 101 frames, steps = max(1, 101 - 160 + 78) = 19 -> one window; its coverage 0.625 is
    # below 0.75 but it is the only one.  The waveform is zero-extended to 25600.
    assert E.compute_partial_slices(16000) == (sl((0, 25600)), sl((0, 160)))
    # an exact multiple: 161 frames, steps = 79 -> windows at 0 and 77; the second covers (25600 - 12320) / 25600 = 0.52 -> dropped
    assert E.compute_partial_slices(25600) == (sl((0, 25600)), sl((0, 160)))
    # dropped for coverage: 188 frames, steps = 106 -> 0, 77; (30000 - 12320) / 25600 = 0.69 < 0.75
    assert E.compute_partial_slices(30000) == (sl((0, 25600)), sl((0, 160)))
    # kept: 201 frames, steps = 119 -> 0, 77; (32000 - 12320) / 25600 = 0.77 >= 0.75; zero-extension to (77 + 160) * 160 = 37920
    assert E.compute_partial_slices(32000) == (sl((0, 25600), (12320, 37920)), sl((0, 160), (77, 237)))
    # three seconds: 301 frames, steps = 219 -> 0, 77, 154; (48000 - 24640) / 25600 = 0.91
    assert E.compute_partial_slices(48000)[1] == sl((0, 160), (77, 237), (154, 314))
    for n in list(range(201, 60000, 997)) + [25599, 25601, 31519, 31520, 31521]:
        assert E.compute_partial_slices(n) == O.partial_slices(n), n


# ---- front-end and d-vectors against the float64 restatement -----------------------------------------------------------------------------
def _check_front_end(lib_path, dims, max_partials):
    wavs = _wavs()
    emb = _embedder(lib_path, dims, max_partials=max_partials)
    assert sum(len(E.compute_partial_slices(len(w))[1]) for w in wavs) > max_partials                # at least two chunks
    mels = emb.wav_to_mel_spectrogram(wavs)
    vec, slices = emb.embed_utterances(wavs, return_slices=True)
    worst = [0.0, 0.0, 0.0, 0.0]
    for w, mel, sl, v in zip(wavs, mels, slices, vec):
        r64, r32 = O.mel_power(w), O.mel_power(w, np.float32)
        assert mel.shape == r64.shape and mel.dtype == np.float32
        m = r64.max()
        if len(w) == 30000:
            assert r64.max(axis=0).min() > 0.02 * m                                            # the broadband utterance: every mel bin within 50x of the loudest
        dev, ref = np.abs(mel - r64) / m, np.abs(r32 - r64) / m
        worst[0], worst[1] = max(worst[0], dev.max()), max(worst[1], ref.max())
        assert dev.max() <= 3 * ref.max() + 1e-7, (dev.max(), ref.max())
        s64, s32 = O.mel_slices(w), O.mel_slices(w, np.float32)
        assert sl.shape == s64.shape == (len(E.compute_partial_slices(len(w))[1]), 160, 40)
        m = s64.max()
        assert np.abs(sl - s64).max() / m <= 3 * np.abs(s32 - s64).max() / m + 1e-7
        e64, e32 = O.embed(emb.encoder.state, w, **dims), O.embed(emb.encoder.state, w, np.float32, **dims)
        cos = lambda a, b: float(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)))   # noqa: E731
        d_dev, d_ref = 1 - cos(v.astype(np.float64), e64), 1 - cos(e32.astype(np.float64), e64)
        worst[2], worst[3] = max(worst[2], d_dev), max(worst[3], d_ref)
        assert abs(np.linalg.norm(v) - 1) < 1e-5
        assert d_dev <= 3 * max(d_ref, 0.0) + 1e-6, (d_dev, d_ref)
    print("mel max |device - f64| / m %.3g, |f32 - f64| / m %.3g; d-vector 1 - cos device %.3g, f32 %.3g" % tuple(worst))
    emb.close()


def test_front_end_and_dvectors_emulator():
    _check_front_end(_emu(), TINY, 6)


@pytest.mark.gpu
def test_front_end_and_dvectors_gpu():
    _check_front_end(None, FULL, 6)


# ---- bit-identity ------------------------------------------------------------------------------------------------------------------------
def _check_bit_identity(lib_path, dims):
    wavs = _wavs()
    emb = _embedder(lib_path, dims, max_partials=6)
    alone = [emb.embed_utterances([w], return_slices=True) for w in wavs[:3]]            # small calls first: the workspace grows below
    vec, slices = emb.embed_utterances(wavs, return_slices=True)                        # chunks of <= 6 partials: boundaries inside
    rev_vec, rev_slices = emb.embed_utterances(wavs[::-1], return_slices=True)           # first <-> last, other chunk boundaries
    again = [emb.embed_utterances([w], return_slices=True) for w in wavs]                # after the workspace has grown
    big = _embedder(lib_path, dims, max_partials=64)                                     # one chunk
    one_vec, one_slices = big.embed_utterances(wavs, return_slices=True)
    for i in range(len(wavs)):
        j = len(wavs) - 1 - i
        for v, s in ((rev_vec[j], rev_slices[j]), (again[i][0][0], again[i][1][0]), (one_vec[i], one_slices[i])) + (((alone[i][0][0], alone[i][1][0]),) if i < 3 else ()):
            assert np.array_equal(v, vec[i]) and np.array_equal(s, slices[i]), i
        assert np.array_equal(emb.reference_mel_slices(wavs[i]), slices[i])
    emb.close()
    big.close()


def test_bit_identity_emulator():
    _check_bit_identity(_emu(), TINY)


@pytest.mark.gpu
def test_bit_identity_gpu():
    _check_bit_identity(None, FULL)


@pytest.mark.gpu
def test_two_streams_are_ordered_by_events_gpu():
    """The two handles on streams of their own (front-end of chunk k + 1 overlapping the encoder of chunk k): same bits as on one stream."""
    import torch
    wavs = _wavs()
    emb = _embedder(None, FULL, max_partials=6)
    want = emb.embed_utterances(wavs, return_slices=True)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    emb.set_streams(s1.cuda_stream, s2.cuda_stream)
    for _ in range(3):
        got = emb.embed_utterances(wavs, return_slices=True)
        assert np.array_equal(got[0], want[0]) and all(np.array_equal(a, b) for a, b in zip(got[1], want[1]))
    emb.set_streams(0, 0)
    emb.close()


def _check_embed_device_matches_host_entry(lib_path, dims):
    """mtts_dvector_embed (host mels, launch queue) and the device chain agree to fp32 rounding on the same slices."""
    emb = _embedder(lib_path, dims, max_partials=16)
    vec, slices = emb.embed_utterances(_wavs()[:2], return_slices=True)
    stack = np.concatenate(slices)
    bounds = np.cumsum([0] + [len(s) for s in slices])
    host, host_part = emb.encoder.embed(stack, [slice(int(a), int(b)) for a, b in zip(bounds[:-1], bounds[1:])], return_partials=True)
    np.testing.assert_allclose(vec, host, rtol=0, atol=2e-6)
    # mtts_dvector_embed_device called directly on a stack in device memory (the emulator's device memory is the host's), with partial_out
    if lib_path is None:
        import torch
        dev_stack = torch.from_numpy(stack).cuda()
        torch.cuda.synchronize()
        ptr = dev_stack.data_ptr()
    else:
        stack = np.ascontiguousarray(stack)
        ptr = stack.ctypes.data
    direct, direct_part = emb.encoder.embed_device(ptr, len(stack), bounds, return_partials=True)
    assert np.array_equal(direct, vec)                                                   # the same fixed-tile forward as the chain
    np.testing.assert_allclose(direct_part, host_part, rtol=0, atol=2e-6)
    assert direct_part.shape == (len(stack), dims["emb"]) and np.allclose(np.linalg.norm(direct_part, axis=1), 1, atol=1e-5)
    with pytest.raises(MttsError, match="offsets must cover"):
        emb.encoder.embed_device(ptr, len(stack), bounds[:-1])
    emb.close()


def test_embed_device_matches_host_entry_emulator():
    _check_embed_device_matches_host_entry(_emu(), TINY)


@pytest.mark.gpu
def test_embed_device_matches_host_entry_gpu():
    _check_embed_device_matches_host_entry(None, FULL)


# ---- errors -------------------------------------------------------------------------------------------------------------------------------
def _check_errors(lib_path, dims):
    emb = _embedder(lib_path, dims, max_partials=4)
    good = _wavs()[1:3]
    before = emb.embed_utterances(good, return_slices=True)
    with pytest.raises(MttsError, match=r"utterance 1: waveform too short for the reflection padding \(need n_samples > filter_length / 2 = 200\)"):
        emb.embed_utterances([good[0], np.zeros(200, np.float32)])
    with pytest.raises(MttsError, match=r"utterance 1: 9 partial utterances exceed the encoder's max_partials = 4"):
        emb.embed_utterances([good[0], O.chirps(123457, 5)])
    with pytest.raises(MttsError, match="waveform too short"):
        emb.wav_to_mel_spectrogram([np.zeros(100, np.float32)])
    lib, n = emb.lib, np.asarray([len(good[0])], np.int32)
    out, cnt = np.full((1, emb.emb), 7.0, np.float32), np.full(1, -1, np.int32)
    args = (E._ptr(n), E._ptr(good[0]), 160, 77, 0.75)
    assert lib.mtts_dvector_embed_wavs(emb.encoder.h, emb._dev.h, 1, None, *args[1:], E._ptr(out), E._ptr(cnt), None) != 0
    assert "NULL" in lib.mtts_stft_last_error(emb._dev.h).decode() and "NULL" in lib.mtts_dvector_last_error(emb.encoder.h).decode()
    assert lib.mtts_dvector_embed_wavs(emb.encoder.h, emb._dev.h, 1, *args, None, E._ptr(cnt), None) != 0           # no output
    assert lib.mtts_dvector_embed_wavs(None, emb._dev.h, 1, *args, E._ptr(out), E._ptr(cnt), None) != 0             # front-end only needs slices_out
    assert lib.mtts_dvector_embed_wavs(emb.encoder.h, None, 1, *args, E._ptr(out), E._ptr(cnt), None) != 0
    assert lib.mtts_dvector_embed_wavs(emb.encoder.h, emb._dev.h, 1, *args[:2], 80, 77, 0.75, E._ptr(out), E._ptr(cnt), None) != 0
    assert "the encoder expects partials of 160 x 40" in lib.mtts_stft_last_error(emb._dev.h).decode()
    assert np.all(out == 7.0) and np.all(cnt == -1)                                     # nothing was written by a refused call
    if lib_path is not None:   # the emulator's hipSetDevice takes any ordinal: an encoder created on device 1 against the STFT handle on device 0
        other = E.DVectorEncoder(synthetic_state_dict(3, **dims), device=1, lib_path=lib_path, **dims)
        assert lib.mtts_dvector_embed_wavs(other.h, emb._dev.h, 1, *args, E._ptr(out), E._ptr(cnt), None) != 0
        for msg in (lib.mtts_stft_last_error(emb._dev.h).decode(), lib.mtts_dvector_last_error(other.h).decode()):
            assert msg == "mtts_dvector_embed_wavs: the encoder and the STFT handle are on different devices"
        assert np.all(out == 7.0) and np.all(cnt == -1)
        other.close()
    with pytest.raises(MttsError, match="index out of range"):
        emb.cosine_similarity(np.ones((2, 8)), np.ones((2, 8)), [0, 2], [0, 1])
    after = emb.embed_utterances(good, return_slices=True)                              # the handles are as they were
    assert np.array_equal(before[0], after[0]) and all(np.array_equal(a, b) for a, b in zip(before[1], after[1]))
    emb.close()


def test_errors_emulator():
    _check_errors(_emu(), TINY)


@pytest.mark.gpu
def test_errors_gpu():
    _check_errors(None, FULL)


# ---- scoring against the reference's fixture -----------------------------------------------------------------------------------------------
def _arbiter(name, dev, ref32, f64):
    dev, ref32 = np.asarray(dev, np.float64), np.asarray(ref32, np.float64)
    assert dev.shape == ref32.shape == f64.shape, name
    e_dev, e_ref = np.abs(dev - f64), np.abs(ref32 - f64)
    print(f"{name}: max |device - f64| {e_dev.max():.3g}, max |reference_f32 - f64| {e_ref.max():.3g}, max |device - reference| {np.abs(dev - ref32).max():.3g}")
    assert np.all(e_dev <= 3 * e_ref + 1e-7), name


def _fixture_config(tmp_path):
    modes = {}
    for key in G["modes"]:
        m, s = str(key).rsplit("_step", 1)
        modes.setdefault(m, []).append(int(s))
    return E.EvalConfig("Synthetic", {}, int(G["n_speaker"]), int(G["n_sample"]), list(modes.items()), work_dir=str(tmp_path))


def _check_scoring(lib_path, tmp_path):
    emb = _embedder(lib_path, TINY, max_partials=4)
    cfg = _fixture_config(tmp_path)
    cuts = np.cumsum(G["enrollment_sizes"])[:-1]
    cent = emb.centroids(np.split(G["enrollment"], cuts))
    assert cent.dtype == np.float32
    _arbiter("centroid", cent, G["centroid"], G["centroid_f64"])
    assert np.array_equal(cent, emb.centroids(np.split(G["enrollment"], cuts)))           # deterministic
    p = E.PairSimilarity(cfg, emb)
    c = E.CentroidSimilarity(cfg, emb, shuffle_map=G["shuffle_map"])
    for mode in ["recon", "real", "pair"] + [str(m) for m in G["modes"]]:
        p.dvector_list_dict[mode] = c.dvector_list_dict[mode] = G[f"dvector|{mode}"]
    c.dvector_list_dict["centroid"] = cent                                               # the device's own centroids: the whole chain
    for mode in ["recon", "real"] + [str(m) for m in G["modes"]]:
        sim = p.compute_pair_similarity(G[f"dvector|{mode}"])
        assert sim.dtype == np.float32
        _arbiter(f"pair_sim {mode}", sim, G[f"pair_sim|{mode}"], G[f"pair_sim_f64|{mode}"])
        p.pair_similarity_dict[mode] = sim
    # the whole chain: EER and AUC from the DEVICE's similarities equal the reference's (the generator asserts that opposite-label scores are
    # at least 1e-6 apart, four times the largest device-vs-reference difference above, so no pair of them can change order)
    v = E.SpeakerVerification(cfg)
    v.pair_similarity_dict = p.pair_similarity_dict
    v.get_eer()
    v.get_auc()
    for mode in v.pair_similarity_dict:
        assert v.eer_dict[mode] == float(G[f"eer|{mode}"]), mode
        assert (mode in v.auc_dict) == (f"auc|{mode}" in G) and (mode not in v.auc_dict or v.auc_dict[mode] == float(G[f"auc|{mode}"])), mode
        at = np.flatnonzero(G[f"pair_sim|{mode}"].flatten() == G[f"threshold|{mode}"])           # the threshold is the SAME score, as the device computed it
        assert v.threshold_dict[mode] in v.pair_similarity_dict[mode].flatten()[at], mode
    for mode in ["recon_random", "recon"] + [str(m) for m in G["modes"]]:
        _arbiter(f"centroid_sim {mode}", c.compute_centroid_similarity(mode), G[f"centroid_sim|{mode}"], G[f"centroid_sim_f64|{mode}"])
    emb.close()


def test_scoring_vs_reference_fixture_emulator(tmp_path):
    _check_scoring(_emu(), tmp_path)


@pytest.mark.gpu
def test_scoring_vs_reference_fixture_gpu(tmp_path):
    _check_scoring(None, tmp_path)


def test_eer_auc_threshold_equal_the_reference(tmp_path):
    v = E.SpeakerVerification(_fixture_config(tmp_path))
    modes = ["recon", "real"] + [str(m) for m in G["modes"]]
    v.pair_similarity_dict = {m: G[f"pair_sim|{m}"] for m in modes}
    v.get_eer()
    v.get_auc()
    for m in modes:
        print(m, v.eer_dict[m], v.threshold_dict[m], v.auc_dict.get(m))
        assert v.eer_dict[m] == float(G[f"eer|{m}"]) and (m in v.auc_dict) == (f"auc|{m}" in G) and (m not in v.auc_dict or v.auc_dict[m] == float(G[f"auc|{m}"]))
        assert v.threshold_dict[m] == G[f"threshold|{m}"] and v.threshold_dict[m].dtype == G[f"threshold|{m}"].dtype
    assert open(v.output_path).read() == str(G["eer_txt"][()])
    assert v.output_path == os.path.join(str(tmp_path), "txt", "Synthetic", "eer.txt")


def test_shuffle_map_invariants():
    m = E.custom_shuffle_map(5, 3, random.Random(1))
    E.check_shuffle_map(m, 5, 3)
    E.check_shuffle_map(G["shuffle_map"], int(G["n_speaker"]), int(G["n_sample"]))
    with pytest.raises(ValueError, match="own speaker"):
        E.check_shuffle_map(list(range(15)), 5, 3)
    with pytest.raises(ValueError, match="n_sample times"):
        E.check_shuffle_map([3] * 3 + [0] * 12, 5, 3)


# ---- the tree walk -----------------------------------------------------------------------------------------------------------------------
def _write_tree(root, n_speaker, n_sample, steps):
    """A Saver-shaped result tree (meta_tts_amd/saver.py) of short 16 kHz wavs + the raw corpus + test_SQids.json; mode `m1` one output
    per task, mode `m5` the five-fold layout test_###_0 .. 4."""
    from scipy.io import wavfile
    g = np.random.RandomState(0)
    raw, sq, k = os.path.join(root, "raw"), [], 0
    write = lambda path, seed: (os.makedirs(os.path.dirname(path), exist_ok=True),   # noqa: E731
                                wavfile.write(path, 16000, (O.chirps(int(g.randint(9000, 30000)), seed) * 20000).astype(np.int16)))
    for s in range(n_speaker):
        for u in range(5):
            write(os.path.join(raw, f"{100 + s}", f"{100 + s}_{u:02d}.wav"), 1000 * s + u)
        for q in range(n_sample):
            sq.append({"sup_id": [f"{100 + s}_04"], "qry_id": [f"{100 + s}_{q:02d}"]})
    dirs = {"recon": os.path.join(root, "result", "m1"), "m1": os.path.join(root, "result", "m1"), "m5": os.path.join(root, "result", "m5"),
            "real": raw, "enrollment": raw}
    for data_id, q in enumerate(sq):
        base = q["qry_id"][0]
        d = os.path.join(dirs["m1"], "audio", "Testing", f"test_{data_id:03d}")
        write(os.path.join(d, f"{base}.recon.wav"), 5000 + data_id)
        for st in steps:
            write(os.path.join(d, f"{base}.step_100000-FTstep_{st}.synth.wav"), 6000 + 10 * data_id + st)
            for i in range(5):
                write(os.path.join(dirs["m5"], "audio", "Testing", "step_100000", f"test_{data_id:03d}_{i}", f"{base}.step_100000-FTstep_{st}.synth.wav"), 7000 + k)
                k += 1
    json.dump(sq, open(os.path.join(dirs["recon"], "test_SQids.json"), "w"))
    return dirs


def _check_tree_walk(lib_path, dims, tmp_path):
    n_speaker, n_sample, steps = 5, 2, [0, 5]
    dirs = _write_tree(str(tmp_path), n_speaker, n_sample, steps)
    cfg = E.EvalConfig("Tiny", dirs, n_speaker, n_sample, [("m1", steps), ("m5", [5])], work_dir=str(tmp_path / "work"))
    emb = _embedder(lib_path, dims, max_partials=8)
    w = E.WavsToDvector(cfg, emb, rng=random.Random(3))
    n, e = n_speaker * n_sample, dims["emb"]
    npy = lambda name: np.load(os.path.join(str(tmp_path), "work", "npy", "Tiny", name), allow_pickle=True)   # noqa: E731
    assert npy("real_dvector.npy").shape == npy("recon_dvector.npy").shape == npy("m1_step5_dvector.npy").shape == (n, e)
    assert npy("m5_step5_dvector.npy").shape == (5 * n, e) and npy("pair_dvector.npy").shape == (2, 4 * n, e)
    assert npy("centroid_dvector.npy").shape == (n_speaker, e) and [len(x) for x in npy("enrollment_dvector.npy")] == [5] * n_speaker
    assert len(json.load(open(os.path.join(str(tmp_path), "work", "json", "Tiny", "pair.json")))) == n
    real0 = emb.embed_utterance(E.read_wav_16k(w.real_filelist[0]))
    assert np.array_equal(real0, w.dvector_list_dict["real"][0])                          # one wav alone = its row of the batched walk
    p = E.PairSimilarity(cfg, emb)
    p.load_dvector()
    p.get_pair_similarity()
    p.save_pair_similarity()
    assert p.pair_similarity_dict["m5_step5"].shape == (2, 20 * n) and p.pair_similarity_dict["real"].shape == (2, 4 * n)
    c = E.CentroidSimilarity(cfg, emb, rng=random.Random(4))
    c.load_dvector()
    c.get_centroid_similarity()
    assert c.similarity_list_dict["recon_random"].shape == (n,) and c.similarity_list_dict["m5_step5"].shape == (5 * n,)
    v = E.SpeakerVerification(cfg)
    v.load_pair_similarity()
    v.get_eer()
    v.get_auc()
    lines = open(v.output_path).read().split("\n")
    assert lines[0::2][:-1] == [m + ":" for m in ["recon", "real", "m1_step0", "m1_step5", "m5_step5"]]
    for ln, m in zip(lines[1::2], v.eer_dict):
        assert ln == f"threshold:{v.threshold_dict[m]:.4f}\tEER:{v.eer_dict[m]:.4f}" and 0 <= v.eer_dict[m] <= 1 and 0 <= v.auc_dict.get(m, 0.5) <= 1
    assert v.auc_dict["real"] == pytest.approx(0.5)
    emb.close()


def test_tree_walk_emulator(tmp_path):
    _check_tree_walk(_emu(), TINY, tmp_path)


@pytest.mark.gpu
def test_tree_walk_gpu(tmp_path):
    _check_tree_walk(None, FULL, tmp_path)


# ---- the preprocess hook ---------------------------------------------------------------------------------------------------------------------
def test_preprocess_writes_spk_ref_mel_slices(tmp_path):
    import test_preprocess as TP
    c = TP._Corpus("small", str(tmp_path), _emu())
    f0_fn = c.write_raw()
    emb = E.SpeakerEmbedder(lib_path=_emu(), encoder=False)
    with pytest.raises(MttsError, match="sampling rate"):      # the corpus' rate is not 16 kHz and nothing here resamples
        c.pp.speaker_reference_fn(emb)(*c.utts[0])
    to16k = lambda wav, rate: O.chirps(20000 + 7 * len(wav) % 9000, len(wav))   # noqa: E731  (a stand-in for a resampler)
    c.pp.build_from_path(f0_fn=f0_fn, batch_utterances=4, spk_ref_fn=c.pp.speaker_reference_fn(emb, resample=to16k))
    out = c.pp.out_dir
    names = sorted(os.listdir(os.path.join(out, "spk_ref_mel_slices")))
    assert names == sorted(os.listdir(os.path.join(out, "mel"))) and names
    ds = D.FeatureDataset(out, "train.txt", lambda t: [1] * len(t.strip("{}").split()), spk_refer_wav=True)
    samples = [ds[i] for i in range(len(ds))]
    for smp, base in zip(samples, c.kept):
        n16 = 20000 + 7 * len(TP.G[f"{c.name}|{base}|wav"]) % 9000
        want = (len(E.compute_partial_slices(n16)[1]), 160, 40)
        assert smp["spk_ref_mel_slices"].shape == want and smp["spk_ref_mel_slices"].dtype == np.float32
        assert np.array_equal(smp["spk_ref_mel_slices"], emb.reference_mel_slices(to16k(TP.G[f"{c.name}|{base}|wav"], 0)))
    ref_mels, ref_slices = D.reprocess(samples, list(range(len(samples))))[2]
    assert ref_mels.shape == (sum(len(s["spk_ref_mel_slices"]) for s in samples), 160, 40) and len(ref_slices) == len(samples)
    emb.close()
    c.pp.close()
