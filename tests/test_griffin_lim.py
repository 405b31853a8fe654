"""Spectrogram -> waveform (csrc/griffin.h through include/mtts.h: mtts_stft_load_inverse / _transform / _inverse / _griffin_lim /
_inv_mel) against tests/golden/griffin.npz — outputs of the reference's own STFT.transform / STFT.inverse / griffin_lim / inv_mel_spec
(tests/golden/make_griffin_golden.py) — and against tests/gl_oracle.py (CPU torch restatement, pinned to the same fixture) for batches
the fixture does not cover.  Small transforms through the SIMT emulator; the LibriTTS configuration (1024 / 256 / 1024, 80 mels,
22050 Hz) on the MI355X."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import gl_oracle as GO
from meta_tts_amd.audio import audio_processing as AP
from meta_tts_amd.audio import stft as S
from meta_tts_amd.audio import tools
from meta_tts_amd.audio.griffin import GriffinLim
from meta_tts_amd.engine import MttsError

HERE = os.path.dirname(os.path.abspath(__file__))
SMALL = ("small", "short_window")
ALL = SMALL + ("libritts",)


def _golden():
    return np.load(os.path.join(HERE, "golden", "griffin.npz"))


def _cfg(g, tag):
    n_fft, hop, win, n_mel, sr, n, seed = (int(x) for x in g[tag + "_cfg"])
    return n_fft, hop, win, n_mel, sr, n, seed


def _stft(g, tag, lib_path):
    n_fft, hop, win, n_mel, sr, n, _ = _cfg(g, tag)
    st = S.TacotronSTFT(n_fft, hop, win, n_mel, sr, 0, None, max_samples=n + 64, lib_path=lib_path)
    np.testing.assert_array_equal(st.mel_basis, g[tag + "_mel_basis"])
    return st


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


def _check_transform(g, tag, fn):
    mag, ph = fn.transform(g[tag + "_wav"])
    rm, rp = g[tag + "_magnitude"], g[tag + "_phase"]
    assert mag.shape == (1,) + rm.shape and mag.dtype == np.float32
    np.testing.assert_allclose(mag[0], rm, rtol=0, atol=2e-5 * rm.max())
    live = rm > 1e-3 * rm.max()
    d = np.angle(np.exp(1j * (ph[0][live].astype(np.float64) - rp[live])))     # phase difference, wrapped to (-pi, pi]
    assert np.abs(d).max() < 1e-3, np.abs(d).max()
    # no clip: the signal leaves [-1, 1], and its clipped version has a visibly different spectrum
    assert np.abs(g[tag + "_wav"]).max() > 1.2
    cm, _ = fn.transform(np.clip(g[tag + "_wav"], -1, 1))
    assert np.abs(cm[0] - rm).max() > 1e-2 * rm.max()


def _check_inverse(g, tag, fn):
    y = fn.inverse(g[tag + "_magnitude"][None], g[tag + "_phase"][None])
    r = g[tag + "_inverse"]
    assert y.shape == (1, 1, len(r)) and y.dtype == np.float32
    assert np.abs(y[0, 0] - r).max() <= 1e-5 * np.abs(r).max()


def _check_griffin_lim(g, tag, fn, iters):
    seed = _cfg(g, tag)[6]
    for k in iters:
        np.random.seed(seed + k)
        y = AP.griffin_lim(g[tag + "_magnitude"][None], fn, k)
        r = g[f"{tag}_gl{k}"]
        assert y.shape == (1, len(r))
        assert _rel(y[0], r) <= 1e-5, (k, _rel(y[0], r))


def _check_inv_mel(g, tag, st, tmp_path, rel_gate, abs_gate):
    from scipy.io import wavfile
    n_fft, hop, win, n_mel, sr, n, seed = _cfg(g, tag)
    mel = g[tag + "_mel"]
    np.random.seed(seed + 1000)
    p = str(tmp_path / f"{tag}.wav")
    assert tools.inv_mel_spec(torch.from_numpy(mel), p, st, 60) is None
    rate, w = wavfile.read(p)
    r = g[tag + "_inv_mel_wav"]
    assert rate == sr and w.dtype == np.float32 and len(w) == hop * (mel.shape[1] - 2) == len(r)
    assert _rel(w, r) <= rel_gate and np.abs(w - r).max() <= abs_gate, (_rel(w, r), np.abs(w - r).max())


# ---- host-side restatements --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ALL)
def test_inverse_basis_and_window_envelope_match_fixture(tag):
    g = _golden()
    n_fft, hop, win = _cfg(g, tag)[:3]
    e = int(g["env_frames"][0])
    env = AP.window_sumsquare("hann", e, hop_length=hop, win_length=win, n_fft=n_fft, dtype=np.float32)
    assert env.dtype == np.float32 and env.shape == (n_fft + hop * (e - 1),)
    np.testing.assert_allclose(env, g[tag + "_window_sum"], rtol=1e-6, atol=0)
    if tag + "_inverse_basis" in g:
        ib = S.inverse_basis(n_fft, hop, win)
        assert ib.shape == (2 * (n_fft // 2 + 1), n_fft) and ib.dtype == np.float32
        np.testing.assert_allclose(ib, g[tag + "_inverse_basis"], rtol=1e-6, atol=1e-9)


def test_spectral_normalize_round_trip():
    x = np.abs(np.random.RandomState(0).standard_normal((3, 7))).astype(np.float32)
    x[0, 0] = 0.0
    c = AP.dynamic_range_compression(x)
    assert c.dtype == np.float32 and c[0, 0] == np.float32(np.log(np.float32(1e-5)))
    np.testing.assert_allclose(AP.dynamic_range_decompression(c)[1:], x[1:], rtol=1e-6)


@pytest.mark.parametrize("tag", ALL)
def test_torch_restatement_matches_fixture(tag):
    """Pins tests/gl_oracle.py to the reference's own outputs (every quantity of the fixture, 60 iterations included)."""
    g = _golden()
    n_fft, hop, win, n_mel, sr, n, seed = _cfg(g, tag)
    o = GO.Stft(n_fft, hop, win)
    m, p = o.transform(g[tag + "_wav"][None])
    np.testing.assert_allclose(m[0].numpy(), g[tag + "_magnitude"], rtol=0, atol=1e-6 * g[tag + "_magnitude"].max())
    y = o.inverse(torch.from_numpy(g[tag + "_magnitude"])[None], torch.from_numpy(g[tag + "_phase"])[None])
    assert np.abs(y[0].numpy() - g[tag + "_inverse"]).max() <= 1e-6 * np.abs(g[tag + "_inverse"]).max()
    for k in (int(x) for x in g["iters"]):
        np.random.seed(seed + k)
        a = AP.random_angles((1,) + g[tag + "_magnitude"].shape)
        y = o.griffin_lim(g[tag + "_magnitude"][None], a, k)
        assert _rel(y[0].numpy(), g[f"{tag}_gl{k}"]) <= (1e-6 if k <= 5 else 1e-4)
    np.random.seed(seed + 1000)
    a = AP.random_angles((1, n_fft // 2 + 1, g[tag + "_mel"].shape[1] - 1))[0]
    w = GO.inv_mel(o, g[tag + "_mel"], g[tag + "_mel_basis"], a, 60).numpy()
    assert _rel(w, g[tag + "_inv_mel_wav"]) <= 1e-4


# ---- the device code through the SIMT emulator ---------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", SMALL)
def test_emulator_transform_inverse_griffin_lim_vs_fixture(tag):
    g = _golden()
    st = _stft(g, tag, ge.build_emulator())
    _check_transform(g, tag, st.stft_fn)
    _check_inverse(g, tag, st.stft_fn)
    _check_griffin_lim(g, tag, st.stft_fn, (0, 1, 5))
    st.close()


@pytest.mark.parametrize("tag", SMALL)
def test_emulator_inv_mel_spec_writes_the_reference_wav(tag, tmp_path):
    g = _golden()
    st = _stft(g, tag, ge.build_emulator())
    assert st._stft_fn is st.stft_fn
    _check_inv_mel(g, tag, st, tmp_path, 1e-3, 1e-3)
    st.close()


def test_stand_alone_stft_forward_round_trip():
    """STFT(...) owns its handle; forward = inverse(transform(x)) reconstructs the interior of the signal (Hann at hop = n_fft / 4
    satisfies the overlap-add condition)."""
    st = S.STFT(64, 16, 64, lib_path=ge.build_emulator())
    x = np.random.RandomState(3).standard_normal((2, 400)).astype(np.float32) * 1.5
    y = st.forward(torch.from_numpy(x))
    assert y.shape == (2, 1, 16 * (400 // 16)) and isinstance(y, np.ndarray)
    np.testing.assert_allclose(y[:, 0, :384], x[:, :384], rtol=0, atol=2e-5)
    st.close()


def test_batch_of_three_equals_three_single_calls():
    lib = ge.build_emulator()
    st = S.TacotronSTFT(64, 16, 64, 12, 8000, 0, None, max_samples=600, lib_path=lib)
    rs = np.random.RandomState(5)
    frames = [9, 23, 14]
    mels = np.full((3, 12, 25), -11.5, np.float32)
    for b, f in enumerate(frames):
        mels[b, :, :f] = rs.uniform(-6, 0, (12, f))
    voc = GriffinLim(st, n_iters=5)
    np.random.seed(77)
    batched = voc.mel2wav(mels, frames)
    np.random.seed(77)
    singles = [voc.mel2wav(mels[b:b + 1], [f])[0] for b, f in enumerate(frames)]
    o = GO.Stft(64, 16, 64)
    np.random.seed(77)
    for b, f in enumerate(frames):
        assert len(batched[b]) == 16 * (f - 2) == len(singles[b])
        np.testing.assert_allclose(batched[b], singles[b], rtol=0, atol=1e-6 * np.abs(singles[b]).max())
        a = AP.random_angles((1, 33, f - 1))[0]
        ref = GO.inv_mel(o, mels[b, :, :f], st.mel_basis, a, 5).numpy()
        assert _rel(batched[b], ref) <= 1e-5
    st.close()


def test_named_errors_before_any_launch():
    lib_path = ge.build_emulator()
    st = S.TacotronSTFT(64, 16, 64, 12, 8000, 0, None, max_samples=600, lib_path=lib_path)
    mel = np.full((12, 3), -3.0, np.float32)   # 2 frames after the drop: 16 samples, not more than n_fft / 2 = 32
    with pytest.raises(MttsError, match="too short"):
        tools.inv_mel_spec(mel, "/nonexistent/never_written.wav", st, 60)
    with pytest.raises(MttsError, match="n_iters < 0"):
        st.inv_mel_with_angles([np.zeros((12, 10), np.float32)], [np.zeros((33, 9), np.float32)], -1)
    with pytest.raises(MttsError, match="too short"):
        st.stft_fn.transform(np.zeros(32, np.float32))
    # the C ABI itself: no inverse basis loaded, a negative iteration count, a too-short spectrogram -> error, output untouched
    lib = st.lib
    h = C.c_void_p()
    assert lib.mtts_stft_create(64, 16, 12, 600, 0, C.byref(h)) == 0
    fb = S.forward_basis(64, 64)
    assert lib.mtts_stft_load(h, fb.ctypes.data_as(C.c_void_p), st.mel_basis.ctypes.data_as(C.c_void_p)) == 0
    T = np.asarray([10], np.int32)
    mag = np.ones((10, 33), np.float32)
    out = np.full(16 * 9, 7.0, np.float32)
    args = lambda n_it: (h, 1, T.ctypes.data_as(C.c_void_p), mag.ctypes.data_as(C.c_void_p), mag.ctypes.data_as(C.c_void_p), n_it,
                         out.ctypes.data_as(C.c_void_p))
    assert lib.mtts_stft_griffin_lim(*args(1)) < 0
    assert b"inverse basis not loaded" in lib.mtts_stft_last_error(h)
    ib = S.inverse_basis(64, 16, 64)
    wsq = (AP._window("hann", 64, 64) ** 2).astype(np.float32)
    assert lib.mtts_stft_load_inverse(h, ib.ctypes.data_as(C.c_void_p), wsq.ctypes.data_as(C.c_void_p)) == 0
    assert lib.mtts_stft_griffin_lim(*args(-1)) < 0
    assert b"n_iters < 0" in lib.mtts_stft_last_error(h)
    T[0] = 3
    assert lib.mtts_stft_griffin_lim(*args(1)) < 0
    assert b"too short" in lib.mtts_stft_last_error(h)
    assert (out == 7.0).all()
    T[0] = 10
    assert lib.mtts_stft_griffin_lim(*args(1)) == 16 * 9 and np.isfinite(out).all() and not (out == 7.0).all()
    lib.mtts_stft_destroy(h)
    st.close()


def test_griffin_lim_vocoder_feeds_the_unmodified_saver(tmp_path):
    """GriffinLim.infer has MelGAN.infer's duck type: the Saver writes `<id>.recon.wav` and `<id>.<step>.synth.wav` from it."""
    from scipy.io import wavfile
    from meta_tts_amd.saver import CSV_COLUMNS, Saver
    st = S.TacotronSTFT(1024, 256, 1024, 80, 22050, 0, 8000, max_samples=22050, lib_path=ge.build_emulator())
    voc = GriffinLim(st, n_iters=1)
    rs = np.random.RandomState(11)
    B, T = 2, 12
    mel_lens = np.asarray([12, 7], np.int64)
    gt = rs.uniform(-8, -1, (B, T, 80)).astype(np.float32)
    post = rs.uniform(-8, -1, (B, T, 80)).astype(np.float32)
    ids = ["spk_a", "spk_b"]
    targets = (ids, None, None, None, None, None, gt, mel_lens)
    preds = [None, post] + [None] * 7 + [mel_lens]
    outputs = [{"_batch": targets, "step_0": {"recon": {"output": preds, "losses": [0.1] * len(CSV_COLUMNS)}, "synth": {"output": preds}}}]
    batch = [([(["s0"],)], [(["q0"],)])]
    pre = {"preprocessing": {"stft": {"hop_length": 256}, "audio": {"sampling_rate": 22050, "max_wav_value": 32768.0}}}
    sv = Saver(pre, str(tmp_path / "log"), str(tmp_path / "result"))
    sv.on_test_batch_end(outputs, batch, {"s0.q0": "task_1"}, 5, 1, 0, voc)
    adir = tmp_path / "result" / "audio" / "Testing" / "step_5" / "task_1"
    assert sorted(os.listdir(adir)) == sorted([f"{i}.recon.wav" for i in ids] + [f"{i}.step_5-FTstep_0.synth.wav" for i in ids])
    for i, L in zip(ids, mel_lens):
        for name in (f"{i}.recon.wav", f"{i}.step_5-FTstep_0.synth.wav"):
            rate, w = wavfile.read(adir / name)
            assert rate == 22050 and w.dtype == np.int16 and len(w) == 256 * (int(L) - 2)
            assert np.abs(w).max() > 0
    st.close()


# ---- the MI355X, LibriTTS configuration ----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_libritts_vs_reference_fixture(tmp_path):
    ge.build_device()
    g = _golden()
    st = _stft(g, "libritts", None)
    _check_transform(g, "libritts", st.stft_fn)
    _check_inverse(g, "libritts", st.stft_fn)
    _check_griffin_lim(g, "libritts", st.stft_fn, (0, 1, 5))
    _check_inv_mel(g, "libritts", st, tmp_path, 1e-3, 1e-3)
    np.random.seed(int(g["libritts_cfg"][6]) + 60)
    y = AP.griffin_lim(g["libritts_magnitude"][None], st.stft_fn, 60)
    assert _rel(y[0], g["libritts_gl60"]) <= 1e-3 and np.abs(y[0] - g["libritts_gl60"]).max() <= 1e-3
    st.close()


@pytest.mark.gpu
def test_gpu_batch_of_eight_vs_torch_restatement():
    """8 utterances of 1-6 s in one call, 60 iterations, each against the CPU restatement from the same starting phases."""
    ge.build_device()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    sr, hop = 22050, 256
    st = S.TacotronSTFT(1024, hop, 1024, 80, sr, 0, 8000, max_samples=sr * 7, lib_path=None)
    rs = np.random.RandomState(21)
    secs = [1.0, 6.0, 2.3, 4.1, 1.6, 5.2, 3.0, 2.7]
    mels = []
    for s in secs:
        n = int(s * sr)
        t = np.arange(n) / sr
        f0 = rs.uniform(100, 300)
        w = (0.5 * np.sin(2 * np.pi * f0 * t + 3 * np.sin(2 * np.pi * 0.7 * t)) * np.hanning(n) + 0.02 * rs.standard_normal(n))
        mels.append(tools.get_mel_from_wav(w.astype(np.float32), st)[0])
    Tmax = max(m.shape[1] for m in mels)
    batch = np.full((8, 80, Tmax), np.log(1e-5), np.float32)
    for b, m in enumerate(mels):
        batch[b, :, :m.shape[1]] = m
    np.random.seed(99)
    got = GriffinLim(st, n_iters=60).mel2wav(batch, [m.shape[1] for m in mels])
    o = GO.Stft(1024, hop, 1024)
    np.random.seed(99)
    for b, m in enumerate(mels):
        a = AP.random_angles((1, 513, m.shape[1] - 1))[0]
        ref = GO.inv_mel(o, m, st.mel_basis, a, 60).numpy()
        assert len(got[b]) == len(ref) == hop * (m.shape[1] - 2)
        assert _rel(got[b], ref) <= 1e-3 and np.abs(got[b] - ref).max() <= 1e-3, (b, _rel(got[b], ref), np.abs(got[b] - ref).max())
    st.close()
