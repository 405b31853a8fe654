#!/usr/bin/env python3
"""Generates tests/golden/griffin.npz by running the REFERENCE's own inverse STFT path (/root/reference/audio/stft.py: STFT.transform,
STFT.inverse; audio/audio_processing.py: window_sumsquare, griffin_lim; audio/tools.py: inv_mel_spec) in the build container.
Shims, as in make_stft_golden.py (the container has neither librosa nor a GPU):
  * librosa.util.pad_center / tiny / normalize: one-liners restated below;
  * librosa.filters.mel: meta_tts_amd.audio.stft.mel_filterbank (stored as an INPUT of the fixture);
  * torch.Tensor.cuda: identity (STFT.transform hard-codes .cuda());
  * `_stft._stft_fn`: inv_mel_spec reads this attribute, which the reference's TacotronSTFT does not define (it defines `stft_fn`) —
    as written the reference function raises AttributeError; the script aliases it to `stft_fn`.
The reference never travels: only this script and the arrays it writes are committed."""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference")

from meta_tts_amd.audio import stft as ours  # noqa: E402  (mel basis shim only)


def pad_center(data, size, axis=-1, **kw):
    n = data.shape[axis]
    lpad = int((size - n) // 2)
    lengths = [(0, 0)] * data.ndim
    lengths[axis] = (lpad, int(size - n - lpad))
    return np.pad(data, lengths, **kw)


def tiny(x):
    return np.finfo(np.asarray(x).dtype if np.issubdtype(np.asarray(x).dtype, np.floating) else np.float32).tiny


def normalize(S, norm=np.inf, **kw):
    return S if norm is None else S / np.max(np.abs(S))


librosa = types.ModuleType("librosa")
librosa.util = types.ModuleType("librosa.util")
librosa.util.pad_center, librosa.util.tiny, librosa.util.normalize = pad_center, tiny, normalize
librosa.filters = types.ModuleType("librosa.filters")
librosa.filters.mel = lambda sr, n_fft, n_mels, fmin, fmax: ours.mel_filterbank(sr, n_fft, n_mels, fmin, fmax)
sys.modules.update({"librosa": librosa, "librosa.util": librosa.util, "librosa.filters": librosa.filters})
torch.Tensor.cuda = lambda self, *a, **k: self

from audio.audio_processing import griffin_lim, window_sumsquare  # noqa: E402  (the reference)
from audio.stft import TacotronSTFT  # noqa: E402
from audio.tools import get_mel_from_wav, inv_mel_spec  # noqa: E402
from scipy.io import wavfile  # noqa: E402


def wave(n, sr, seed):   # tests/test_griffin_lim.py: _wave — exceeds [-1, 1] (transform must not clip)
    g = np.random.RandomState(seed)
    t = np.arange(n) / sr
    w = 0.9 * np.sin(2 * np.pi * 220 * t) + 0.6 * np.sin(2 * np.pi * 1870 * t + 1.0) + 0.05 * g.standard_normal(n)
    w[n // 3] = 1.7
    return w.astype(np.float32)


ITERS = (0, 1, 5, 60)
ENV_FRAMES = 8
out = {}
for tag, (n_fft, hop, win, n_mel, sr, n) in {"small": (64, 16, 64, 12, 8000, 500), "short_window": (64, 16, 48, 12, 8000, 333),
                                             "libritts": (1024, 256, 1024, 80, 22050, 7600)}.items():
    st = TacotronSTFT(n_fft, hop, win, n_mel, sr, 0, None)
    st._stft_fn = st.stft_fn
    fn = st.stft_fn
    seed = 1234 + n
    wav = wave(n, sr, seed)
    with torch.no_grad():
        mag, phase = fn.transform(torch.from_numpy(wav)[None])
        inv = fn.inverse(mag, phase)
        out[tag + "_cfg"] = np.asarray([n_fft, hop, win, n_mel, sr, n, seed], np.int64)
        out[tag + "_wav"] = wav
        out[tag + "_mel_basis"] = st.mel_basis.numpy()
        out[tag + "_window_sum"] = window_sumsquare("hann", ENV_FRAMES, hop_length=hop, win_length=win, n_fft=n_fft, dtype=np.float32)
        if tag != "libritts":   # (4 MB at the LibriTTS size: that one is pinned by the CPU restatement instead)
            out[tag + "_inverse_basis"] = fn.inverse_basis.numpy()[:, 0, :]
        out[tag + "_magnitude"] = mag[0].numpy()
        out[tag + "_phase"] = phase[0].numpy()
        out[tag + "_inverse"] = inv[0, 0].numpy()
        for k in ITERS:
            np.random.seed(seed + k)
            out[f"{tag}_gl{k}"] = griffin_lim(mag, fn, k)[0].numpy()
        mel, _ = get_mel_from_wav(wav, st)
        np.random.seed(seed + 1000)
        with tempfile.TemporaryDirectory() as d:
            p = os.path.join(d, "inv.wav")
            inv_mel_spec(torch.from_numpy(mel), p, st, 60)
            rate, w = wavfile.read(p)
        assert rate == sr and w.dtype == np.float32 and len(w) == hop * (mel.shape[1] - 2)
        out[tag + "_mel"] = mel
        out[tag + "_inv_mel_wav"] = w
out["iters"] = np.asarray(ITERS, np.int64)
out["env_frames"] = np.asarray([ENV_FRAMES], np.int64)
path = os.path.join(HERE, "griffin.npz")
np.savez_compressed(path, **out)
print({k: v.shape for k, v in out.items()}, os.path.getsize(path))
