"""Silence trimming of waveform batches on libmtts.so (csrc/vad.h through include/mtts.h: mtts_stft_load_vad / mtts_stft_trim_batch; the
chained mtts_dvector_embed_wavs_preprocessed is reached through `meta_tts_amd.evaluation.SpeakerEmbedder.embed_utterances(..., trim=True)`).

The third step of resemblyzer's `preprocess_wav`: `trim_long_silences` asks webrtcvad whether each 30 ms window is voiced, smooths the
flags with a moving average of width 8 rounded to bool, dilates them by 7 windows and keeps the samples of the windows that remain.
webrtcvad's GMM decision is third party, is not part of this project and is NOT restated: PARITY with it is UNPINNED.  In its place
stands an energy detector defined in include/mtts.h,

    W = window_ms * sampling_rate / 1000,  n_w = len(wav) // W,  e[w] = mean(wav[w W : (w + 1) W] ** 2)   (float64),
    noise = sorted(e)[floor(noise_quantile * (n_w - 1))],  raw[w] = e[w] >= max(10 ** (floor_db / 10), noise * 10 ** (margin_db / 10)),

whose three constants (floor_db -50, noise_quantile 0.1, margin_db 10) are this project's choice and have not been tuned against
webrtcvad.  Everything resemblyzer does around the decision is restated exactly (`trim_long_silences` below is the host form), and a
caller who owns webrtcvad passes its decisions as `flags`: then only that post-processing runs on the device.  An utterance whose mask
keeps no window (shorter than a window, digital silence) is returned as it is, where resemblyzer would return an empty array."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np

from ..engine import MttsError
from .stft import _Handle, _StageOnHandle, _pack_wavs

SAMPLING_RATE = 16000            # resemblyzer hparams: sampling_rate
VAD_WINDOW_LENGTH = 30           # ms
VAD_MOVING_AVERAGE_WIDTH = 8
VAD_MAX_SILENCE_LENGTH = 6
FLOOR_DB, NOISE_QUANTILE, MARGIN_DB = -50.0, 0.1, 10.0   # this project's detector; untuned


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def moving_average(array, width: int) -> np.ndarray:
    """resemblyzer's helper as written: zero padding of (width - 1) // 2 and width // 2, a cumulative sum, the mean of every `width` entries."""
    padded = np.concatenate((np.zeros((width - 1) // 2), np.asarray(array, np.float64), np.zeros(width // 2)))
    ret = np.cumsum(padded, dtype=float)
    ret[width:] = ret[width:] - ret[:-width]
    return ret[width - 1:] / width


def smooth_and_dilate(flags, ma_width: int = VAD_MOVING_AVERAGE_WIDTH, max_silence: int = VAD_MAX_SILENCE_LENGTH) -> np.ndarray:
    """Per-window flags -> the mask of kept windows: np.round(moving_average(flags, ma_width)).astype(bool), then
    scipy.ndimage.binary_dilation(., np.ones(max_silence + 1)) written out (scipy is not imported)."""
    flags = np.asarray(flags).astype(bool)
    if len(flags) == 0:
        return flags
    smooth = np.round(moving_average(flags, ma_width)).astype(bool)
    left, right = max_silence // 2, (max_silence + 1) // 2       # mask[w] = any smooth[w - left .. w + right]
    mask = np.zeros(len(smooth), bool)
    for k in range(-left, right + 1):
        mask |= _shift(smooth, k)
    return mask


def _shift(a: np.ndarray, k: int) -> np.ndarray:
    """b[w] = a[w + k], False outside."""
    b = np.zeros(len(a), bool)
    if abs(k) >= len(a):
        return b
    if k >= 0:
        b[:len(a) - k] = a[k:]
    else:
        b[-k:] = a[:len(a) + k]
    return b


def trim_long_silences(wav, flags, window: int = VAD_WINDOW_LENGTH * SAMPLING_RATE // 1000, ma_width: int = VAD_MOVING_AVERAGE_WIDTH,
                       max_silence: int = VAD_MAX_SILENCE_LENGTH) -> np.ndarray:
    """resemblyzer's `trim_long_silences` after the webrtcvad loop, on the host: `flags` holds one voiced / unvoiced decision per window
    of `window` samples (len(wav) // window of them; the tail is dropped).  Returns the samples of the kept windows — or, when no window
    is kept, `wav` as it is (the device entries' rule)."""
    wav = np.asarray(wav)
    n_w = len(wav) // window
    flags = np.asarray(flags)
    if len(flags) != n_w:
        raise ValueError(f"trim_long_silences: {len(flags)} flags for {n_w} windows of {window} samples")
    mask = smooth_and_dilate(flags, ma_width, max_silence)
    if not mask.any():
        return wav
    return wav[: n_w * window][np.repeat(mask, window)]


class SilenceTrimmer(_StageOnHandle):
    """Batched silence trimming on the device.  A stand-alone SilenceTrimmer owns a small mtts_stft handle; `_handle=` attaches it to an
    existing one (a SpeakerEmbedder's), which then also serves the chained entry.  A handle holds ONE configuration: `load()` makes this
    trimmer's the current one (done by the constructor and, when several share a handle, again before each use)."""
    _slot = "_vad_key"

    def __init__(self, sampling_rate: int = SAMPLING_RATE, window_ms: int = VAD_WINDOW_LENGTH, ma_width: int = VAD_MOVING_AVERAGE_WIDTH,
                 max_silence: int = VAD_MAX_SILENCE_LENGTH, floor_db: float = FLOOR_DB, noise_quantile: float = NOISE_QUANTILE, margin_db: float = MARGIN_DB,
                 device: int = 0, lib_path=None, *, max_samples: int = SAMPLING_RATE * 120, _handle: Optional[_Handle] = None):
        self.sampling_rate, self.window_ms, self.ma_width, self.max_silence = int(sampling_rate), int(window_ms), int(ma_width), int(max_silence)
        self.floor_db, self.noise_quantile, self.margin_db = float(floor_db), float(noise_quantile), float(margin_db)
        self.window = self.window_ms * self.sampling_rate // 1000
        self._key = (self.sampling_rate, self.window_ms, self.ma_width, self.max_silence, self.floor_db, self.noise_quantile, self.margin_db)
        self._attach(_handle, 16, 4, 1, max_samples, device, lib_path)
        self._first_load()

    def _load(self):
        self._check(self.lib.mtts_stft_load_vad(self.h, self.sampling_rate, self.window_ms, self.ma_width, self.max_silence, self.floor_db, self.noise_quantile,
                                                self.margin_db))

    def trim_batch(self, wavs: Sequence, flags: Optional[Sequence] = None, return_masks: bool = False):
        """A list of waveforms -> the list of trimmed float32 waveforms, one device call.  flags: per utterance, one decision per window
        (len(wav) // window of them) in place of the energy detector's.  return_masks: also (masks, n_voiced, energies): the bool mask of
        kept windows and the float64 window energies per utterance (energies None with flags), n_voiced int32 — 0 where the utterance
        was passed through as it is."""
        ws, n, packed = _pack_wavs(wavs)
        self.ensure_loaded()
        n_w = n // max(self.window, 1)
        fl = None
        if flags is not None:
            fs = [np.ascontiguousarray(np.asarray(f).astype(bool).astype(np.uint8).reshape(-1)) for f in flags]
            if len(fs) != len(ws) or any(len(f) != k for f, k in zip(fs, n_w)):
                raise MttsError(f"trim_batch: flags must hold len(wav) // {self.window} decisions per utterance")
            fl = np.ascontiguousarray(np.concatenate(fs + [np.zeros(1, np.uint8)]))
        out, n_out, n_voiced = np.empty(len(packed), np.float32), np.zeros(len(ws), np.int32), np.zeros(len(ws), np.int32)
        mask, energy = np.zeros(int(n_w.sum()) + 1, np.uint8), np.zeros(int(n_w.sum()) + 1, np.float64)
        total = self._check(self.lib.mtts_stft_trim_batch(self.h, len(ws), _ptr(n), _ptr(packed), _ptr(fl) if fl is not None else None, _ptr(out), _ptr(n_out),
                                                          _ptr(n_voiced), _ptr(mask), _ptr(energy)))
        assert total == int(n_out.sum())
        res = np.split(out[:total].copy(), np.cumsum(n_out)[:-1])
        if not return_masks:
            return res
        cuts = np.cumsum(n_w)[:-1]
        masks = np.split(mask[:-1].astype(bool), cuts)
        energies = np.split(energy[:-1], cuts) if fl is None else None
        return res, (masks, n_voiced, energies)

    def __call__(self, wav) -> np.ndarray:
        """The `trim_fn(wav) -> wav` callable `audio.resample.preprocess_wav(trim_fn=)` takes."""
        return self.trim_batch([wav])[0]


def trim_batch(wavs: Sequence, device: int = 0, lib_path=None, **config) -> List[np.ndarray]:
    """One-off form of `SilenceTrimmer(**config).trim_batch(wavs)`."""
    t = SilenceTrimmer(device=device, lib_path=lib_path, **config)
    try:
        return t.trim_batch(wavs)
    finally:
        t.close()
