"""MOSNet host layer: what stands behind `NeuralMOS.compute_mosnet` of the reference's evaluation/compute_mos.py
(`speechmetrics.load('mosnet')(path)['mosnet']`, one wav file at a time on the CPU).

Neither speechmetrics, its TensorFlow model code nor the published `cnn_blstm.h5` is part of the reference tree, so parity with the
published weights is UNPINNED, and with them the analysis window (a symmetric Hamming window: the default of `forward_basis`) and the
recurrent activation (sigmoid, tf.keras 2's default).  What is pinned is the definition in include/mtts.h (mtts_mosnet_*): the published
CNN-BLSTM MOSNet (Lo et al. 2019) in inference mode, restated in torch by tests/mosnet_oracle.py.  This class takes a state dict in
torch layouts (`tensor_spec`), Keras' `get_weights()` list (`from_keras_weights`; a user who has the published .h5 and h5py elsewhere
converts with it) or synthetic weights, and packs the images `libmtts.so` reads (csrc/mosnet.h).
"""
from __future__ import annotations

import ctypes as C
import math
import zlib

import numpy as np

from . import _lib
from .engine import MttsError

CHANNELS = (16, 32, 64, 128)
HIDDEN = 128
SAMPLING_RATE = 16000
HOP = 256
KERAS_ORDER = ([f"conv.{l}.{p}" for l in range(12) for p in ("weight", "bias")] +
               ["blstm.weight_ih", "blstm.weight_hh", "blstm.bias", "blstm.weight_ih_reverse", "blstm.weight_hh_reverse", "blstm.bias_reverse",
                "dense.weight", "dense.bias", "frame_score.weight", "frame_score.bias"])


def same_pad(f_in: int, stride: int):
    """TensorFlow "same" padding of a 3-wide kernel along frequency: (F_out, left, right)."""
    f_out = -(-int(f_in) // stride)
    total = max((f_out - 1) * stride + 3 - int(f_in), 0)
    return f_out, total // 2, total - total // 2


def widths(n_freq: int):
    """The widths in front of the four blocks and behind the last: 257 -> [257, 86, 29, 10, 4]."""
    out = [int(n_freq)]
    for _ in CHANNELS:
        out.append(same_pad(out[-1], 3)[0])
    return out


def tensor_spec(n_freq: int = 257):
    """[(name, torch-layout shape)] in module order."""
    spec, cin = [], 1
    for b, c in enumerate(CHANNELS):
        for j in range(3):
            spec += [(f"conv.{3 * b + j}.weight", (c, cin, 3, 3)), (f"conv.{3 * b + j}.bias", (c,))]
            cin = c
    n_in = CHANNELS[-1] * widths(n_freq)[-1]
    for sfx in ("", "_reverse"):
        spec += [("blstm.weight_ih" + sfx, (4 * HIDDEN, n_in)), ("blstm.weight_hh" + sfx, (4 * HIDDEN, HIDDEN)), ("blstm.bias" + sfx, (4 * HIDDEN,))]
    spec += [("dense.weight", (HIDDEN, 2 * HIDDEN)), ("dense.bias", (HIDDEN,)), ("frame_score.weight", (1, HIDDEN)), ("frame_score.bias", (1,))]
    return spec


def synthetic_state_dict(seed: int = 0, n_freq: int = 257):
    """Deterministic weights that keep every stage alive on magnitudes of order 1: convolutions at He's gain (a ReLU halves the second
    moment, sqrt(2 / fan_in) restores it) with biases of 0.05; the LSTM input projection at 1 / sqrt(fan_in) and the recurrent one at
    half of that, so gate pre-activations are of order 1 and stay out of saturation; the dense layers wide enough that frame scores
    move with the input; the score bias at 3, mid-scale of a MOS."""
    sd = {}
    for name, shape in tensor_spec(n_freq):
        g = np.random.RandomState((zlib.crc32(name.encode()) ^ seed) & 0x7FFFFFFF)
        v = g.standard_normal(shape)
        if name.endswith("bias") or name.endswith("bias_reverse"):
            v = 0.05 * v + (3.0 if name == "frame_score.bias" else 0.0)
        elif name.startswith("conv."):
            v *= math.sqrt(2.0 / (9 * shape[1]))
        elif "weight_ih" in name:
            v *= 1.0 / math.sqrt(shape[1])
        elif "weight_hh" in name:
            v *= 0.5 / math.sqrt(shape[1])
        elif name == "dense.weight":
            v *= 3.0 / math.sqrt(shape[1])
        else:
            v *= 2.0 / math.sqrt(shape[1])
        sd[name] = v.astype(np.float32)
    return sd


def _np(sd):
    return {k: np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, np.float32) for k, v in sd.items()}


def check_state_dict(sd, n_freq: int = 257):
    sd = _np(sd)
    for name, shape in tensor_spec(n_freq):
        if name not in sd:
            raise MttsError(f"MOSNet: tensor {name} is missing")
        if tuple(sd[name].shape) != tuple(shape):
            raise MttsError(f"MOSNet: {name} has shape {tuple(sd[name].shape)}, n_freq = {n_freq} asks for {tuple(shape)}")
    return sd


def pack_tensors(sd, n_freq: int = 257):
    """torch-layout state dict -> {libmtts tensor name: float32 array} (layouts documented in include/mtts.h)."""
    sd = check_state_dict(sd, n_freq)
    out = {}
    for l in range(12):
        w = sd[f"conv.{l}.weight"]
        cout, cin = w.shape[:2]
        k = w.transpose(2, 3, 1, 0).reshape(9, cin, cout)                                    # [tap][cin][cout]
        out[f"conv.{l}.w"] = k.reshape(9, cout) if cin == 1 else k.reshape(9, cin // 8, 8, cout).transpose(0, 1, 3, 2)
        out[f"conv.{l}.b"] = sd[f"conv.{l}.bias"]
    out["blstm.w_ih"] = np.concatenate([sd["blstm.weight_ih"], sd["blstm.weight_ih_reverse"]])
    out["blstm.b"] = np.concatenate([sd["blstm.bias"], sd["blstm.bias_reverse"]])
    out["blstm.w_hh"] = np.stack([sd["blstm.weight_hh" + s].reshape(4 * HIDDEN, HIDDEN // 4, 4).transpose(1, 0, 2) for s in ("", "_reverse")])
    out["dense.w"], out["dense.b"] = sd["dense.weight"], sd["dense.bias"]
    out["frame_score.w"], out["frame_score.b"] = sd["frame_score.weight"].reshape(-1), sd["frame_score.bias"]
    return {k: np.ascontiguousarray(v, np.float32) for k, v in out.items()}


def from_keras_weights(weights, n_freq: int = 257):
    """Keras' `model.get_weights()` of the published CNN-BLSTM (conv kernels (3, 3, cin, cout) and biases; per direction, forward first,
    the LSTM kernel (in, 4H), recurrent kernel (H, 4H) and ONE bias; dense kernels (in, out) and biases) -> the torch-layout state dict."""
    weights = [np.asarray(w, np.float32) for w in weights]
    if len(weights) != len(KERAS_ORDER):
        raise MttsError(f"MOSNet: {len(weights)} Keras arrays given, the CNN-BLSTM has {len(KERAS_ORDER)}")
    sd = {}
    for name, w in zip(KERAS_ORDER, weights):
        if name.startswith("conv.") and name.endswith("weight"):
            w = w.transpose(3, 2, 0, 1) if w.ndim == 4 else w
        elif name.endswith("weight") or "weight_" in name:
            w = w.T
        sd[name] = np.ascontiguousarray(w)
    return check_state_dict(sd, n_freq)


def forward_basis(window="hamming", n_freq: int = 257):
    """[2 n_freq][n_fft] float32 for `mtts_stft_load`: the real and imaginary rows of the DFT times the analysis window of length n_fft.
    "hamming" / "hann" are the SYMMETRIC windows (numpy's); another name goes to scipy.signal.get_window(., fftbins=False); an array is used
    as it is."""
    n_fft = 2 * (int(n_freq) - 1)
    if isinstance(window, str):
        if window == "hamming":
            w = np.hamming(n_fft)
        elif window == "hann":
            w = np.hanning(n_fft)
        else:
            from scipy.signal import get_window
            w = get_window(window, n_fft, fftbins=False)
    else:
        w = np.asarray(window, np.float64).reshape(n_fft)
    fb = np.fft.fft(np.eye(n_fft))[:n_freq]
    return np.ascontiguousarray(np.vstack([fb.real, fb.imag]) * w[None, :], np.float32)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class MOSNet:
    """The device MOSNet.  `score_magnitudes(mags)` takes a list of [T][n_freq] magnitude spectrograms, `score_wavs(wavs, source_rate)`
    waveforms; both return (utterance scores float32 [n], [frame scores float32 [T]]) and cut a long list into device calls of at most
    `frames_per_call` frames — an utterance's scores are the same bits under any cut."""

    def __init__(self, state_dict=None, n_freq=257, max_frames=8192, max_utts=1024, lib_path=None, device=0, window="hamming", max_samples=SAMPLING_RATE * 120):
        self.lib = _lib.load(lib_path)
        self.n_freq, self.max_frames, self.max_utts = int(n_freq), int(max_frames), int(max_utts)
        self.device, self._lib_path, self.window, self.max_samples = device, lib_path, window, int(max_samples)
        self._front, self._resamplers = None, {}
        self.hop = min(HOP, self.n_freq - 1)      # 256 at the published width; a narrow test spectrum keeps hop <= filter length
        h = C.c_void_p()
        self.h = None
        if self.lib.mtts_mosnet_create(self.n_freq, self.max_frames, self.max_utts, device, C.byref(h)) != 0:
            raise MttsError(self.lib.mtts_mosnet_last_error(None).decode())
        self.h = h
        sd = state_dict if state_dict is not None else synthetic_state_dict(0, self.n_freq)
        self.state_dict_ = sd
        try:
            for k, v in pack_tensors(sd, self.n_freq).items():
                self.load(k, v)
        except Exception:
            self.close()
            raise

    def _check(self, rc):
        if rc != 0:
            raise MttsError(self.lib.mtts_mosnet_last_error(self.h).decode())

    def load(self, name, array):
        a = np.ascontiguousarray(array, np.float32)
        self._check(self.lib.mtts_mosnet_load(self.h, name.encode(), _ptr(a), a.size))

    def close(self):
        for r in self._resamplers.values():
            r.close()
        self._resamplers = {}
        if self._front is not None:
            self._front.close()
            self._front = None
        if getattr(self, "h", None):
            self.lib.mtts_mosnet_destroy(self.h)
            self.h = None

    def set_stream(self, stream_ptr):
        self.lib.mtts_mosnet_set_stream(self.h, C.c_void_p(stream_ptr))

    def _cuts(self, frames, frames_per_call):
        """Consecutive runs [lo, hi) of at most frames_per_call frames and max_utts utterances; an utterance beyond the budget goes alone
        (and is refused by the device when it exceeds max_frames)."""
        budget = self.max_frames if frames_per_call is None else max(1, min(int(frames_per_call), self.max_frames))
        lo, acc, out = 0, 0, []
        for i, t in enumerate(frames):
            if i > lo and (acc + t > budget or i - lo >= self.max_utts):
                out.append((lo, i))
                lo, acc = i, 0
            acc += int(t)
        out.append((lo, len(frames)))
        return out

    def score_magnitudes(self, mags, frames_per_call=None):
        ms = [np.ascontiguousarray(np.asarray(m, np.float32)) for m in mags]
        if not ms:
            raise MttsError("no spectrograms")
        for m in ms:
            if m.ndim != 2 or m.shape[1] != self.n_freq:
                raise MttsError(f"score_magnitudes: a spectrogram of shape {m.shape}, need [T][{self.n_freq}]")
        frames = [m.shape[0] for m in ms]
        utt, fr = np.empty(len(ms), np.float32), []
        for lo, hi in self._cuts(frames, frames_per_call):
            n = np.asarray(frames[lo:hi], np.int32)
            packed = np.ascontiguousarray(np.concatenate(ms[lo:hi], axis=0)) if int(n.sum()) else np.zeros((1, self.n_freq), np.float32)
            fs, us = np.empty(max(int(n.sum()), 1), np.float32), np.empty(hi - lo, np.float32)
            self._check(self.lib.mtts_mosnet_score(self.h, hi - lo, _ptr(n), _ptr(packed), _ptr(us), _ptr(fs)))
            utt[lo:hi] = us
            fr += [f.copy() for f in np.split(fs[:int(n.sum())], np.cumsum(n)[:-1])]
        return utt, fr

    def front(self):
        """The filter length 2 (n_freq - 1), hop 256 `mtts_stft` handle `score_wavs` owns, with the windowed basis loaded (created on first use)."""
        if self._front is None:
            from .audio.stft import _Handle
            self._front = _Handle(2 * (self.n_freq - 1), self.hop, 1, self.max_samples, self.device, self._lib_path)
            fb = forward_basis(self.window, self.n_freq)
            self._front.check(self.lib.mtts_stft_load(self._front.h, _ptr(fb), None))
        return self._front

    def resampler(self, source_rate: int, preset: str = "kaiser_best"):
        """The Resampler source_rate -> 16 kHz on `front()` (the preset `SpeakerEmbedder.resampler` uses), created once per rate."""
        key = (int(source_rate), preset)
        if key not in self._resamplers:
            from .audio.resample import Resampler
            self._resamplers[key] = Resampler(int(source_rate), SAMPLING_RATE, preset, _handle=self.front())
        return self._resamplers[key]

    def score_wavs(self, wavs, source_rate=None, frames_per_call=None):
        """Waveforms at 16 kHz (source_rate None or 16000) or at source_rate, resampled to 16 kHz on the device in front of the STFT."""
        from .audio.stft import _pack_wavs
        ws, n, _ = _pack_wavs(wavs)
        front = self.front()
        rs = self.resampler(source_rate) if source_rate is not None and int(source_rate) != SAMPLING_RATE else None
        n16 = [rs.output_length(int(k)) if rs is not None else int(k) for k in n]
        frames = [k // self.hop + 1 for k in n16]
        utt, fr = np.empty(len(ws), np.float32), []
        for lo, hi in self._cuts(frames, frames_per_call):
            if rs is not None:
                rs.ensure_loaded()
            packed = np.ascontiguousarray(np.concatenate(ws[lo:hi]))
            nn = np.ascontiguousarray(n[lo:hi])
            total = int(sum(frames[lo:hi]))
            fs, us, nf = np.empty(max(total, 1), np.float32), np.empty(hi - lo, np.float32), np.zeros(hi - lo, np.int32)
            self._check(self.lib.mtts_mosnet_score_wavs(self.h, front.h, hi - lo, _ptr(nn), _ptr(packed), int(rs is not None), _ptr(us), _ptr(nf), _ptr(fs)))
            assert [int(t) for t in nf] == frames[lo:hi]
            utt[lo:hi] = us
            fr += [f.copy() for f in np.split(fs[:total], np.cumsum(nf)[:-1])]
        return utt, fr

    def __call__(self, wav, rate=SAMPLING_RATE):
        """One waveform -> its score (speechmetrics' `mosnet(path)['mosnet']` on an already loaded file)."""
        return float(self.score_wavs([wav], source_rate=rate)[0][0])
