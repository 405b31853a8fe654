"""`STFT` and `TacotronSTFT` on libmtts.so (reference audio/stft.py:15-178).

The bases are built on the host exactly as the reference builds its buffers — `np.fft.fft(np.eye(n))` split into real / imaginary
rows and multiplied by the periodic Hann window (stft.py:27-46; scipy.signal.get_window, as there) — and the Slaney mel filter
bank of `librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax)` (librosa is not part of this image: restated from its documented
algorithm, htk=False, norm="slaney").  The device does the framing, both contractions, magnitude, log and energy (csrc/melfront.h,
the front-end every audio stage shares); in the inverse direction (csrc/griffin.h) the inverse-basis contraction, the overlap-add
and whole Griffin-Lim loops."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from .. import _lib
from ..engine import MttsError


def forward_basis(filter_length: int, win_length: int, window: str = "hann") -> np.ndarray:
    """[2 * (filter_length // 2 + 1)][filter_length] float32 — STFT.forward_basis without its singleton channel axis."""
    from scipy.signal import get_window
    fb = np.fft.fft(np.eye(filter_length))
    cutoff = filter_length // 2 + 1
    basis = np.vstack([np.real(fb[:cutoff, :]), np.imag(fb[:cutoff, :])]).astype(np.float32)   # torch.FloatTensor(...) in the reference
    assert filter_length >= win_length
    w = get_window(window, win_length, fftbins=True)
    lpad = (filter_length - win_length) // 2                                                    # librosa.util.pad_center
    w = np.pad(w, (lpad, filter_length - win_length - lpad))
    return (basis * w.astype(np.float32)[None, :]).astype(np.float32)


@functools.lru_cache(maxsize=8)
def _inverse_basis(filter_length: int, hop_length: int, win_length: int, window: str) -> np.ndarray:
    fb = np.fft.fft(np.eye(filter_length))
    cutoff = filter_length // 2 + 1
    fourier = np.vstack([np.real(fb[:cutoff, :]), np.imag(fb[:cutoff, :])])
    inv = np.linalg.pinv((filter_length / hop_length) * fourier).T.astype(np.float32)       # torch.FloatTensor(...) in the reference
    from .audio_processing import _window
    w = _window(window, win_length, filter_length).astype(np.float32)
    out = (inv * w[None, :]).astype(np.float32)
    out.setflags(write=False)
    return out


def inverse_basis(filter_length: int, hop_length: int, win_length: int, window: str = "hann") -> np.ndarray:
    """[2 * (filter_length // 2 + 1)][filter_length] float32 — STFT.inverse_basis (stft.py:33-45) without its singleton channel axis:
    np.linalg.pinv(scale * fourier_basis).T with scale = filter_length / hop_length, cast to float32, times the float32 window."""
    assert filter_length >= win_length
    return _inverse_basis(int(filter_length), int(hop_length), int(win_length), window).copy()


class _Handle:
    """One `mtts_stft` device handle: create, error check, close.  An STFT, the TacotronSTFT it belongs to and a Preprocessor built on
    that TacotronSTFT all hold the same one."""

    def __init__(self, filter_length, hop_length, n_mel, max_samples, device, lib_path):
        self.lib = _lib.load(lib_path)
        h = C.c_void_p()
        if self.lib.mtts_stft_create(filter_length, hop_length, n_mel, max_samples, device, C.byref(h)) != 0:
            raise MttsError(self.lib.mtts_stft_last_error(None).decode())
        self.h = h
        self.hop_length = int(hop_length)

    def check(self, rc):
        if rc < 0:
            raise MttsError(self.lib.mtts_stft_last_error(self.h).decode())
        return rc

    def close(self):
        if getattr(self, "h", None):
            self.lib.mtts_stft_destroy(self.h)
        self.h = None

    __del__ = close


class _OnHandle:
    """`lib`, `h` and `_check` of the `_Handle` in `self._dev`."""
    lib = property(lambda self: self._dev.lib)
    h = property(lambda self: self._dev.h)

    def _check(self, rc):
        return self._dev.check(rc)


class _StageOnHandle(_OnHandle):
    """A stage of which an `mtts_stft` handle holds ONE configuration at a time (a resampler bank, a pitch or a VAD configuration).
    A stand-alone stage owns a small handle; `_handle=` attaches it to an existing one.  A subclass names the handle attribute that
    records the configuration loaded (`_slot`), sets `_key` (its own configuration), and sends it to the device in `_load()`."""
    _slot = None

    def _attach(self, _handle, *create):
        self._owner = _handle is None
        self._dev = _handle if _handle is not None else _Handle(*create)

    def _first_load(self):
        try:
            self.load()
        except MttsError:
            self.close()
            raise

    def load(self):
        """Make this stage's configuration the handle's current one (done by the constructor)."""
        self._load()
        setattr(self._dev, self._slot, self._key)

    def ensure_loaded(self):
        """`load()` when the handle holds another configuration: before each use, since several stages may share a handle."""
        if getattr(self._dev, self._slot, None) != self._key:
            self.load()

    def close(self):
        if self._owner:
            self._dev.close()


def _pack_wavs(wavs):
    """A list of waveforms -> (the float32 vectors, their lengths int32, all of them one after another)."""
    ws = [np.ascontiguousarray(np.asarray(w, np.float32).reshape(-1)) for w in wavs]
    if not ws:
        raise MttsError("no waveforms")
    return ws, np.asarray([len(w) for w in ws], np.int32), np.ascontiguousarray(np.concatenate(ws))


def _np32(x):
    return np.ascontiguousarray(np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x, np.float32))


class STFT(_OnHandle):
    """audio/stft.py:15-125 on the device.  `transform(x)` takes (B, n) waveforms and returns (magnitude, phase), each (B, F, T) float32;
    `inverse(magnitude, phase)` takes (B, F, T) and returns (B, 1, hop * (T - 1)); `forward(x)` is inverse(transform(x)).  Inputs may be
    numpy arrays or torch tensors; outputs are numpy.  Only string windows (scipy.signal.get_window) are supported.

    A TacotronSTFT's `stft_fn` shares that TacotronSTFT's device handle (its `_Handle`, passed as `_handle`); a stand-alone STFT owns one."""

    def __init__(self, filter_length, hop_length, win_length, window="hann", *, max_samples=22050 * 40, device=0, lib_path=None,
                 _handle=None):
        if window is None:
            raise NotImplementedError("STFT(window=None): the device path divides by the window envelope; pass a window name")
        self.filter_length, self.hop_length, self.win_length, self.window = filter_length, hop_length, win_length, window
        self.n_bins = filter_length // 2 + 1
        self.forward_basis = forward_basis(filter_length, win_length, window)
        self._inverse_loaded = False
        self._owner = _handle is None
        self._dev = _handle if _handle is not None else _Handle(filter_length, hop_length, 1, max_samples, device, lib_path)
        if self._owner:
            self._check(self.lib.mtts_stft_load(self.h, self.forward_basis.ctypes.data_as(C.c_void_p), None))

    @property
    def inverse_basis(self) -> np.ndarray:
        return inverse_basis(self.filter_length, self.hop_length, self.win_length, self.window)

    def _ensure_inverse(self):
        """The inverse basis (a pseudo-inverse on the host) and the squared window go to the device on first use."""
        if self._inverse_loaded:
            return
        from .audio_processing import _window
        ib = self.inverse_basis
        wsq = (_window(self.window, self.win_length, self.filter_length) ** 2).astype(np.float32)
        self._check(self.lib.mtts_stft_load_inverse(self.h, ib.ctypes.data_as(C.c_void_p), wsq.ctypes.data_as(C.c_void_p)))
        self._inverse_loaded = True

    def close(self):
        if self._owner:
            self._dev.close()

    def _frames_of(self, n_frames, what, transforms=True):
        n = np.asarray(n_frames, np.int32).reshape(-1)
        bad = (n < 1) | (transforms & (self.hop_length * (n.astype(np.int64) - 1) <= self.filter_length // 2))
        if bad.any():
            raise MttsError(f"{what}: spectrogram too short: {int(n[bad][0])} frames give a waveform of hop_length * (T - 1) samples, which must exceed "
                            f"filter_length / 2 = {self.filter_length // 2} (the reference's reflection padding raises)")
        return np.ascontiguousarray(n)

    def transform(self, input_data):
        """stft.py:52-77: reflect padding WITHOUT clipping, (magnitude, phase) each (B, F, T)."""
        x = _np32(input_data)
        if x.ndim == 1:
            x = x[None]
        n = x.shape[1]
        if n <= self.filter_length // 2:
            raise MttsError(f"transform: {n} samples is too short for the reflection padding of filter_length / 2 = {self.filter_length // 2}")
        T = n // self.hop_length + 1
        mag = np.empty((x.shape[0], T, self.n_bins), np.float32)
        ph = np.empty_like(mag)
        for b in range(x.shape[0]):
            row = np.ascontiguousarray(x[b])
            got = self._check(self.lib.mtts_stft_transform(self.h, row.ctypes.data_as(C.c_void_p), n, mag[b].ctypes.data_as(C.c_void_p),
                                                           ph[b].ctypes.data_as(C.c_void_p)))
            assert got == T
        return mag.transpose(0, 2, 1), ph.transpose(0, 2, 1)

    def _packed(self, fn, mats, frames, extra, n_out):
        self._ensure_inverse()
        out = np.empty(int(n_out), np.float32)
        got = self._check(fn(self.h, len(frames), frames.ctypes.data_as(C.c_void_p), *[m.ctypes.data_as(C.c_void_p) for m in mats], *extra,
                             out.ctypes.data_as(C.c_void_p)))
        assert got == n_out, (got, n_out)
        return out

    def _batched(self, magnitude, angles, n_iters):
        """(B, F, T) magnitude and angles -> (B, hop * (T - 1)) through one device call."""
        m, a = _np32(magnitude), _np32(angles)
        if m.ndim == 2:
            m, a = m[None], a[None]
        assert m.shape == a.shape and m.shape[1] == self.n_bins, (m.shape, a.shape)
        B, _, T = m.shape
        frames = self._frames_of([T] * B, "inverse" if not n_iters else "griffin_lim", transforms=bool(n_iters))
        mf = np.ascontiguousarray(m.transpose(0, 2, 1)).reshape(B * T, self.n_bins)
        af = np.ascontiguousarray(a.transpose(0, 2, 1)).reshape(B * T, self.n_bins)
        L = self.hop_length * (T - 1)
        if n_iters is None:
            out = self._packed(self.lib.mtts_stft_inverse, (mf, af), frames, (), B * L)
        else:
            if int(n_iters) < 0:
                raise MttsError("griffin_lim: n_iters < 0")
            out = self._packed(self.lib.mtts_stft_griffin_lim, (mf, af), frames, (int(n_iters),), B * L)
        return out.reshape(B, L)

    def inverse(self, magnitude, phase):
        """stft.py:79-119: (B, F, T) magnitude and phase -> (B, 1, hop * (T - 1)) float32."""
        return self._batched(magnitude, phase, None)[:, None, :]

    def griffin_lim_with_angles(self, magnitudes, angles, n_iters):
        """audio_processing.py:66-80 from given starting phases: (B, F, T) -> (B, hop * (T - 1))."""
        return self._batched(magnitudes, angles, n_iters)

    def forward(self, input_data):
        magnitude, phase = self.transform(input_data)
        return self.inverse(magnitude, phase)

    __call__ = forward


def _hz_to_mel(f):
    f = np.asanyarray(f, np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-30) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asanyarray(m, np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_filterbank(sr: int, n_fft: int, n_mels: int, fmin: float = 0.0, fmax=None) -> np.ndarray:
    """librosa.filters.mel (Slaney scale, slaney area normalisation): [n_mels][n_fft // 2 + 1] float32."""
    fmax = float(sr) / 2 if fmax is None else float(fmax)
    fftfreqs = np.linspace(0, float(sr) / 2, n_fft // 2 + 1)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    w = np.zeros((n_mels, n_fft // 2 + 1))
    for i in range(n_mels):
        lower, upper = -ramps[i] / fdiff[i], ramps[i + 2] / fdiff[i + 1]
        w[i] = np.maximum(0, np.minimum(lower, upper))
    w *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]
    return w.astype(np.float32)


class TacotronSTFT(_OnHandle):
    """audio/stft.py:128: same constructor arguments; `mel_spectrogram(y)` takes (B, T) waveforms in [-1, 1] and returns
    (mel (B, n_mel, T'), energy (B, T')) float32 arrays."""

    def __init__(self, filter_length, hop_length, win_length, n_mel_channels, sampling_rate, mel_fmin, mel_fmax, *, max_samples=22050 * 40,
                 device=0, lib_path=None):
        self.filter_length, self.hop_length, self.win_length = filter_length, hop_length, win_length
        self.n_mel_channels, self.sampling_rate = n_mel_channels, sampling_rate
        self.forward_basis = forward_basis(filter_length, win_length)
        self.mel_basis = mel_filterbank(sampling_rate, filter_length, n_mel_channels, mel_fmin or 0.0, mel_fmax)
        self._dev = _Handle(filter_length, hop_length, n_mel_channels, max_samples, device, lib_path)
        self._check(self.lib.mtts_stft_load(self.h, self.forward_basis.ctypes.data_as(C.c_void_p), self.mel_basis.ctypes.data_as(C.c_void_p)))
        self.stft_fn = STFT(filter_length, hop_length, win_length, _handle=self._dev)   # stft.py:140 (shares this handle)
        self._stft_fn = self.stft_fn   # the name audio/tools.py:inv_mel_spec reads (the reference's TacotronSTFT lacks it)

    def set_stream(self, stream_ptr: int):
        if self.lib.mtts_stft_set_stream(self.h, C.c_void_p(stream_ptr)) != 0:
            raise RuntimeError("mtts_stft_set_stream failed")

    def close(self):
        self._dev.close()

    def spectral_normalize(self, magnitudes):
        from .audio_processing import dynamic_range_compression
        return dynamic_range_compression(magnitudes)

    def spectral_de_normalize(self, magnitudes):
        from .audio_processing import dynamic_range_decompression
        return dynamic_range_decompression(magnitudes)

    def inv_mel_with_angles(self, log_mels, angles, n_iters):
        """tools.py:18-37 up to the waveform for a list of log-mels (n_mel, Tm_u) and starting phases (F, Tm_u - 1): one device call,
        returns the list of waveforms (hop * (Tm_u - 2) samples each)."""
        mels = [_np32(m) for m in log_mels]
        if int(n_iters) < 0:
            raise MttsError("inv_mel: n_iters < 0")
        tm = np.asarray([m.shape[1] for m in mels], np.int32)
        for m, a in zip(mels, angles):
            assert m.shape[0] == self.n_mel_channels and a.shape == (self.stft_fn.n_bins, m.shape[1] - 1), (m.shape, a.shape)
        self.stft_fn._frames_of(tm - 1, "inv_mel (the last mel frame is dropped)", transforms=int(n_iters) > 0)
        lm = np.ascontiguousarray(np.concatenate([m.T for m in mels], axis=0))
        af = np.ascontiguousarray(np.concatenate([_np32(a).T for a in angles], axis=0))
        lens = self.hop_length * (tm.astype(np.int64) - 2)
        out = self.stft_fn._packed(self.lib.mtts_stft_inv_mel, (lm, af), np.ascontiguousarray(tm), (int(n_iters),), int(lens.sum()))
        return np.split(out, np.cumsum(lens)[:-1])

    def mel_spectrogram(self, y):
        y = np.ascontiguousarray(np.asarray(y.detach().cpu().numpy() if hasattr(y, "detach") else y, np.float32))
        assert y.ndim == 2
        assert y.min() >= -1 and y.max() <= 1      # stft.py:168-169
        T = y.shape[1] // self.hop_length + 1
        mel = np.empty((y.shape[0], T, self.n_mel_channels), np.float32)
        energy = np.empty((y.shape[0], T), np.float32)
        for b in range(y.shape[0]):
            got = self._check(self.lib.mtts_stft_mel_spectrogram(self.h, y[b].ctypes.data_as(C.c_void_p), y.shape[1], mel[b].ctypes.data_as(C.c_void_p),
                                                                 energy[b].ctypes.data_as(C.c_void_p)))
            assert got == T
        return mel.transpose(0, 2, 1), energy
