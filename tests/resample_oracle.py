"""TEST INFRASTRUCTURE ONLY — restatement of the resampler and the volume normaliser, the checker of meta_tts_amd/csrc/resample.h.

PARITY UNPINNED against librosa / resampy / resemblyzer (none is available).  What IS pinned: `resample` below, a direct evaluation of

    y[n] = sum_m h[n down - m up] x[m]   over |n down - m up| <= H, 0 <= m < n_in,   n_out = ceil(n_in up / down)

(no polyphase bank, no phases: the sum as written), equals scipy.signal.resample_poly with the same Kaiser window to 1e-13
(tests/test_resample.py::test_oracle_equals_scipy_resample_poly).  The filter is designed here independently of
meta_tts_amd/audio/resample.py: h[i] = fc sinc(fc i) kaiser(2 H + 1, beta)[i + H], fc = rolloff / max(up, down), H = zeros max(up,
down), scaled to sum(h) = up.  `normalize_volume` restates resemblyzer's published function."""
import math

import numpy as np

PRESETS = {"scipy": (10, 5.0, 1.0), "kaiser_fast": (16, 8.555504641634386, 0.85), "kaiser_best": (64, 14.769656459379492, 0.9475937167399596)}
PAIRS = [(22050, 16000), (24000, 22050), (24000, 16000), (48000, 22050), (16000, 22050)]      # (orig_sr, target_sr)


def design(orig_sr, target_sr, preset="kaiser_best"):
    """(up, down, H, h float64 [2 H + 1])."""
    zeros, beta, rolloff = PRESETS[preset]
    g = math.gcd(orig_sr, target_sr)
    up, down = target_sr // g, orig_sr // g
    mx = max(up, down)
    H = zeros * mx
    i = np.arange(-H, H + 1, dtype=np.float64)
    fc = rolloff / mx
    h = fc * np.sinc(fc * i) * np.kaiser(2 * H + 1, beta)
    return up, down, H, h * (up / h.sum())


def resample(x, up, down, H, h, dtype=np.float64, return_abs=False, block=4096):
    """The sum above for one waveform, products and sums in `dtype` (float32: h and x rounded to float32 first, numpy's float32 sum).
    return_abs: also sum_m |h32[.]| |x[m]| per output in float64 — the scale of the a-priori fp32 bound."""
    x64 = np.asarray(x, np.float64)
    n_in = len(x64)
    n_out = -(-n_in * up // down)
    hd, xd = np.asarray(h, dtype), np.asarray(x, dtype)
    habs = np.abs(np.asarray(h, np.float32).astype(np.float64))
    y, a = np.zeros(n_out, dtype), np.zeros(n_out, np.float64)
    width = 2 * H // up + 2
    for lo in range(0, n_out, block):
        c = np.arange(lo, min(lo + block, n_out), dtype=np.int64) * down            # positions on the up-sampled grid
        m_lo = -((H - c) // up)                                                       # ceil((c - H) / up)
        m = m_lo[:, None] + np.arange(width, dtype=np.int64)[None, :]
        k = c[:, None] - m * up                                                       # n down - m up
        ok = (np.abs(k) <= H) & (m >= 0) & (m < n_in)
        ki, mi = np.where(ok, k + H, 0), np.where(ok, m, 0)
        y[lo: lo + len(c)] = np.where(ok, hd[ki] * xd[mi], dtype(0)).sum(axis=1, dtype=dtype)
        if return_abs:
            a[lo: lo + len(c)] = np.where(ok, habs[ki] * np.abs(x64[mi]), 0.0).sum(axis=1)
    return (y, a) if return_abs else y


def gain_of(y, target_dbfs=-30.0, increase_only=True):
    """resemblyzer's normalize_volume in float64: the gain it applies to y (1.0 when it leaves y as it is)."""
    y = np.asarray(y, np.float64)
    change = target_dbfs - 10.0 * np.log10(np.mean(y ** 2))
    if change < 0 and increase_only:
        return 1.0
    return float(10.0 ** (change / 20.0))


def chirps(n, sr, seed, amp=1.0):
    """A sum of chirps + noise at `sr`, inside [-1, 1] for amp <= 1."""
    g = np.random.RandomState(seed)
    t = np.arange(n) / sr
    w = np.zeros(n)
    for k in range(3):
        f0, f1 = g.uniform(80, 400) * (k + 1), g.uniform(500, 0.45 * sr)
        w += g.uniform(0.1, 0.3) * np.sin(2 * np.pi * (f0 * t + 0.5 * (f1 - f0) / max(t[-1], 1e-3) * t * t) + g.uniform(0, 6))
    return (amp * (w + 0.02 * g.standard_normal(n))).astype(np.float32)
