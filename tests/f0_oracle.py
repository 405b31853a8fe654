"""The F0 definition of include/mtts.h (mtts_stft_load_pitch / mtts_stft_f0_batch) in numpy: YIN (de Cheveigné & Kawahara 2002) on
DIO's frame grid.  float64 is the oracle; `dtype=np.float32` runs the same arithmetic in float32 in the device's summation order (the
difference function as a chain of fused multiply-adds in ascending j — emulated as one float64 operation rounded to float32, which
differs from a true FMA only where that double rounding falls on a tie —, the running sum in ascending tau, the energy as 16
interleaved partial sums added in order; refinement and division in float64 on both sides).

Besides f0 and the chosen d' ("aperiodicity") every frame gets a decision margin: the smallest |d'(tau) - threshold| over the local
minima of d' restricted to the search range [tau_min, tau_max) (an end of the range counts when it is not above its one neighbour
inside).  The voicing decision and the lag chosen can only change when one of these minima crosses the threshold, so a frame with
margin < UNDECIDED is one on which two correct implementations may disagree.  Silent frames have margin 1.

Also here: the seeded test signals (silence, a six-harmonic glide, white noise, the glide again) and their ground truth."""
import math

import numpy as np

UNDECIDED = 1e-3
CONFIGS = ((22050, 256), (16000, 200), (8000, 64))
SEEDS = (0, 1, 2)


def window(sr, f0_floor=71.0, f0_ceil=800.0):
    """(tau_min, tau_max, W, L)"""
    tau_max, tau_min = int(math.ceil(sr / f0_floor)), int(math.floor(sr / f0_ceil))
    W = ((int(math.ceil(1.5 * tau_max)) + 63) // 64) * 64
    return tau_min, tau_max, W, W + tau_max


def spans(n, sr, hop, f0_floor=71.0, f0_ceil=800.0):
    """[T, 2]: first and one-past-last sample index of every frame's span (may lie outside 0 .. n)."""
    _, _, _, L = window(sr, f0_floor, f0_ceil)
    start = np.arange(n // hop + 1, dtype=np.int64) * hop - L // 2
    return np.stack([start, start + L], axis=1)


def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def yin(x, sr, hop, f0_floor=71.0, f0_ceil=800.0, threshold=0.15, silence_rms=1e-4, dtype=np.float64):
    """(f0 float64 [T], aperiodicity [T] of dtype, margin float64 [T]) for one utterance."""
    dt = np.dtype(dtype).type
    x = np.asarray(x, np.float32).astype(dt)              # the device reads float32 waveforms
    tmin, tmax, W, L = window(sr, f0_floor, f0_ceil)
    T = len(x) // hop + 1
    xp = np.concatenate([np.zeros(L // 2, dt), x, np.zeros(L + hop, dt)])
    S = np.stack([xp[t * hop: t * hop + L] for t in range(T)])                       # [T, L]
    a = S[:, :W]
    d = np.zeros((T, tmax + 1), dt)
    if dt is np.float32:
        for j in range(W):
            diff = a[:, j, None] - S[:, j: j + tmax + 1]
            d = _fma32(diff, diff, d)
        part = np.zeros((T, 16), np.float32)
        for j in range(0, W, 16):
            part = _fma32(a[:, j: j + 16], a[:, j: j + 16], part)
        e = np.zeros(T, np.float32)
        for p in range(16):
            e = e + part[:, p]
    else:
        for tau in range(tmax + 1):
            diff = a - S[:, tau: tau + W]
            d[:, tau] = np.sum(diff * diff, axis=1)
        e = np.sum(a * a, axis=1)
    cs = np.cumsum(d[:, 1:], axis=1, dtype=dt)
    dp = np.ones((T, tmax + 1), dt)
    with np.errstate(all="ignore"):
        dp[:, 1:] = np.where(cs > 0, d[:, 1:] * np.arange(1, tmax + 1, dtype=dt)[None, :] / cs, dt(1))
    thr = dt(threshold)
    f0, ap, margin = np.zeros(T, np.float64), np.ones(T, dt), np.ones(T, np.float64)
    for t in range(T):
        if float(e[t]) / W < silence_rms * silence_rms:
            continue
        r = dp[t]
        seg = r[tmin:tmax]
        left = np.concatenate([[True], seg[1:] <= seg[:-1]])
        right = np.concatenate([seg[:-1] <= seg[1:], [True]])
        margin[t] = float(np.abs(seg[left & right].astype(np.float64) - float(thr)).min())
        below = np.nonzero(seg < thr)[0]
        if len(below) == 0:
            continue
        tau = tmin + int(below[0])
        while tau + 1 < tmax and r[tau + 1] < r[tau]:
            tau += 1
        off = 0.0
        if tmin < tau < tmax - 1:
            y0, y1, y2 = float(r[tau - 1]), float(r[tau]), float(r[tau + 1])
            den = y0 - 2.0 * y1 + y2
            off = 0.5 * (y0 - y2) / den if den != 0 else 0.0
        f0[t] = sr / (tau + off)
        ap[t] = r[tau]
    return f0, ap, margin


def signal(sr, seed, n=None):
    """(x float32 [n], truth float64 [n], segments): n = 0.6 s + 37 * seed samples; a glide of six harmonics (amplitudes 0.2 / h) from
    90-160 Hz to 160-320 Hz whose first eighth is silence and whose third quarter is white noise at 0.1.  truth = the glide's frequency
    per sample, 0 in silence and noise; segments = [(kind, first, one past last)] with kind in "silence", "tone", "noise"."""
    n = int(sr * 0.6) + 37 * seed if n is None else n
    g = np.random.RandomState(seed)
    t = np.arange(n) / sr
    fa, fb = g.uniform(90, 160), g.uniform(160, 320)
    f = fa + (fb - fa) * t / t[-1]
    ph = 2 * np.pi * np.cumsum(f) / sr
    x = sum(np.sin(h * ph + g.uniform(0, 6.28)) / h for h in range(1, 7)) * 0.2
    truth = f.copy()
    q = n // 4
    x[: q // 2] = 0
    truth[: q // 2] = 0
    x[2 * q: 3 * q] = 0.1 * g.standard_normal(q)
    truth[2 * q: 3 * q] = 0
    return x.astype(np.float32), truth, [("silence", 0, q // 2), ("tone", q // 2, 2 * q), ("noise", 2 * q, 3 * q), ("tone", 3 * q, n)]


def frames_inside(n, sr, hop, segments, kinds):
    """bool [T]: the frame's span lies wholly inside one segment whose kind is in `kinds`."""
    sp = spans(n, sr, hop)
    inside = np.zeros(len(sp), bool)
    for kind, lo, hi in segments:
        if kind in kinds:
            inside |= (sp[:, 0] >= lo) & (sp[:, 1] <= hi)
    return inside


def tone(sr, hz, secs=0.3, amp=0.3, n=None):
    return (amp * np.sin(2 * np.pi * hz * np.arange(int(sr * secs) if n is None else n) / sr)).astype(np.float32)
