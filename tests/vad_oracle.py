"""The silence-trimming definition of include/mtts.h in float64 numpy, independent of the package (tests/test_vad_trim.py).

webrtcvad's decision is not restated anywhere (parity UNPINNED); what is written here is the energy detector that stands in its place
and resemblyzer's post-processing of per-window flags: the moving average as resemblyzer writes it (a cumulative sum over the zero-padded
array, np.round) and a direct binary dilation."""
import numpy as np

SR, WINDOW_MS, MA_WIDTH, MAX_SILENCE = 16000, 30, 8, 6
FLOOR_DB, NOISE_QUANTILE, MARGIN_DB = -50.0, 0.1, 10.0
W = WINDOW_MS * SR // 1000


def energies(wav, window=W):
    x = np.asarray(wav, np.float32).astype(np.float64)
    n_w = len(x) // window
    return np.mean(x[: n_w * window].reshape(n_w, window) ** 2, axis=1) if n_w else np.zeros(0)


def threshold(e, floor_db=FLOOR_DB, noise_quantile=NOISE_QUANTILE, margin_db=MARGIN_DB):
    k = int(np.floor(noise_quantile * (len(e) - 1)))
    return max(10.0 ** (floor_db / 10.0), float(np.sort(e)[k]) * 10.0 ** (margin_db / 10.0))


def raw_flags(e, **kw):
    return e >= threshold(e, **kw) if len(e) else np.zeros(0, bool)


def margin(e, **kw):
    """min over the windows of |e[w] - threshold| / threshold: the tests construct inputs that keep it above 1e-9."""
    if not len(e):
        return np.inf
    t = threshold(e, **kw)
    return float(np.min(np.abs(e - t)) / t)


def moving_average(array, width):
    array_padded = np.concatenate((np.zeros((width - 1) // 2), array, np.zeros(width // 2)))
    ret = np.cumsum(array_padded, dtype=float)
    ret[width:] = ret[width:] - ret[:-width]
    return ret[width - 1:] / width


def dilate(flags, length):
    """binary dilation by a centred structure of `length` ones (origin at length // 2): out[w] = any flags[w - (length - 1) // 2 .. w + length // 2]."""
    n = len(flags)
    out = np.zeros(n, bool)
    for w in range(n):
        lo, hi = max(0, w - (length - 1) // 2), min(n, w + length // 2 + 1)
        out[w] = flags[lo:hi].any()
    return out


def post(flags, ma_width=MA_WIDTH, max_silence=MAX_SILENCE):
    flags = np.asarray(flags).astype(bool)
    if not len(flags):
        return flags
    return dilate(np.round(moving_average(flags.astype(np.float64), ma_width)).astype(bool), max_silence + 1)


def trim(wav, flags=None, window=W, ma_width=MA_WIDTH, max_silence=MAX_SILENCE, **kw):
    """(out, mask, n_voiced, energies): energies None when flags are injected.  No window kept: the waveform as it is, n_voiced 0."""
    wav = np.asarray(wav, np.float32)
    e = None
    if flags is None:
        e = energies(wav, window)
        flags = raw_flags(e, **kw)
    mask = post(flags, ma_width, max_silence)
    assert len(mask) == len(wav) // window
    if not mask.any():
        return wav, mask, 0, e
    return wav[: len(mask) * window][np.repeat(mask, window)], mask, int(mask.sum()), e


def speechlike(n, seed, sr=SR, noise=1e-4):
    """Bursts of a loud chirp between stretches of faint noise: leading, inner and trailing `silence`."""
    g = np.random.RandomState(seed)
    t = np.arange(n) / sr
    x = noise * g.standard_normal(n)
    gate = (np.sin(2 * np.pi * (0.7 + 0.3 * g.rand()) * t + g.rand() * 6.28) > -0.2).astype(np.float64)
    gate[: min(n, int(0.2 * sr * g.rand()))] = 0
    x += gate * 0.3 * np.sin(2 * np.pi * (150 + 50 * g.rand()) * t * (1 + 0.3 * t / max(t[-1], 1e-3)))
    return x.astype(np.float32)
