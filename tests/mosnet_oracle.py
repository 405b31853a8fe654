"""TEST INFRASTRUCTURE ONLY — the MOSNet definition of include/mtts.h (mtts_mosnet_*) restated with torch.nn.functional on a state dict in
torch layouts, independent of the package (tests/test_mosnet.py).  Evaluated in float64 (the arbiter) and in float32 (whose distance to
float64 sets the tolerance), one utterance at a time.  Explicit F.pad + F.conv2d(padding=0); the BLSTM is a plain loop over frames."""
import numpy as np
import torch
import torch.nn.functional as F

CHANNELS = (16, 32, 64, 128)
H = 128


def same_pad(f_in, stride):
    """TensorFlow "same" for a 3-wide kernel: (F_out, left, right)."""
    f_out = -(-f_in // stride)
    total = max((f_out - 1) * stride + 3 - f_in, 0)
    return f_out, total // 2, total - total // 2


def conv_layer(x, w, b, stride):
    """x (1, cin, T, F) -> relu(conv3x3): one zero row before and after in time, "same" columns in frequency, stride (1, stride)."""
    _, left, right = same_pad(x.shape[3], stride)
    return F.relu(F.conv2d(F.pad(x, (left, right, 1, 1)), w, b, stride=(1, stride), padding=0))


def conv_stack(sd, mag, dtype, stats=None):
    """mag (T, n_freq) -> features (T, F4 * 128), frequency-major then channel.  stats: a list that receives each ReLU's positive share."""
    x = torch.as_tensor(np.ascontiguousarray(mag), dtype=dtype)[None, None]
    for l in range(12):
        x = conv_layer(x, torch.as_tensor(sd[f"conv.{l}.weight"], dtype=dtype), torch.as_tensor(sd[f"conv.{l}.bias"], dtype=dtype), 3 if l % 3 == 2 else 1)
        if stats is not None:
            stats.append(float((x > 0).double().mean()))
    return x[0].permute(1, 2, 0).reshape(x.shape[2], -1)       # (C, T, F) -> (T, F, C) -> (T, F * C)


def lstm_direction(x, w_ih, w_hh, b, reverse, pre=None):
    """Gate order i, f, g, o; zero initial state; reverse: from the last frame to the first.  -> (T, H), aligned with the frames."""
    T = x.shape[0]
    h, c = torch.zeros(H, dtype=x.dtype), torch.zeros(H, dtype=x.dtype)
    out = [None] * T
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        z = w_ih @ x[t] + w_hh @ h + b
        if pre is not None:
            pre.append(z)
        i, f, g, o = torch.sigmoid(z[:H]), torch.sigmoid(z[H:2 * H]), torch.tanh(z[2 * H:3 * H]), torch.sigmoid(z[3 * H:])
        c = f * c + i * g
        h = o * torch.tanh(c)
        out[t] = h
    return torch.stack(out)


def blstm_head(sd, feats, dtype, pre=None):
    """features (T, IN) -> frame scores (T,): BLSTM, Dense + ReLU, Dense.  The magnitudes-free entry of the backward-direction test."""
    t = lambda k: torch.as_tensor(sd[k], dtype=dtype)   # noqa: E731
    x = torch.as_tensor(np.asarray(feats), dtype=dtype) if not torch.is_tensor(feats) else feats.to(dtype)
    fw = lstm_direction(x, t("blstm.weight_ih"), t("blstm.weight_hh"), t("blstm.bias"), False, pre)
    bw = lstm_direction(x, t("blstm.weight_ih_reverse"), t("blstm.weight_hh_reverse"), t("blstm.bias_reverse"), True, pre)
    d = F.relu(torch.cat([fw, bw], dim=1) @ t("dense.weight").T + t("dense.bias"))
    return (d @ t("frame_score.weight").T + t("frame_score.bias"))[:, 0]


def network(sd, mags, n_freq, dtype=torch.float64, stats=None):
    """[(T, n_freq) magnitudes] -> ([utterance score], [frame scores (T,)]) as numpy arrays of `dtype`.  stats: a dict that receives
    'relu' (the positive share behind each of the 12 ReLUs, per utterance) and 'gates' (all BLSTM gate pre-activations, flat)."""
    utt, frames = [], []
    with torch.no_grad():
        for m in mags:
            m = np.asarray(m)
            assert m.ndim == 2 and m.shape[1] == n_freq, m.shape
            relu, pre = ([], []) if stats is not None else (None, None)
            fs = blstm_head(sd, conv_stack(sd, m, dtype, relu), dtype, pre)
            if stats is not None:
                stats.setdefault("relu", []).append(relu)
                stats.setdefault("gates", []).append(torch.cat(pre).double().numpy())
            frames.append(fs.numpy())
            utt.append(fs.mean().numpy()[()])
    return utt, frames


def stft_magnitude(wav, n_fft=512, hop=256, dtype=np.float64):
    """|STFT| with a symmetric Hamming window of length n_fft, centred with reflection padding: (n // hop + 1, n_fft // 2 + 1) in `dtype`
    (float32: every step in float32, the front-end's own precision)."""
    x = np.pad(np.asarray(wav, dtype), n_fft // 2, mode="reflect")
    T = len(wav) // hop + 1
    fr = np.stack([x[t * hop:t * hop + n_fft] for t in range(T)]) * np.hamming(n_fft).astype(dtype)[None, :]
    k = np.arange(n_fft // 2 + 1)[:, None] * np.arange(n_fft)[None, :]
    ang = 2.0 * np.pi * (k % n_fft) / n_fft
    re, im = fr @ np.cos(ang).astype(dtype).T, fr @ (-np.sin(ang)).astype(dtype).T
    return np.sqrt(re * re + im * im).astype(dtype)
