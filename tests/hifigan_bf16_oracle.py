"""TEST INFRASTRUCTURE ONLY — the bf16-operand mode of the HiFi-GAN generator (include/mtts.h: mtts_hifigan_set_numerics, mode 1) restated
with torch.nn.functional, independent of the package (tests/test_hifigan_bf16.py).  It is tests/hifigan_oracle.py's graph with ONE change:
conv_pre, every transposed convolution and every residual convolution multiply operands rounded to bf16 — the activation operand (the
scaled mel for conv_pre, the LeakyReLU image elsewhere) and the folded fp32 weight, each rounded once by torch's own
`.to(torch.bfloat16)` of the float32 value (in the float64 evaluation the operand is first taken to float32).  Products and sums are
then carried in `dtype`: float64 is the arbiter (exact products, no accumulation error), float32 restates the device's arithmetic in
another summation order.  Bias, LeakyReLU, residual add, the MRF mean and conv_post + tanh are not rounded.  `round_operands=False` is
tests/hifigan_oracle.py again."""
import numpy as np
import torch
import torch.nn.functional as F

from hifigan_oracle import _weight


def bf16_round(x, on=True):
    """x (any float dtype) -> the same dtype, every element the bf16 neighbour (round to nearest even) of its float32 value."""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype) if on else x


def conv_rows(x, lens, w, bias, k, d, in_slope=1.0, dtype=torch.float64, round_operands=True):
    """One convolution of the mode on channels-last rows, as mtts_hifigan_conv_bf16 sees it: x [B][T][C], w [C][k][C] (out, tap, in),
    zero padding at each utterance's own ends (rows >= lens[b] are not read).  -> bias + conv, [B][T][C] in `dtype` (rows >= lens[b]: 0)."""
    x, w, bias = (torch.as_tensor(np.asarray(a, np.float32)) for a in (x, w, bias))
    out = torch.zeros(x.shape, dtype=dtype)
    wt = bf16_round(w, round_operands).to(dtype).permute(0, 2, 1).contiguous()   # [out][in][tap]
    with torch.no_grad():
        for b, L in enumerate(lens):
            a = F.leaky_relu(x[b, :L], in_slope) if in_slope != 1.0 else x[b, :L]   # (float32, as the device computes it)
            a = bf16_round(a, round_operands).to(dtype).T[None]
            out[b, :L] = F.conv1d(a, wt, bias.to(dtype), dilation=d, padding=d * (k - 1) // 2)[0].T
    return out.numpy()


def generator(sd, mel, config, dtype=torch.float64, round_operands=True, mel_scale=1.0):
    """mel (B, n_mel, T) -> (B, T * hop) in `dtype`; every utterance at full length T (run ragged batches one utterance at a time)."""
    R = lambda t: bf16_round(t, round_operands)
    with torch.no_grad():
        W = lambda n: R(_weight(sd, n, dtype))
        Bv = lambda n: torch.as_tensor(np.asarray(sd[n + ".bias"]), dtype=torch.float32).to(dtype)
        x = torch.as_tensor(np.asarray(mel, np.float32)).to(dtype)
        if mel_scale != 1.0:
            x = x * mel_scale
        x = F.conv1d(R(x), W("conv_pre"), Bv("conv_pre"), padding=3)
        n_k = len(config["resblock_kernel_sizes"])
        for i, (r, ku) in enumerate(zip(config["upsample_rates"], config["upsample_kernel_sizes"])):
            x = F.leaky_relu(x, 0.1)
            x = F.conv_transpose1d(R(x), W(f"ups.{i}"), Bv(f"ups.{i}"), stride=r, padding=(ku - r) // 2)
            xs = None
            for j, k in enumerate(config["resblock_kernel_sizes"]):
                y = x
                for m, d in enumerate(config["resblock_dilation_sizes"][j]):
                    n1, n2 = f"resblocks.{i * n_k + j}.convs1.{m}", f"resblocks.{i * n_k + j}.convs2.{m}"
                    t = F.leaky_relu(y, 0.1)
                    t = F.conv1d(R(t), W(n1), Bv(n1), dilation=d, padding=d * (k - 1) // 2)
                    t = F.leaky_relu(t, 0.1)
                    t = F.conv1d(R(t), W(n2), Bv(n2), dilation=1, padding=(k - 1) // 2)
                    y = t + y
                xs = y if xs is None else xs + y
            x = xs / n_k
        x = F.leaky_relu(x, 0.01)
        x = F.conv1d(x, _weight(sd, "conv_post", dtype), Bv("conv_post"), padding=3)
        return torch.tanh(x).squeeze(1).numpy()
