"""TEST INFRASTRUCTURE ONLY — the HiFi-GAN generator definition of include/mtts.h (mtts_hifigan_*) restated with torch.nn.functional on
a state dict in the published naming, independent of the package (tests/test_hifigan.py).  Evaluated in float64 (the arbiter) and in
float32 (whose distance to the arbiter sets the tolerance)."""
import numpy as np
import torch
import torch.nn.functional as F


def tensor_list(config, n_mel):
    """[(name, shape of the weight)] of every convolution, written down from the definition (not from the package's spec)."""
    c = config["upsample_initial_channel"]
    out = [("conv_pre", (c, n_mel, 7))]
    n_k = len(config["resblock_kernel_sizes"])
    for i, (r, ku) in enumerate(zip(config["upsample_rates"], config["upsample_kernel_sizes"])):
        out.append((f"ups.{i}", (c, c // 2, ku)))
        c //= 2
        for j, k in enumerate(config["resblock_kernel_sizes"]):
            for m in range(len(config["resblock_dilation_sizes"][j])):
                out.append((f"resblocks.{i * n_k + j}.convs1.{m}", (c, c, k)))
                out.append((f"resblocks.{i * n_k + j}.convs2.{m}", (c, c, k)))
    out.append(("conv_post", (1, c, 7)))
    return out


def _weight(sd, name, dtype):
    if name + ".weight" in sd:
        return torch.as_tensor(np.asarray(sd[name + ".weight"]), dtype=dtype)
    v = torch.as_tensor(np.asarray(sd[name + ".weight_v"]), dtype=torch.float64)
    g = torch.as_tensor(np.asarray(sd[name + ".weight_g"]), dtype=torch.float64).reshape(-1, 1, 1)
    w = g * v / v.pow(2).sum(dim=(1, 2), keepdim=True).sqrt()     # torch.nn.utils.weight_norm, dim 0
    # the folded weight is a float32 tensor on the device: the arbiter starts from the same numbers
    return w.to(torch.float32).to(dtype)


def generator(sd, mel, config, dtype=torch.float64):
    """mel (B, n_mel, T) -> (B, T * hop) in `dtype`; every utterance at full length T (run ragged batches one utterance at a time)."""
    with torch.no_grad():
        W = lambda n: _weight(sd, n, dtype)
        Bv = lambda n: torch.as_tensor(np.asarray(sd[n + ".bias"]), dtype=torch.float32).to(dtype)
        x = torch.as_tensor(np.asarray(mel, np.float32)).to(dtype)
        x = F.conv1d(x, W("conv_pre"), Bv("conv_pre"), padding=3)
        n_k = len(config["resblock_kernel_sizes"])
        for i, (r, ku) in enumerate(zip(config["upsample_rates"], config["upsample_kernel_sizes"])):
            x = F.leaky_relu(x, 0.1)
            x = F.conv_transpose1d(x, W(f"ups.{i}"), Bv(f"ups.{i}"), stride=r, padding=(ku - r) // 2)
            xs = None
            for j, k in enumerate(config["resblock_kernel_sizes"]):
                y = x
                for m, d in enumerate(config["resblock_dilation_sizes"][j]):
                    n1, n2 = f"resblocks.{i * n_k + j}.convs1.{m}", f"resblocks.{i * n_k + j}.convs2.{m}"
                    t = F.leaky_relu(y, 0.1)
                    t = F.conv1d(t, W(n1), Bv(n1), dilation=d, padding=d * (k - 1) // 2)
                    t = F.leaky_relu(t, 0.1)
                    t = F.conv1d(t, W(n2), Bv(n2), dilation=1, padding=(k - 1) // 2)
                    y = t + y
                xs = y if xs is None else xs + y
            x = xs / n_k
        x = F.leaky_relu(x, 0.01)
        x = F.conv1d(x, W("conv_post"), Bv("conv_post"), padding=3)
        return torch.tanh(x).squeeze(1).numpy()
