"""HiFi-GAN generator host layer: what stands behind the `name == "HiFi-GAN"` branch of the reference's `vocoder_infer`
(utils/model.py:32-50: `vocoder(mels).squeeze(1)`, x max_wav_value -> int16, cut to `lengths`).

Neither the generator's code nor a checkpoint (`generator_universal.pth.tar`) is part of the reference tree, so parity with published
weights is UNPINNED: this class takes a state dict in the published module's naming (`conv_pre`, `ups.{i}`,
`resblocks.{i*n_k+j}.convs1.{m}` / `convs2.{m}`, `conv_post`, each with `weight_g` / `weight_v` / `bias` or an already folded `weight`;
a `{"generator": sd}` wrapper is unwrapped) or synthetic weights, folds the weight normalisation and re-packs the ConvTranspose1d
kernels into the polyphase images `libmtts.so` consumes (include/mtts.h, mtts_hifigan_*).  `config` carries the keys of the published
json (`upsample_rates`, `upsample_kernel_sizes`, `upsample_initial_channel`, `resblock_kernel_sizes`, `resblock_dilation_sizes`,
`resblock`); only ResBlock type "1" is built (V1, V2), V3 is refused.
"""
from __future__ import annotations

import ctypes as C
import math
import zlib

import numpy as np

from . import _lib
from .engine import MttsError
from .vocoder import WaveGenerator, fold_weight_norm, polyphase_image

V1 = {"resblock": "1", "upsample_rates": [8, 8, 2, 2], "upsample_kernel_sizes": [16, 16, 4, 4], "upsample_initial_channel": 512,
      "resblock_kernel_sizes": [3, 7, 11], "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5], [1, 3, 5]]}
V2 = dict(V1, upsample_initial_channel=128)
V3 = {"resblock": "2", "upsample_rates": [8, 8, 4], "upsample_kernel_sizes": [16, 16, 8], "upsample_initial_channel": 256,
      "resblock_kernel_sizes": [3, 5, 7], "resblock_dilation_sizes": [[1, 2], [2, 6], [3, 12]]}

# `direct_max_channels` of a HiFiGAN built without one: 0 (GEMM route everywhere) until both routes have been timed in one session
# (tools/hifigan_bench.py; README "HiFi-GAN generator").
DEFAULT_DIRECT_MAX_CHANNELS = 0
# the same rule for the bf16-operand mode: legs (e) / (f) of tools/hifigan_bench.py were timed in one session, 8.78 against 6.18 ms with
# spreads of 0.05 ms, so the direct route is the bf16 mode's default
DEFAULT_DIRECT_MAX_CHANNELS_BF16 = 128
NUMERICS = {"fp32": 0, "bf16": 1}


def _check(config):
    """The refusals that can be decided on the host before anything is created; the rest is mtts_hifigan_create's."""
    if str(config["resblock"]) != "1":
        raise MttsError(f"HiFiGAN: resblock {config['resblock']!r} is not supported (only ResBlock \"1\": V1 / V2)")
    rates, ks = list(config["upsample_rates"]), list(config["upsample_kernel_sizes"])
    if len(rates) != len(ks):
        raise MttsError("HiFiGAN: upsample_kernel_sizes and upsample_rates differ in length")
    for i, (r, k) in enumerate(zip(rates, ks)):
        if r < 2 or r % 2:
            raise MttsError(f"HiFiGAN: upsample_rates[{i}] = {r}: every rate must be even and >= 2")
        if k != 2 * r:
            raise MttsError(f"HiFiGAN: upsample_kernel_sizes[{i}] = {k} is not 2 * upsample_rates[{i}] = {2 * r}")
    dil = [list(d) for d in config["resblock_dilation_sizes"]]
    if len(dil) != len(config["resblock_kernel_sizes"]) or len({len(d) for d in dil}) != 1:
        raise MttsError("HiFiGAN: resblock_dilation_sizes must give one equally long list per resblock_kernel_sizes entry")


def generator_spec(config=V1, n_mel=80):
    """[(published name prefix, kind, shape of weight_v)] in the order of the library's tensor table (a block's pairs convs1.m, convs2.m
    one after another); kinds: conv / convT."""
    _check(config)
    c = int(config["upsample_initial_channel"])
    n_k = len(config["resblock_kernel_sizes"])
    spec = [("conv_pre", "conv", (c, n_mel, 7))]
    for i, r in enumerate(config["upsample_rates"]):
        spec.append((f"ups.{i}", "convT", (c, c // 2, 2 * r)))
        c //= 2
        for j, k in enumerate(config["resblock_kernel_sizes"]):
            for m in range(len(config["resblock_dilation_sizes"][j])):
                for half in (1, 2):
                    spec.append((f"resblocks.{i * n_k + j}.convs{half}.{m}", "conv", (c, c, k)))
    spec.append(("conv_post", "conv", (1, c, 7)))
    return spec


def synthetic_state_dict(seed=0, config=V1, n_mel=80):
    """Deterministic weights in the published naming (weight_g / weight_v / bias).  The gains keep activations O(1) through all blocks,
    by the reasoning of `vocoder.synthetic_state_dict`: a weight-normed conv output has variance g^2 per unit second moment of its input.
    LeakyReLU(0.1) halves the second moment (0.505), so convs1 and the transposed convolutions carry sqrt(2) (the latter times MelGAN's
    sqrt(r C_out / C_in)); convs2 — the residual branch — carries 1/2, so a pair adds 0.125 to a unit variance and three pairs leave
    `t + x` under 1.4; conv_pre takes natural-log mels (second moment ~ 18 for the tests' mels): 1/4; conv_post 1/2 keeps tanh out of
    saturation."""
    sd = {}
    for name, kind, shape in generator_spec(config, n_mel):
        g = np.random.RandomState((zlib.crc32(name.encode()) ^ seed) & 0x7FFFFFFF)
        v = g.standard_normal(shape).astype(np.float32)
        if kind == "convT":
            gain, nb = math.sqrt(2.0 * (shape[2] // 2) * shape[1] / shape[0]), shape[1]
        else:
            nb = shape[0]
            gain = 0.25 if name == "conv_pre" else 0.5 if (name == "conv_post" or ".convs2." in name) else math.sqrt(2.0)
        sd[name + ".weight_v"] = v
        sd[name + ".weight_g"] = np.full((shape[0], 1, 1), gain, np.float32)
        sd[name + ".bias"] = (0.05 * g.standard_normal(nb)).astype(np.float32)
    return sd


def pack_tensors(sd, config=V1, n_mel=80):
    """published-style state dict -> {libmtts tensor name: float32 array} (layouts documented in include/mtts.h)."""
    if "generator" in sd and "conv_pre.bias" not in sd:
        sd = sd["generator"]
    sd = {k: (v.detach().cpu().numpy() if hasattr(v, "detach") else v) for k, v in sd.items()}
    out = {}
    for name, kind, shape in generator_spec(config, n_mel):
        w = fold_weight_norm(sd, name)
        if tuple(w.shape) != tuple(shape):
            raise MttsError(f"HiFiGAN: {name} has shape {tuple(w.shape)}, the config asks for {tuple(shape)}")
        if kind == "convT":
            out[name + ".w"] = polyphase_image(w)
        elif name == "conv_post":
            out[name + ".w"] = np.ascontiguousarray(w[0].T)                     # [7][C_last]
        else:
            out[name + ".w"] = np.ascontiguousarray(w.transpose(0, 2, 1))       # [C_out][k][C_in]
        out[name + ".b"] = np.asarray(sd[name + ".bias"], np.float32).reshape(-1)
    return out


class HiFiGAN(WaveGenerator):
    """The reference's HiFi-GAN vocoder object with `vocoder.MelGAN`'s duck type: `__call__(mels)` is the reference branch's call,
    `infer(mels, max_wav_value, lengths)` is `vocoder_infer`; mel (B, n_mel, T), natural-log mels as the model makes them and as the
    generator takes them (mel scale 1)."""
    _prefix = "mtts_hifigan_"

    def __init__(self, state_dict=None, config=V1, n_mel=80, max_B=8, max_T=1024, device=0, lib_path=None, direct_max_channels=None,
                 numerics="fp32"):
        _check(config)
        if numerics not in NUMERICS:
            raise MttsError(f"HiFiGAN: numerics {numerics!r} is not one of {sorted(NUMERICS)}")
        self.lib = _lib.load(lib_path)
        self.config, self.n_mel = config, n_mel
        self.max_B, self.max_T = max_B, max_T
        self.device, self.stream, self._wav_dev = device, 0, None
        requested = direct_max_channels
        if numerics == "bf16":   # the handle is created in fp32 (the C entry's only mode) and switched below
            direct_max_channels = 0
        self.direct_max_channels = DEFAULT_DIRECT_MAX_CHANNELS if direct_max_channels is None else int(direct_max_channels)
        rates = [int(r) for r in config["upsample_rates"]]
        kernels = [int(k) for k in config["resblock_kernel_sizes"]]
        dil = [[int(d) for d in row] for row in config["resblock_dilation_sizes"]]
        flat = [d for row in dil for d in row]
        h = C.c_void_p()
        self.h = None
        if self.lib.mtts_hifigan_create(n_mel, int(config["upsample_initial_channel"]), (C.c_int * len(rates))(*rates), len(rates),
                                        (C.c_int * len(kernels))(*kernels), len(kernels), (C.c_int * len(flat))(*flat), len(dil[0]),
                                        int(config["resblock"]), self.direct_max_channels, device, max_B, max_T, C.byref(h)) != 0:
            raise MttsError(self.lib.mtts_hifigan_last_error(None).decode())
        self.h = h
        self.hop = self.lib.mtts_hifigan_hop(h)
        sd = state_dict if state_dict is not None else synthetic_state_dict(0, config, n_mel)
        self.state_dict_ = sd
        try:
            for k, v in pack_tensors(sd, config, n_mel).items():
                self.load(k, v)
            if numerics != "fp32":
                self.set_numerics(numerics, requested)
        except Exception:
            self.close()
            raise

    @property
    def numerics(self):
        """"fp32" or "bf16": the mode in force (include/mtts.h: mtts_hifigan_set_numerics)."""
        mode = self.lib.mtts_hifigan_get_numerics(self.h)
        return next(k for k, v in NUMERICS.items() if v == mode)

    def set_numerics(self, mode, direct_max_channels=None):
        """mode "fp32" / "bf16" (or 0 / 1); direct_max_channels None: the mode's default.  Takes effect at the next call; tensors loaded
        later are re-packed by the library."""
        m = NUMERICS.get(mode, mode)
        if isinstance(m, bool) or not isinstance(m, (int, np.integer)):
            raise MttsError(f"HiFiGAN.set_numerics: mode {mode!r} is not one of {sorted(NUMERICS)}")
        if direct_max_channels is None:
            direct_max_channels = DEFAULT_DIRECT_MAX_CHANNELS_BF16 if m == 1 else DEFAULT_DIRECT_MAX_CHANNELS
        if self.lib.mtts_hifigan_set_numerics(self.h, int(m), int(direct_max_channels)) != 0:
            raise MttsError(self.lib.mtts_hifigan_last_error(self.h).decode())
        self.direct_max_channels = int(direct_max_channels)

    def conv_bf16(self, x, lens, w, bias, k, d, in_slope=1.0, epilogue=0, res=None, mrf=None, inv_nk=1.0, mrf_init=0, out=None, route=0):
        """Kernel-level entry (mtts_hifigan_conv_bf16): one convolution of the bf16 mode on host arrays x [B][T][C], w [C][k][C].
        Returns `out` (epilogues 0, 1) or `mrf` (epilogue 2), which must be C-contiguous float32 arrays and are written in place."""
        x = np.ascontiguousarray(x, np.float32)
        B, T, Cc = x.shape
        lens = np.ascontiguousarray(lens, np.int32)
        w, bias = np.ascontiguousarray(w, np.float32), np.ascontiguousarray(bias, np.float32)
        assert w.shape == (Cc, k, Cc) and bias.shape == (Cc,) and lens.shape == (B,)
        res = None if res is None else np.ascontiguousarray(res, np.float32)
        for a in (out, mrf):
            assert a is None or (a.dtype == np.float32 and a.flags.c_contiguous and a.shape == x.shape)
        P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        if self.lib.mtts_hifigan_conv_bf16(self.h, route, Cc, k, d, B, T, P(lens), P(x), P(w), P(bias), C.c_float(in_slope), epilogue, P(res),
                                           P(mrf), C.c_float(inv_nk), mrf_init, P(out)) != 0:
            raise MttsError(self.lib.mtts_hifigan_last_error(self.h).decode())
        return mrf if epilogue == 2 else out

    def __call__(self, mels):                      # utils/model.py:38: vocoder(mels) -> (B, 1, T * hop)
        return self.mel2wav(mels)[:, None, :]
