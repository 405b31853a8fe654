"""Shared helpers for tests that drive the oracle (tests/ may import oracle/, the product may not)."""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from meta_tts_amd import synth  # noqa: E402
from meta_tts_amd.config import ModelDims  # noqa: E402
from oracle import fs2_oracle as O  # noqa: E402

SMALL = dict(s_range=(6, 13), d_range=(1, 7), first_len=12)


def c5_edit(params):
    """Duration predictor giving LibriTTS-like durations at random init (tests/golden/make_golden.py: c5_edit; bench.py)."""
    params["variance_adaptor.duration_predictor.linear_layer.bias"][:] = np.log(8.0)
    params["variance_adaptor.duration_predictor.linear_layer.weight"] *= 0.25
    return params


def torch_params(dims, seed=0, requires_grad=False, weight_scale=1.0, edit=None):
    np_params = synth.make_params(dims, seed, weight_scale=weight_scale)
    if edit:
        edit(np_params)
    p = {k: torch.from_numpy(v.copy()) for k, v in np_params.items()}
    if requires_grad:
        frozen = ("position_enc", "pitch_bins", "energy_bins")
        for k, v in p.items():
            if not k.endswith(frozen):
                v.requires_grad_(True)
    return p


def torch_buffers(dims):
    return {k: torch.from_numpy(v.copy()) for k, v in synth.make_buffers(dims).items()}


def heads(dims):
    return (dims.enc_heads, dims.dec_heads)


def tiny_dims(**over):
    """A small architecture for kernel-logic tests (same code paths, tiny GEMMs)."""
    from meta_tts_amd.config import default_model_config, default_preprocess_config
    mc = default_model_config()
    mc["transformer"].update(dict(encoder_layer=1, decoder_layer=2, encoder_hidden=32, decoder_hidden=32,
                                  conv_filter_size=64, encoder_head=2, decoder_head=2))
    mc["variance_predictor"].update(dict(filter_size=32))
    mc["variance_embedding"]["n_bins"] = 16
    mc["max_seq_len"] = 64
    mc["_postnet_dim"] = 48
    pc = default_preprocess_config()
    pc["preprocessing"]["mel"]["n_mel_channels"] = 32
    pc["preprocessing"]["pitch"]["feature"] = over.pop("pitch_level", "phoneme_level")
    pc["preprocessing"]["energy"]["feature"] = over.pop("energy_level", "phoneme_level")
    mc.update(over.pop("model", {}))
    return ModelDims(mc, pc, n_speaker=over.pop("n_speaker", 12), vocab=over.pop("vocab", 40))


def check_grads(pairs, rtol, arbitrate, atol=0.0, label=""):
    """Gradient parity on a piecewise-smooth loss without an escape hatch.  `pairs`: {tensor name: (engine gradient, fp32-oracle gradient)}.
    A tensor passes when max |got - ref| <= rtol * max |ref| + atol (it agrees tightly with an independent fp32 implementation).  Every tensor
    that does not is handed to the float64 arbiter (`arbitrate(names)` -> oracle/arbiter.py report with both parties): it must pass
    err(engine, fp64) <= 3 * err(oracle32, fp64) + 1e-3 there, where L1 sign flips are read off each party's own forward output and ReLU flips are
    identified unit by unit — a ReLU / L1 kink inside fp32 noise is explained exactly, anything else fails.  Returns the arbiter's report (or None)."""
    failing = [n for n, (got, ref) in pairs.items() if float(np.abs(got - ref).max()) > rtol * float(np.abs(ref).max()) + atol]
    if not failing:
        return None
    rep = arbitrate(failing)
    bad = {n: rep["tensors"][n] for n in failing if not rep["tensors"][n]["ok"]}
    assert not bad, (label, bad, rep["parties"])
    return rep


class Dev:
    """Device-or-host buffers behind one interface: torch CUDA tensors on the GPU, numpy arrays for the emulator (whose 'device'
    memory is host memory)."""

    def __init__(self, gpu):
        import __graft_entry__ as ge
        from meta_tts_amd import _lib
        self.gpu = gpu
        self.lib = _lib.load(None if gpu else ge.build_emulator())
        self.keep = []

    def put(self, a):
        a = np.ascontiguousarray(a)
        if self.gpu:
            t = torch.from_numpy(a).cuda()
            self.keep.append(t)
            return t
        self.keep.append(a)
        return a

    def empty(self, shape, dtype=np.float32, fill=0):
        return self.put(np.full(shape, fill, dtype))

    def ptr(self, x):
        if x is None:
            return None
        return C.c_void_p(x.data_ptr()) if self.gpu else x.ctypes.data_as(C.c_void_p)

    def get(self, x):
        if self.gpu:
            torch.cuda.synchronize()
            return x.cpu().numpy()
        return x

    def ws(self, rows, n_mat=0):
        return self.empty((int(self.lib.mtts_kernel_ws_bytes(rows, n_mat)) + 3) // 4, np.float32)
