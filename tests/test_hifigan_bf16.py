"""The bf16-operand mode of the HiFi-GAN generator (include/mtts.h: mtts_hifigan_set_numerics / get_numerics / conv_bf16; csrc/hifigan.h:
hg_conv_direct_bf16_kernel, the bf16 GEMM family through the handle's GemmCtx) against tests/hifigan_bf16_oracle.py, the torch
restatement of the mode's definition.  Every case runs on the SIMT emulator (CPU suite) and again on the GPU.

Kernel level (one convolution, both routes of mtts_hifigan_conv_bf16): against the float64 convolution of the bf16-ROUNDED operands only
fp32 accumulation order is left, so the bound is tests/test_bf16_mode.py's fp32-roundoff one, err < 3e-6 sqrt(k C) max(1, max |want|), and
the unrounded float64 convolution must be more than 10x further away than that error (it really is bf16).

Network level: roundings are chaotic (a last-bit difference that crosses a bf16 boundary re-draws the next layer), so the measure is the
relative L2 error per utterance against the float64 rounded-operand oracle.  Gate: err_device <= 4 e32r, e32r = the float32
rounded-operand oracle's own relative L2 distance to the float64 one (4: the factor tests/test_hifigan.py grants another summation
order).  And it is the right definition: err_device < half the distance between the rounded and the unrounded float64 oracles, and the
same handle in fp32 mode is more than twice as far from the rounded oracle as in bf16 mode.

The measured figures are in test_network_vs_rounded_oracle's docstring."""
import ctypes as C

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from meta_tts_amd import hifigan as H
from meta_tts_amd.engine import MttsError

import hifigan_bf16_oracle as BO
import hifigan_oracle as HO

# CFG_B of tests/test_hifigan.py restated: initial channels 128, rates [2, 2] -> stages of 64 and 32 channels
CFG_B = {"resblock": "1", "upsample_rates": [2, 2], "upsample_kernel_sizes": [4, 4], "upsample_initial_channel": 128,
         "resblock_kernel_sizes": [3, 11], "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5]]}
# initial channels 256, rates [2] -> one stage of 128 channels (the widest instance of the direct bf16 kernel), with CFG_B's blocks.
# The blocks are three pairs deep on purpose.  A network error here is made of discrete events — an element that lands on the other side
# of a bf16 boundary (2^-8 of one element: ~2e-5 of an utterance's L2 norm) and the cascade it starts in the layers behind it.  Six
# convolutions behind one another bring that cascade to its floor (1e-4 .. 5e-4 for both the float32 oracle and the device); with blocks
# two pairs deep ([[1, 5], [3, 1]]) a run holds a handful of events and e32r is a lottery ticket, not a yardstick: the float32 oracle
# ALONE moved from 2.4e-5 to 1.2e-4 on the same utterance from one CPU to another (the device stood at 4.8e-5 and 1.1e-4 beside them).
CFG_C = {"resblock": "1", "upsample_rates": [2], "upsample_kernel_sizes": [4], "upsample_initial_channel": 256,
         "resblock_kernel_sizes": [3, 11], "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5]]}
N_MEL = 16
NET = {"B": (CFG_B, 4, (33, 7)), "C": (CFG_C, 2, (33, 7))}   # name -> (config, hop, mel lengths)
LENS = NET["B"][2]   # (the tests that run configuration B only)


@pytest.fixture(scope="module", params=[pytest.param(False, id="emu"), pytest.param(True, id="gpu", marks=pytest.mark.gpu)])
def lib_path(request):
    """None: libmtts.so on the GPU; else the emulator build of the same sources."""
    if request.param:
        ge.build_device()
        return None
    return ge.build_emulator()


def _mel(seed, B, T, n_mel):
    g = np.random.RandomState(seed)
    return (g.standard_normal((B, n_mel, T)) * 1.5 - 4.0).astype(np.float32)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


_CASE = {}


def _case(name):
    """(state dict, mel, [(float64 rounded oracle, e32r, rounded-vs-unrounded distance)] per utterance alone); computed once, read-only."""
    if name not in _CASE:
        cfg, _, LENS = NET[name]
        sd, mel = H.synthetic_state_dict(5, cfg, N_MEL), _mel(1, 2, max(LENS), N_MEL)
        refs = []
        for b, L in enumerate(LENS):
            m = mel[b:b + 1, :, :L]
            r64 = BO.generator(sd, m, cfg, torch.float64)[0]
            r32 = BO.generator(sd, m, cfg, torch.float32)[0]
            u64 = BO.generator(sd, m, cfg, torch.float64, round_operands=False)[0]
            assert r64.std() > 0.05 and (np.abs(r64) < 0.999).mean() >= 0.99, (name, b, r64.std())   # not a hollow comparison
            r64.setflags(write=False)
            refs.append((r64, _rel(r32, r64), _rel(u64, r64)))
        _CASE[name] = (sd, mel, refs)
    return _CASE[name]


# ---- oracle (CPU) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["B", "C"])
def test_oracle_without_rounding_is_the_fp32_oracle_and_has_room(name):
    cfg, _, LENS = NET[name]
    sd, mel, refs = _case(name)
    for b, L in enumerate(LENS):
        m = mel[b:b + 1, :, :L]
        a = BO.generator(sd, m, cfg, torch.float64, round_operands=False)
        assert np.abs(a - HO.generator(sd, m, cfg, torch.float64)).max() <= 1e-12
        _, e32r, dist = refs[b]
        print(f"{name} utterance {b}: e32r {e32r:.3e}  rounded-vs-unrounded {dist:.3e}")
        assert 2.0 * e32r < 0.5 * dist, (name, b, e32r, dist)   # room to spare under the "right definition" bound (half the distance)


def test_conv_rows_is_the_generators_convolution():
    """The kernel-level oracle and the network oracle state the same convolution (weight image [C][k][C] = weight.transpose(0, 2, 1))."""
    g = np.random.RandomState(0)
    x, w, bias = g.standard_normal((1, 9, 32)).astype(np.float32), g.standard_normal((32, 3, 32)).astype(np.float32), g.standard_normal(32).astype(np.float32)
    got = BO.conv_rows(x, (9,), w, bias, 3, 2, in_slope=0.1)
    t = BO.bf16_round(torch.nn.functional.leaky_relu(torch.from_numpy(x[0].T[None]), 0.1)).double()
    want = torch.nn.functional.conv1d(t, BO.bf16_round(torch.from_numpy(w.transpose(0, 2, 1).copy())).double(), torch.from_numpy(bias).double(), dilation=2, padding=2)
    assert np.abs(got[0] - want[0].T.numpy()).max() < 1e-12


# ---- kernel level ---------------------------------------------------------------------------------------------------------------------
K_LENS, K_T = (130, 5), 130   # 130: a second, nearly empty 128-row tile; 5: shorter than the halo, zeros enter on both sides
SENTINEL = 7.0


@pytest.fixture(scope="module")
def handle(lib_path):
    voc = H.HiFiGAN(None, CFG_B, n_mel=N_MEL, max_B=2, max_T=8, lib_path=lib_path)   # any handle: the entry brings its own operands
    yield voc
    voc.close()


def _conv_case(C_, k, d, in_slope):
    g = np.random.RandomState(1000 * C_ + 10 * k + d)
    x = g.standard_normal((2, K_T, C_)).astype(np.float32)
    w = (g.standard_normal((C_, k, C_)) / np.sqrt(k * C_)).astype(np.float32)
    bias = g.standard_normal(C_).astype(np.float32)
    res, mrf0 = g.standard_normal(x.shape).astype(np.float32), g.standard_normal(x.shape).astype(np.float32)
    want = BO.conv_rows(x, K_LENS, w, bias, k, d, in_slope)
    full = BO.conv_rows(x, K_LENS, w, bias, k, d, in_slope, round_operands=False)
    return x, w, bias, res, mrf0, want, full


def _check_conv(got, want, full, C_, k):
    for b, L in enumerate(K_LENS):
        assert np.all(got[b, L:] == SENTINEL), "rows beyond lens were written"
    v = np.concatenate([np.arange(L) + b * K_T for b, L in enumerate(K_LENS)])
    g, w_, f = (a.reshape(-1, C_)[v].astype(np.float64) for a in (got, want, full))
    err = np.abs(g - w_).max()
    bound = 3e-6 * np.sqrt(k * C_) * max(1.0, np.abs(w_).max())
    print(f"C {C_} k {k}: error {err:.3e}  bound {bound:.3e}  distance to the unrounded convolution {np.abs(g - f).max():.3e}")
    assert err < bound, (err, bound)                 # fp32 accumulation only: NOT a bf16-sized error
    assert np.abs(g - f).max() > 10 * err            # and it is not the fp32 product


@pytest.mark.parametrize("route", [0, 1])
@pytest.mark.parametrize("k,d", [(3, 1), (7, 3), (11, 5)])
@pytest.mark.parametrize("C_", [32, 64, 128])
def test_conv_bf16_vs_rounded_operands(handle, C_, k, d, route):
    x, w, bias, _, _, want, full = _conv_case(C_, k, d, 0.1)
    out = np.full(x.shape, SENTINEL, np.float32)
    got = handle.conv_bf16(x, K_LENS, w, bias, k, d, in_slope=0.1, epilogue=0, out=out, route=route)
    lr = lambda a: np.where(a > 0, a, np.float32(0.1).astype(np.float64) * a)
    # the epilogue's LeakyReLU is fp32 work on the sum: compare behind it, at its Lipschitz constant 1
    _check_conv(got, lr(want), lr(full), C_, k)


@pytest.mark.parametrize("route", [0, 1])
@pytest.mark.parametrize("epilogue,mrf_init", [(1, 0), (2, 0), (2, 1)])
def test_conv_bf16_epilogues(handle, epilogue, mrf_init, route):
    C_, k, d = 64, 7, 3
    x, w, bias, res, mrf0, want, full = _conv_case(C_, k, d, 1.0)
    inv_nk = 0.5
    if epilogue == 1:
        out = np.full(x.shape, SENTINEL, np.float32)
        got = handle.conv_bf16(x, K_LENS, w, bias, k, d, epilogue=1, res=res, out=out, route=route)
        fin = lambda a: a + res
    else:
        mrf = mrf0.copy()
        for b, L in enumerate(K_LENS):
            mrf[b, L:] = SENTINEL
        base = 0.0 if mrf_init else mrf0.astype(np.float64)
        got = handle.conv_bf16(x, K_LENS, w, bias, k, d, epilogue=2, res=res, mrf=mrf, inv_nk=inv_nk, mrf_init=mrf_init, route=route)
        fin = lambda a: base + inv_nk * (a + res)
    _check_conv(got, fin(want), fin(full), C_, k)


# ---- network level --------------------------------------------------------------------------------------------------------------------
def _voc(name, lib_path, numerics="bf16", dm=0, sd=None):
    cfg, _, LENS = NET[name]
    return H.HiFiGAN(_case(name)[0] if sd is None else sd, cfg, n_mel=N_MEL, max_B=2, max_T=max(NET[name][2]), lib_path=lib_path, direct_max_channels=dm, numerics=numerics)


@pytest.mark.parametrize("name,dm", [("B", 0), ("B", 64), ("C", 128)])
def test_network_vs_rounded_oracle(lib_path, name, dm):
    """Measured, relative L2 per utterance (33 frames; 7 frames): e32r / bf16 device error / fp32-mode and rounded-vs-unrounded distance
        MI355X    B, dm 0 and 64:  4.561e-04 / 4.941e-04 / 2.092e-03;   1.625e-07 / 7.109e-08 / 2.677e-03
        MI355X    C, dm 128:       7.963e-05 / 1.686e-04 / 1.293e-03;   2.563e-04 / 1.906e-04 / 1.625e-03
        emulator  B, dm 0 and 64:  4.539e-04 / 4.286e-04 / 2.092e-03;   1.509e-07 / 1.444e-07 / 2.677e-03
        emulator  C, dm 128:       2.014e-04 / 1.260e-04 / 1.293e-03;   1.941e-04 / 1.385e-04 / 1.625e-03
    (e32r is the float32 torch oracle on the host of each run: it differs between hosts, see the note at CFG_C)."""
    _, hop, LENS = NET[name]
    sd, mel, refs = _case(name)
    voc = _voc(name, lib_path, "bf16", dm)
    assert voc.numerics == "bf16" and voc.direct_max_channels == dm
    lens = np.array(LENS, np.int32)
    wav = voc.mel2wav(mel, lens)
    voc.set_numerics("fp32", min(dm, 64))
    wav32 = voc.mel2wav(mel, lens)
    voc.close()
    for b, (r64, e32r, dist) in enumerate(refs):
        n = LENS[b] * hop
        err, err32 = _rel(wav[b, :n], r64), _rel(wav32[b, :n], r64)
        print(f"{name} dm {dm} utterance {b}: e32r {e32r:.3e}  device {err:.3e}  gate {4 * e32r:.3e}  fp32 mode {err32:.3e}  rounded-vs-unrounded {dist:.3e}")
        assert err <= 4.0 * e32r, (name, dm, b, err, e32r)
        assert err < 0.5 * dist and err32 > 2.0 * err, (name, dm, b, err, err32, dist)
        assert np.all(wav[b, n:] == 0)


# ---- bit for bit, in bf16 mode ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dm", [("B", 0), ("B", 64), ("C", 128)])
def test_alone_equals_batch_and_device_entry_equals_host_entry(lib_path, name, dm):
    _, hop, LENS = NET[name]
    _, mel, _ = _case(name)
    voc = _voc(name, lib_path, "bf16", dm)
    lens = np.array(LENS, np.int32)
    wav = voc.mel2wav(mel, lens)
    for b, L in enumerate(LENS):
        alone = voc.mel2wav(mel[b:b + 1, :, :L])
        np.testing.assert_array_equal(alone[0], wav[b, :L * hop])
    x, T_MEL = np.ascontiguousarray(mel.transpose(0, 2, 1)), max(LENS)
    if lib_path is None:
        xd, outd = torch.from_numpy(x).cuda(), torch.zeros(2, T_MEL * hop, device="cuda")
        voc.set_stream(torch.cuda.current_stream().cuda_stream)
        voc.mel2wav_device(xd.data_ptr(), 0, 2, T_MEL, lens, outd.data_ptr())
        torch.cuda.synchronize()
        got = outd.cpu().numpy()
    else:   # the emulator's device memory is host memory
        got = np.zeros((2, T_MEL * hop), np.float32)
        voc.mel2wav_device(x.ctypes.data, 0, 2, T_MEL, lens, got.ctypes.data)
    for b, L in enumerate(LENS):
        np.testing.assert_array_equal(got[b, :L * hop], wav[b, :L * hop])
    voc.close()


@pytest.mark.parametrize("d", [0, 64])
def test_back_to_fp32_is_bit_for_bit(lib_path, d):
    _, mel, _ = _case("B")
    voc = _voc("B", lib_path, "fp32", d)
    lens = np.array(LENS, np.int32)
    assert voc.numerics == "fp32"
    before = voc.mel2wav(mel, lens)
    voc.set_numerics("bf16", 64)
    assert voc.numerics == "bf16"
    mid = voc.mel2wav(mel, lens)
    assert not np.array_equal(mid, before)
    voc.set_numerics(0, d)
    assert voc.numerics == "fp32"
    np.testing.assert_array_equal(voc.mel2wav(mel, lens), before)
    voc.close()


@pytest.mark.parametrize("dm", [0, 64])
def test_tensor_loaded_after_the_mode_takes_effect(lib_path, dm):
    cfg, _, LENS = NET["B"]
    sd, mel, _ = _case("B")
    lens = np.array(LENS, np.int32)
    name = "resblocks.1.convs1.2"   # a 64-channel residual convolution: the direct route reads its packed image
    new = dict(sd)
    new[name + ".weight_v"] = np.random.RandomState(9).standard_normal(sd[name + ".weight_v"].shape).astype(np.float32)
    packed = H.pack_tensors(new, cfg, N_MEL)[name + ".w"]
    voc = _voc("B", lib_path, "bf16", dm)
    first = voc.mel2wav(mel, lens)
    voc.load(name + ".w", packed)                   # after the mode was set
    second = voc.mel2wav(mel, lens)
    voc.close()
    assert not np.array_equal(first, second)
    fresh = _voc("B", lib_path, "fp32", 0, sd=new)  # loaded first, mode set afterwards
    fresh.set_numerics("bf16", dm)
    np.testing.assert_array_equal(fresh.mel2wav(mel, lens), second)
    fresh.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_set_numerics_refusals_and_get(lib_path):
    _, mel, _ = _case("B")
    voc = _voc("B", lib_path, "fp32", 0)
    lens = np.array(LENS, np.int32)
    before = voc.mel2wav(mel, lens)
    for (mode, dm), word in (((2, 0), "mode"), ((0, 128), "direct_max_channels"), ((1, 48), "direct_max_channels")):
        assert voc.lib.mtts_hifigan_set_numerics(voc.h, mode, dm) != 0
        msg = voc.lib.mtts_hifigan_last_error(voc.h).decode()
        assert word in msg and str(dm if word != "mode" else mode) in msg, msg
        assert voc.lib.mtts_hifigan_get_numerics(voc.h) == 0 and voc.numerics == "fp32"
    with pytest.raises(MttsError, match="mode"):
        voc.set_numerics(2)
    with pytest.raises(MttsError, match="numerics"):
        H.HiFiGAN(None, CFG_B, n_mel=N_MEL, max_B=1, max_T=8, lib_path=lib_path, numerics="fp16")
    np.testing.assert_array_equal(voc.mel2wav(mel, lens), before)   # a refused call changed nothing
    for mode, dm in ((1, 128), (1, 0), (0, 64), (1, 32), (0, 0)):
        assert voc.lib.mtts_hifigan_set_numerics(voc.h, mode, dm) == 0
        assert voc.lib.mtts_hifigan_get_numerics(voc.h) == mode
    with pytest.raises(MttsError, match="C = 48"):
        voc.conv_bf16(np.zeros((1, 8, 48), np.float32), (8,), np.zeros((48, 3, 48), np.float32), np.zeros(48, np.float32), 3, 1, out=np.zeros((1, 8, 48), np.float32))
    voc.close()
