"""HiFi-GAN generator (csrc/hifigan.h through include/mtts.h: mtts_hifigan_*; meta_tts_amd/hifigan.py) against tests/hifigan_oracle.py,
the torch restatement of the definition in include/mtts.h (parity with published weights is UNPINNED: neither the generator's code nor a
checkpoint is in the reference tree).  Host packing and both routes of the residual convolutions (grouped GEMM, direct MFMA kernel)
through the SIMT emulator on the CPU, the real kernels on the GPU.

Tolerance: for each compared waveform e32 = max |float32 oracle - float64 oracle|; the device must stay within max(4 * e32, 2e-5) of the
float64 oracle (4: another summation order — MFMA tiles, per-tap accumulation; 2e-5: the MelGAN gate of tests/test_vocoder.py); int16
output within 2 LSB.  Every compared float64 waveform must have standard deviation > 0.05 and |w| < 0.999 on >= 99 % of its samples, so
that the comparison is not hollow."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from meta_tts_amd import hifigan as H
from meta_tts_amd.engine import MttsError

import hifigan_oracle as HO

CFG_A = {"resblock": "1", "upsample_rates": [4, 2], "upsample_kernel_sizes": [8, 4], "upsample_initial_channel": 64,
         "resblock_kernel_sizes": [3, 7], "resblock_dilation_sizes": [[1, 3], [1, 5]]}          # channels 32, 16
CFG_B = {"resblock": "1", "upsample_rates": [2, 2], "upsample_kernel_sizes": [4, 4], "upsample_initial_channel": 128,
         "resblock_kernel_sizes": [3, 11], "resblock_dilation_sizes": [[1, 3, 5], [1, 3, 5]]}   # channels 64, 32


@pytest.fixture(scope="module")
def emu_lib():
    return ge.build_emulator()


def _mel(seed, B, T, n_mel):
    g = np.random.RandomState(seed)
    return (g.standard_normal((B, n_mel, T)) * 1.5 - 4.0).astype(np.float32)


_REFS = {}


def _refs(key, sd, mel, lens, config):
    """[(float64 oracle, e32)] per utterance, each run alone at its own length; computed once per case and shared."""
    if key not in _REFS:
        out = []
        for b, L in enumerate(lens):
            r64 = HO.generator(sd, mel[b:b + 1, :, :L], config, torch.float64)[0]
            r32 = HO.generator(sd, mel[b:b + 1, :, :L], config, torch.float32)[0]
            assert r64.std() > 0.05 and (np.abs(r64) < 0.999).mean() >= 0.99, (key, b, r64.std())   # precondition on the inputs
            r64.setflags(write=False)
            out.append((r64, float(np.abs(r32.astype(np.float64) - r64).max())))
        _REFS[key] = out
    return _REFS[key]


def _check_against_oracle(key, wav, sd, mel, lens, config, hop):
    for b, (r64, e32) in enumerate(_refs(key, sd, mel, lens, config)):
        n = lens[b] * hop
        err = float(np.abs(wav[b, :n].astype(np.float64) - r64).max())
        gate = max(4.0 * e32, 2e-5)
        print(f"{key} utterance {b}: e32 {e32:.3e}  device error {err:.3e}  gate {gate:.3e}")
        assert err <= gate, (key, b, err, e32)
        assert np.all(wav[b, n:] == 0)


# ---- 1. spec ---------------------------------------------------------------------------------------------------------------------
def test_v1_spec_names_shapes_and_parameter_count(emu_lib):
    sd = H.synthetic_state_dict(0)
    for name, shape in (("conv_pre", (512, 80, 7)), ("ups.0", (512, 256, 16)), ("resblocks.0.convs1.2", (256, 256, 3)),
                        ("resblocks.11.convs1.0", (32, 32, 11)), ("conv_post", (1, 32, 7))):
        assert sd[name + ".weight_v"].shape == shape, name
    spec = H.generator_spec(H.V1)
    assert sorted((n, s) for n, _, s in spec) == sorted(HO.tensor_list(H.V1, 80)) and len(spec) == 78
    n_weights = sum(int(np.prod(s)) for _, s in HO.tensor_list(H.V1, 80))
    n_bias = sum(s[1] if n.startswith("ups.") else s[0] for n, s in HO.tensor_list(H.V1, 80))
    packed = H.pack_tensors(sd)
    assert sum(v.size for v in packed.values()) == n_weights + n_bias
    assert 13_900_000 < n_weights + n_bias < 14_000_000   # the published V1 generator: 13.9 M parameters
    # the device's own table says the same
    voc = H.HiFiGAN(sd, max_B=1, max_T=4, lib_path=emu_lib)
    total, name, numel = 0, C.create_string_buffer(128), C.c_int64()
    for i in range(voc.lib.mtts_hifigan_param_count(voc.h)):
        assert voc.lib.mtts_hifigan_param_info(voc.h, i, name, 128, C.byref(numel)) == 0
        assert packed[name.value.decode()].size == numel.value
        total += numel.value
    assert total == n_weights + n_bias and voc.hop == 256
    voc.close()


def test_polyphase_images_equal_conv_transpose():
    import torch.nn.functional as F
    cfg = {"resblock": "1", "upsample_rates": [4], "upsample_kernel_sizes": [8], "upsample_initial_channel": 32,
           "resblock_kernel_sizes": [3], "resblock_dilation_sizes": [[1]]}
    sd = H.synthetic_state_dict(3, cfg, 16)
    img = H.pack_tensors({"generator": sd}, cfg, 16)["ups.0.w"]          # (the checkpoint's wrapper is unwrapped)
    cin, cout, r, T = 32, 16, 4, 11
    assert img.shape == (r, cout, 2 * cin)
    w = H.fold_weight_norm(sd, "ups.0")
    x = np.random.RandomState(3).standard_normal((T, cin)).astype(np.float32)
    ref = F.conv_transpose1d(torch.from_numpy(x.T[None]), torch.from_numpy(w), stride=r, padding=r // 2).numpy()[0].T  # [rT][cout]
    p = r // 2
    xz = np.concatenate([np.zeros((1, cin), np.float32), x, np.zeros((1, cin), np.float32)])
    out = np.zeros((r * T, cout), np.float32)
    for ph in range(r):
        q0 = 0 if ph >= p else 1
        for m in range(T):
            q = q0 + m
            out[q * r + ph - p] = img[ph] @ np.concatenate([xz[q], xz[q + 1]])
    np.testing.assert_allclose(out, ref, rtol=1e-5, atol=1e-5)


# ---- 2. / 3. tiny configurations through the emulator ---------------------------------------------------------------------------------
def test_tiny_config_a_gemm_route_ragged(emu_lib):
    """Channels 32 and 16: the dilated-tap GEMM (C % 32 == 0) and the per-tap accumulate fallback both run."""
    sd = H.synthetic_state_dict(5, CFG_A, 16)
    voc = H.HiFiGAN(sd, CFG_A, n_mel=16, max_B=2, max_T=24, lib_path=emu_lib, direct_max_channels=0)
    mel, lens = _mel(1, 2, 20, 16), (20, 13)
    wav = voc.mel2wav(mel, np.array(lens, np.int32))
    assert wav.shape == (2, 20 * 8) and voc.hop == 8
    _check_against_oracle("A", wav, sd, mel, lens, CFG_A, 8)
    voc.close()


@pytest.mark.parametrize("direct_max", [0, 64])
def test_tiny_config_b_both_routes(emu_lib, direct_max):
    """Channels 64 and 32.  Length 4 gives 8 and 16 rows against a halo of 50: most of it lies outside the utterance; 33 frames give 132
    rows at the last stage, one tile of 128 and four rows."""
    sd = H.synthetic_state_dict(5, CFG_B, 16)
    voc = H.HiFiGAN(sd, CFG_B, n_mel=16, max_B=2, max_T=33, lib_path=emu_lib, direct_max_channels=direct_max)
    mel, lens = _mel(1, 2, 33, 16), (33, 4)
    wav = voc.mel2wav(mel, np.array(lens, np.int32))
    _check_against_oracle("B", wav, sd, mel, lens, CFG_B, 4)
    assert np.array_equal(wav, voc.mel2wav(mel, np.array(lens, np.int32)))   # run-to-run identical (no atomics)
    voc.close()


# ---- 4. infer / __call__ ---------------------------------------------------------------------------------------------------------------
def test_infer_and_call_follow_the_reference_branch(emu_lib):
    sd = H.synthetic_state_dict(5, CFG_A, 16)
    voc = H.HiFiGAN(sd, CFG_A, n_mel=16, max_B=2, max_T=24, lib_path=emu_lib)
    mel = _mel(1, 2, 20, 16)
    out = voc(mel)
    assert out.shape == (2, 1, 160) and out.dtype == np.float32
    r64 = HO.generator(sd, mel, CFG_A, torch.float64)
    i16 = voc.infer(mel, 32768.0, lengths=[160, 13 * 8 - 3])
    assert i16[0].dtype == np.int16 and len(i16[0]) == 160 and len(i16[1]) == 13 * 8 - 3
    ref0 = (r64[0] * 32768.0).astype("int16")
    assert np.abs(i16[0].astype(np.int32) - ref0.astype(np.int32)).max() <= 2
    ref1 = (HO.generator(sd, mel[1:, :, :13], CFG_A, torch.float64)[0] * 32768.0).astype("int16")[:13 * 8 - 3]
    assert np.abs(i16[1].astype(np.int32) - ref1.astype(np.int32)).max() <= 2
    full = voc.infer(mel, 32768.0)
    assert len(full) == 2 and all(len(w) == 160 and w.dtype == np.int16 for w in full)
    voc.close()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("change, word", [
    ({"upsample_kernel_sizes": [8, 6]}, "upsample_kernel_sizes"),
    ({"upsample_rates": [4, 3], "upsample_kernel_sizes": [8, 6]}, "upsample_rates"),
    ({"resblock": "2"}, "resblock"),
    ({"resblock_kernel_sizes": [3, 4]}, "res_kernels"),
    ({"resblock_dilation_sizes": [[1, 3], [1, 6]]}, "res_dilations"),
])
def test_unsupported_configurations_are_refused_at_create(emu_lib, change, word):
    cfg = dict(CFG_A, **change)
    with pytest.raises(MttsError, match=word):
        H.HiFiGAN(None, cfg, n_mel=16, max_B=2, max_T=24, lib_path=emu_lib)


def test_create_entry_refuses_by_itself(emu_lib):
    """The C entry's own validation (the host layer refuses some of these earlier): the message names the argument, nothing is created."""
    from meta_tts_amd import _lib
    lib = _lib.load(emu_lib)
    live = lib.emu_live_allocs
    live.restype = C.c_longlong
    base = live()

    def create(n_mel=16, c0=64, rates=(4, 2), kernels=(3, 7), dil=((1, 3), (1, 5)), rb=1, dm=0, max_B=2, max_T=24):
        h = C.c_void_p()
        flat = [d for row in dil for d in row]
        rc = lib.mtts_hifigan_create(n_mel, c0, (C.c_int * len(rates))(*rates), len(rates), (C.c_int * len(kernels))(*kernels), len(kernels),
                                     (C.c_int * len(flat))(*flat), len(dil[0]), rb, dm, 0, max_B, max_T, C.byref(h))
        return rc, h, lib.mtts_hifigan_last_error(None).decode()

    for kw, word in ((dict(rb=2), "resblock_type"), (dict(rates=(4, 3)), "rates[1]"), (dict(kernels=(3, 4)), "res_kernels[1]"),
                     (dict(dil=((1, 3), (1, 6))), "res_dilations[1][1]"), (dict(n_mel=20), "n_mel"), (dict(c0=96), "initial_channels"),
                     (dict(dm=48), "direct_max_channels"), (dict(max_T=3), "max_T"), (dict(kernels=(3, 13)), "res_kernels[1]")):
        rc, h, msg = create(**kw)
        assert rc != 0 and word in msg and live() == base, (kw, msg)
    rc, h, _ = create()
    assert rc == 0
    lib.mtts_hifigan_destroy(h)
    assert live() == base


def test_bad_batches_and_tensors_are_refused_without_a_launch(emu_lib):
    sd = H.synthetic_state_dict(5, CFG_A, 16)
    voc = H.HiFiGAN(sd, CFG_A, n_mel=16, max_B=2, max_T=24, lib_path=emu_lib)
    wav = np.full((3, 24 * 8), 7.0, np.float32)

    def call(B, T, lens):
        lens = np.asarray(lens, np.int32)
        x = np.zeros((B, T, 16), np.float32)
        rc = voc.lib.mtts_hifigan_infer(voc.h, x.ctypes.data_as(C.c_void_p), B, T, lens.ctypes.data_as(C.c_void_p), C.c_float(1.0), wav.ctypes.data_as(C.c_void_p))
        return rc, voc.lib.mtts_hifigan_last_error(voc.h).decode()

    for args, word in (((1, 3, [3]), "T_max"), ((2, 20, [20, 21]), "mel_lens[1]"), ((2, 20, [3, 20]), "mel_lens[0]"), ((3, 20, [20, 20, 20]), "max_B"),
                       ((1, 25, [25]), "T_max")):
        rc, msg = call(*args)
        assert rc != 0 and word in msg, (args, msg)
    assert (wav == 7.0).all()   # nothing was written
    with pytest.raises(MttsError, match="unknown HiFi-GAN tensor resblocks.9.convs1.0.w"):
        voc.load("resblocks.9.convs1.0.w", np.zeros(4, np.float32))
    with pytest.raises(MttsError, match="size mismatch for conv_post.w"):
        voc.load("conv_post.w", np.zeros(8, np.float32))
    with pytest.raises(MttsError, match="T_max"):
        voc.mel2wav(np.zeros((1, 16, 3), np.float32))
    voc.close()


def test_refused_loads_leave_the_handle_unchanged_and_the_table_lists_pack_tensors(emu_lib):
    sd = H.synthetic_state_dict(5, CFG_A, 16)
    voc = H.HiFiGAN(sd, CFG_A, n_mel=16, max_B=2, max_T=24, lib_path=emu_lib)
    mel, lens = _mel(1, 2, 20, 16), np.array([20, 13], np.int32)
    before = voc.mel2wav(mel, lens)
    with pytest.raises(MttsError, match="unknown HiFi-GAN tensor resblocks.9.convs1.0.w"):
        voc.load("resblocks.9.convs1.0.w", np.ones(4, np.float32))
    with pytest.raises(MttsError, match="size mismatch for conv_post.w: 8 floats given, 112 expected"):
        voc.load("conv_post.w", np.ones(8, np.float32))
    assert np.array_equal(voc.mel2wav(mel, lens), before)
    table, name, numel = [], C.create_string_buffer(128), C.c_int64()
    for i in range(voc.lib.mtts_hifigan_param_count(voc.h)):
        assert voc.lib.mtts_hifigan_param_info(voc.h, i, name, 128, C.byref(numel)) == 0
        table.append((name.value.decode(), numel.value))
    assert table == [(k, v.size) for k, v in H.pack_tensors(sd, CFG_A, 16).items()]
    assert voc.lib.mtts_hifigan_param_info(voc.h, len(table), name, 128, C.byref(numel)) != 0
    voc.close()


# ---- 6. duck type ----------------------------------------------------------------------------------------------------------------------
def test_hifigan_feeds_the_unmodified_saver(tmp_path, emu_lib):
    from scipy.io import wavfile
    from meta_tts_amd.saver import CSV_COLUMNS, Saver
    voc = H.HiFiGAN(None, CFG_A, n_mel=16, max_B=2, max_T=12, lib_path=emu_lib)
    rs = np.random.RandomState(11)
    B, T = 2, 12
    mel_lens = np.asarray([12, 7], np.int64)
    gt = rs.uniform(-8, -1, (B, T, 16)).astype(np.float32)
    post = rs.uniform(-8, -1, (B, T, 16)).astype(np.float32)
    ids = ["spk_a", "spk_b"]
    targets = (ids, None, None, None, None, None, gt, mel_lens)
    preds = [None, post] + [None] * 7 + [mel_lens]
    outputs = [{"_batch": targets, "step_0": {"recon": {"output": preds, "losses": [0.1] * len(CSV_COLUMNS)}, "synth": {"output": preds}}}]
    batch = [([(["s0"],)], [(["q0"],)])]
    pre = {"preprocessing": {"stft": {"hop_length": voc.hop}, "audio": {"sampling_rate": 22050, "max_wav_value": 32768.0}}}
    sv = Saver(pre, str(tmp_path / "log"), str(tmp_path / "result"))
    sv.on_test_batch_end(outputs, batch, {"s0.q0": "task_1"}, 5, 1, 0, voc)
    adir = tmp_path / "result" / "audio" / "Testing" / "step_5" / "task_1"
    assert sorted(os.listdir(adir)) == sorted([f"{i}.recon.wav" for i in ids] + [f"{i}.step_5-FTstep_0.synth.wav" for i in ids])
    for i, L in zip(ids, mel_lens):
        for name in (f"{i}.recon.wav", f"{i}.step_5-FTstep_0.synth.wav"):
            rate, w = wavfile.read(adir / name)
            assert rate == 22050 and w.dtype == np.int16 and len(w) == voc.hop * int(L) and np.abs(w).max() > 0
    voc.close()


# ---- the MI355X ------------------------------------------------------------------------------------------------------------------------
V1_T, V1_LENS = 40, (40, 23)


@pytest.fixture(scope="module")
def v1_case():
    return H.synthetic_state_dict(0), _mel(2, 2, V1_T, 80)


@pytest.mark.gpu
@pytest.mark.parametrize("direct_max", [0, 64])
def test_full_v1_on_gpu_vs_oracle(v1_case, direct_max):
    """10 240 rows at the last stage: many tiles, a ragged second utterance, every channel count of V1 on both routes."""
    sd, mel = v1_case
    voc = H.HiFiGAN(sd, max_B=2, max_T=48, direct_max_channels=direct_max)
    wav = voc.mel2wav(mel, np.array(V1_LENS, np.int32))
    assert wav.shape == (2, V1_T * 256)
    _check_against_oracle("V1", wav, sd, mel, V1_LENS, H.V1, 256)
    assert np.array_equal(wav, voc.mel2wav(mel, np.array(V1_LENS, np.int32)))
    voc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("direct_max", [0, 64])
def test_device_entry_equals_host_entry_bit_for_bit(v1_case, direct_max):
    sd, mel = v1_case
    voc = H.HiFiGAN(sd, max_B=2, max_T=48, direct_max_channels=direct_max)
    lens = np.array(V1_LENS, np.int32)
    ref = voc.mel2wav(mel, lens)
    voc.set_stream(torch.cuda.current_stream().cuda_stream)
    x = torch.from_numpy(np.ascontiguousarray(mel.transpose(0, 2, 1))).cuda()      # [B][T][n_mel]
    wav_ptr, stride, n, stream = voc.infer_device(x.data_ptr(), 0, 2, V1_T, lens)
    assert stride == V1_T * 256 and np.array_equal(n, lens * 256) and stream == torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    got = voc._wav_dev[:2 * stride].reshape(2, stride).cpu().numpy()
    for b in range(2):
        np.testing.assert_array_equal(got[b, :n[b]], ref[b, :n[b]])
    voc.close()


@pytest.mark.gpu
def test_infer_device_feeds_the_speaker_embedder(v1_case):
    from meta_tts_amd import evaluation as E
    from meta_tts_amd.speaker_encoder import synthetic_state_dict
    tiny = dict(hidden=64, emb=32, layers=2)
    sd, mel = v1_case
    voc = H.HiFiGAN(sd, max_B=2, max_T=48)
    emb = E.SpeakerEmbedder(synthetic_state_dict(3, **tiny), max_partials=2, **tiny)
    x = torch.from_numpy(np.ascontiguousarray(mel.transpose(0, 2, 1))).cuda()
    torch.cuda.synchronize()
    wav_ptr, stride, n, stream = voc.infer_device(x.data_ptr(), 0, 2, V1_T, np.array(V1_LENS, np.int32))
    vec = emb.embed_device(wav_ptr, stride, n, stream=stream, source_rate=22050, normalize_dbfs=-30.0)
    assert vec.shape == (2, 32) and np.isfinite(vec).all()
    np.testing.assert_allclose(np.linalg.norm(vec, axis=1), 1.0, atol=1e-5)
    voc.close(); emb.close()
