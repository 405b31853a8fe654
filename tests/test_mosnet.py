"""MOSNet (csrc/mosnet.h through include/mtts.h: mtts_mosnet_*; meta_tts_amd/mosnet.py; evaluation.NeuralMOS) against
tests/mosnet_oracle.py, the torch restatement of the definition in include/mtts.h (parity with the published weights, the window and the
recurrent activation is UNPINNED: none of speechmetrics, TensorFlow and cnn_blstm.h5 is in the reference tree).  Host packing and the
whole chain through the SIMT emulator on the CPU, the real kernels on the GPU.

Tolerance (the rule of tests/test_hifigan.py): per compared utterance e32 = max |float32 oracle - float64 oracle| over its frame scores
and its utterance score; the device must stay within max(4 * e32, 2e-5 * max(1, max |ref|)) of the float64 oracle on both.  Every
comparison prints e32, the device error and the gate.

Preconditions, asserted on the float64 oracle so that a comparison is not hollow: behind each of the 12 ReLUs between 15 % and 85 % of the
activations are positive; BLSTM gate pre-activations have |x| < 6 on >= 99 % of entries; the frame scores of every compared utterance of
two or more frames have a standard deviation > 0.02 (one frame has none); the utterance scores of a batch differ pairwise by more than
100 x the gate.

The backward-direction test (6) takes the first of the two routes the definition allows: the convolution kernels are reversed along time
together with the swap of the forward and backward LSTM weights (and of the two halves of the dense layer's input, which the
concatenation [forward | backward] hands over in the swapped order), so the whole network run on the time-reversed utterance must give
the reversed frame scores."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from meta_tts_amd import evaluation as E
from meta_tts_amd import mosnet as M
from meta_tts_amd.engine import MttsError

import mosnet_oracle as MO


@pytest.fixture(scope="module")
def emu_lib():
    return ge.build_emulator()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _mags(seed, n_freq, Ts):
    """Magnitude-like inputs of order 1 with structure along time and frequency; utterance i is scaled by 0.6 + 0.35 i so that the
    utterance scores of a batch differ."""
    g = np.random.RandomState(seed)
    out = []
    for i, T in enumerate(Ts):
        env = 0.6 + 0.4 * np.sin(0.7 * np.arange(T)[:, None] + i) * np.cos(0.11 * np.arange(n_freq)[None, :] * (1 + i))
        out.append((np.abs(g.standard_normal((T, n_freq))) * env * (0.6 + 0.35 * i)).astype(np.float32))
    return out


_REFS = {}


def _refs(key, sd, mags, n_freq, mags32=None):
    """[(frame scores float64, utterance score float64, e32, gate)] per utterance, each run alone; computed once per case and shared.
    mags32: what the float32 oracle reads instead (a float32 front-end's magnitudes, when the device computes them itself)."""
    if key not in _REFS:
        torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
        stats = {}
        u64, f64 = MO.network(sd, mags, n_freq, torch.float64, stats)
        u32, f32 = MO.network(sd, mags if mags32 is None else mags32, n_freq, torch.float32)
        gates = np.concatenate(stats["gates"])
        assert (np.abs(gates) < 6).mean() >= 0.99, (key, (np.abs(gates) < 6).mean())
        out = []
        for i in range(len(mags)):
            assert all(0.15 <= s <= 0.85 for s in stats["relu"][i]), (key, i, stats["relu"][i])
            assert len(f64[i]) < 2 or f64[i].std() > 0.02, (key, i, f64[i].std())
            e32 = max(float(np.abs(f32[i].astype(np.float64) - f64[i]).max()), abs(float(u32[i]) - float(u64[i])))
            gate = max(4.0 * e32, 2e-5 * max(1.0, float(np.abs(f64[i]).max()), abs(float(u64[i]))))
            f64[i].setflags(write=False)
            out.append((f64[i], float(u64[i]), e32, gate))
        for i in range(len(out)):
            for j in range(i):
                assert abs(out[i][1] - out[j][1]) > 100.0 * max(out[i][3], out[j][3]), (key, i, j, out[i][1], out[j][1])
        _REFS[key] = out
    return _REFS[key]


def _check(key, refs, utt, frames):
    for i, (f64, u64, e32, gate) in enumerate(refs):
        err = max(float(np.abs(frames[i].astype(np.float64) - f64).max()), abs(float(utt[i]) - u64))
        print(f"{key} utterance {i} (T = {len(f64)}): e32 {e32:.3e}  device error {err:.3e}  gate {gate:.3e}")
        assert frames[i].shape == f64.shape and err <= gate, (key, i, err, e32, gate)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and len(a[1]) == len(b[1]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


# ---- 1. spec -------------------------------------------------------------------------------------------------------------------------
def test_spec_names_shapes_and_parameter_count(emu_lib):
    spec = dict(M.tensor_spec(257))
    assert len(spec) == 34 and M.widths(257) == [257, 86, 29, 10, 4] and M.widths(33) == [33, 11, 4, 2, 1]
    for name, shape in (("conv.0.weight", (16, 1, 3, 3)), ("conv.2.weight", (16, 16, 3, 3)), ("conv.3.weight", (32, 16, 3, 3)), ("conv.11.weight", (128, 128, 3, 3)),
                        ("conv.11.bias", (128,)), ("blstm.weight_ih", (512, 512)), ("blstm.weight_hh_reverse", (512, 128)), ("blstm.bias", (512,)),
                        ("dense.weight", (128, 256)), ("dense.bias", (128,)), ("frame_score.weight", (1, 128)), ("frame_score.bias", (1,))):
        assert spec[name] == shape, name
    assert dict(M.tensor_spec(33))["blstm.weight_ih_reverse"] == (512, 128)
    count = lambda pre: sum(int(np.prod(s)) for n, s in spec.items() if n.startswith(pre))   # noqa: E731
    assert (count("conv."), count("blstm."), count("dense."), count("frame_score.")) == (489_312, 656_384, 32_896, 129)
    sd = M.synthetic_state_dict(0)
    packed = M.pack_tensors(sd)
    assert sum(v.size for v in packed.values()) == 1_178_721
    net = M.MOSNet(sd, max_frames=4, max_utts=1, lib_path=emu_lib)
    total, name, numel = 0, C.create_string_buffer(128), C.c_int64()
    assert net.lib.mtts_mosnet_param_count(net.h) == len(packed)
    for i in range(net.lib.mtts_mosnet_param_count(net.h)):
        assert net.lib.mtts_mosnet_param_info(net.h, i, name, 128, C.byref(numel)) == 0
        assert packed[name.value.decode()].size == numel.value
        total += numel.value
    assert total == 1_178_721
    net.close()


# ---- 2. Keras layouts -----------------------------------------------------------------------------------------------------------------
def test_from_keras_weights_round_trip():
    sd = M.synthetic_state_dict(4, 33)
    keras = []
    for name in M.KERAS_ORDER:
        w = sd[name]
        if name.startswith("conv.") and name.endswith("weight"):
            w = w.transpose(2, 3, 1, 0)                   # (cout, cin, 3, 3) -> (3, 3, cin, cout)
        elif w.ndim == 2:
            w = w.T                                       # (out, in) -> (in, out)
        keras.append(np.ascontiguousarray(w))
    assert keras[2].shape == (3, 3, 16, 16) and keras[24].shape == (128, 512) and keras[25].shape == (128, 512) and keras[30].shape == (256, 128)
    back = M.from_keras_weights(keras, 33)
    assert sorted(back) == sorted(sd) and all(np.array_equal(back[k], sd[k]) for k in sd)
    with pytest.raises(MttsError, match="Keras arrays"):
        M.from_keras_weights(keras[:-1], 33)


# ---- 3. padding rule ------------------------------------------------------------------------------------------------------------------
def test_same_padding_rule_and_one_layer_oracle():
    for f_in in (257, 86, 29, 10, 33, 11, 4, 2):
        f_out = -(-f_in // 3)
        total = max((f_out - 1) * 3 + 3 - f_in, 0)
        assert M.same_pad(f_in, 3) == (f_out, total // 2, total - total // 2) == MO.same_pad(f_in, 3), f_in
        assert M.same_pad(f_in, 1) == (f_in, 1, 1)
    assert [M.same_pad(f, 3)[1] for f in (257, 86, 29, 10)] == [0, 0, 0, 1] and [M.same_pad(f, 3)[1] for f in (33, 11, 4, 2)] == [0, 0, 1, 0]
    g = torch.Generator().manual_seed(0)
    for f_in in (10, 11, 29):
        x = torch.randn(1, 3, 5, f_in, generator=g, dtype=torch.float64)
        w, b = torch.randn(4, 3, 3, 3, generator=g, dtype=torch.float64), torch.randn(4, generator=g, dtype=torch.float64)
        f_out, left, right = M.same_pad(f_in, 3)
        xp = torch.zeros(1, 3, 7, f_in + left + right, dtype=torch.float64)
        xp[:, :, 1:6, left:left + f_in] = x
        want = torch.relu(torch.nn.functional.conv2d(xp, w, b, stride=(1, 3)))
        got = MO.conv_layer(x, w, b, 3)
        assert got.shape == (1, 4, 5, f_out) and torch.equal(got, want)


# ---- 4. the narrow chain, ragged -------------------------------------------------------------------------------------------------------
NARROW_T = (20, 7, 1, 2)


def _narrow_case():
    return M.synthetic_state_dict(1, 33), _mags(33, 33, NARROW_T)


def _narrow(lib_path):
    sd, mags = _narrow_case()
    net = M.MOSNet(sd, 33, max_frames=64, max_utts=8, lib_path=lib_path)
    whole = net.score_magnitudes(mags)
    _check("n_freq 33", _refs("narrow", sd, mags, 33), *whole)
    for i, m in enumerate(mags):
        u, f = net.score_magnitudes([m])
        assert u[0] == whole[0][i] and np.array_equal(f[0], whole[1][i]), i      # alone = in the batch, bit for bit
    for cut in (8, 1000):
        assert _same(net.score_magnitudes(mags, frames_per_call=cut), whole), cut
    net.close()


def test_narrow_chain_ragged_batch(emu_lib):
    _narrow(emu_lib)


# ---- 5. the real width ------------------------------------------------------------------------------------------------------------------
def test_full_width_chain(emu_lib):
    """257 -> 86 -> 29 -> 10 -> 4: every instance of the convolution kernel, the pad-left-1 last stage, 512 BLSTM inputs."""
    sd, mags = M.synthetic_state_dict(1), _mags(257, 257, (12, 3))
    net = M.MOSNet(sd, max_frames=16, max_utts=2, lib_path=emu_lib)
    _check("n_freq 257", _refs("full", sd, mags, 257), *net.score_magnitudes(mags))
    net.close()


# ---- 6. the backward direction ------------------------------------------------------------------------------------------------------------
def test_backward_direction_by_time_reversal(emu_lib):
    sd, mags = _narrow_case()
    rev = {}
    for k, v in sd.items():
        if k.startswith("conv.") and k.endswith("weight"):
            rev[k] = np.ascontiguousarray(v[:, :, ::-1, :])
        elif k.startswith("blstm."):
            rev[k[:-len("_reverse")] if k.endswith("_reverse") else k + "_reverse"] = v
        elif k == "dense.weight":
            rev[k] = np.ascontiguousarray(np.concatenate([v[:, 128:], v[:, :128]], axis=1))   # [forward | backward] change places too
        else:
            rev[k] = v
    x = mags[0]
    refs = _refs("narrow", sd, mags, 33)[:1]
    # the definition has the symmetry: the float64 oracle of the transformed problem is the reverse of the original's
    _, f_rev = MO.network(rev, [x[::-1]], 33, torch.float64)
    assert np.abs(f_rev[0][::-1] - refs[0][0]).max() < 1e-12
    net = M.MOSNet(rev, 33, max_frames=32, max_utts=1, lib_path=emu_lib)
    u, f = net.score_magnitudes([np.ascontiguousarray(x[::-1])])
    _check("time-reversed", refs, u, [f[0][::-1]])
    net.close()


# ---- 7. waveforms -------------------------------------------------------------------------------------------------------------------------
def _wav(seed, n, amp=0.05):
    g = np.random.RandomState(seed)
    t = np.arange(n)
    return (amp * (0.5 + 0.5 * np.sin(2 * np.pi * t / 1900.0 + seed)) * g.standard_normal(n) + 0.5 * amp * np.sin(2 * np.pi * (200.0 + 90 * seed) * t / 16000.0)).astype(np.float32)


def _front_magnitudes(net, wav):
    """MelFront's own magnitudes of one waveform through mtts_stft_transform on the network's front-end handle."""
    front = net.front()
    T = len(wav) // 256 + 1
    mag, ph = np.empty((T, net.n_freq), np.float32), np.empty((T, net.n_freq), np.float32)
    assert front.check(net.lib.mtts_stft_transform(front.h, _ptr(wav), len(wav), _ptr(mag), _ptr(ph))) == T
    return mag


def test_score_wavs_equals_score_magnitudes_of_the_front_end(emu_lib):
    net = M.MOSNet(M.synthetic_state_dict(1), max_frames=32, max_utts=4, lib_path=emu_lib)
    wavs = [_wav(1, 300), _wav(2, 1000), _wav(3, 2600)]
    utt, frames = net.score_wavs(wavs)
    assert [len(f) for f in frames] == [len(w) // 256 + 1 for w in wavs] == [2, 4, 11]
    assert _same((utt, frames), net.score_magnitudes([_front_magnitudes(net, w) for w in wavs]))
    assert _same((utt, frames), net.score_wavs(wavs, source_rate=16000, frames_per_call=5))
    src = [_wav(4, 500), _wav(5, 1400), _wav(6, 3600)]                       # at 22 050 Hz
    two_step = net.resampler(22050).resample_batch(src)
    assert [len(w) for w in two_step] == [-(-len(w) * 320 // 441) for w in src]
    assert _same(net.score_wavs(src, source_rate=22050), net.score_wavs(two_step))
    net.close()


def test_refused_loads_leave_the_handle_unchanged_and_the_table_lists_pack_tensors(emu_lib):
    sd = M.synthetic_state_dict(1, 33)
    mags = _mags(33, 33, (3, 2))
    net = M.MOSNet(sd, 33, max_frames=8, max_utts=2, lib_path=emu_lib)
    before = net.score_magnitudes(mags)
    with pytest.raises(MttsError, match="unknown MOSNet tensor conv.12.w"):
        net.load("conv.12.w", np.ones(4, np.float32))
    with pytest.raises(MttsError, match="size mismatch for dense.b: 127 floats given, 128 expected"):
        net.load("dense.b", np.ones(127, np.float32))
    assert _same(net.score_magnitudes(mags), before)
    table, name, numel = [], C.create_string_buffer(128), C.c_int64()
    for i in range(net.lib.mtts_mosnet_param_count(net.h)):
        assert net.lib.mtts_mosnet_param_info(net.h, i, name, 128, C.byref(numel)) == 0
        table.append((name.value.decode(), numel.value))
    assert table == [(k, v.size) for k, v in M.pack_tensors(sd, 33).items()]
    assert net.lib.mtts_mosnet_param_info(net.h, len(table), name, 128, C.byref(numel)) != 0
    net.close()


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(emu_lib):
    sd = M.synthetic_state_dict(1, 33)
    net = M.MOSNet(sd, 33, max_frames=8, max_utts=2, lib_path=emu_lib)
    good = _mags(1, 33, (3,))[0]
    us, fs = np.zeros(4, np.float32), np.zeros(16, np.float32)

    def raw(n_frames, mag):
        n = np.asarray(n_frames, np.int32)
        rc = net.lib.mtts_mosnet_score(net.h, len(n), _ptr(n), _ptr(mag), _ptr(us), _ptr(fs))
        return rc, net.lib.mtts_mosnet_last_error(net.h).decode()

    rc, msg = raw([3, 0], good)
    assert rc != 0 and "utterance 1: n_frames < 1" in msg
    bad = good.copy()
    bad[2, 5] = np.nan
    rc, msg = raw([3], bad)
    assert rc != 0 and "non-finite magnitude at frame 2, column 5" in msg
    with pytest.raises(MttsError, match="max_frames_per_call = 8"):
        net.score_magnitudes(_mags(2, 33, (9,)))
    rc, msg = raw([1, 1, 1], np.concatenate([good, good]))
    assert rc != 0 and "exceed max_utts = 2" in msg
    assert net.lib.mtts_mosnet_score(net.h, 1, None, _ptr(good), _ptr(us), None) != 0 and "NULL argument" in net.lib.mtts_mosnet_last_error(net.h).decode()
    with pytest.raises(MttsError, match="unknown MOSNet tensor conv.12.w"):
        net.load("conv.12.w", np.zeros(4, np.float32))
    with pytest.raises(MttsError, match="size mismatch for dense.b: 127 floats given, 128 expected"):
        net.load("dense.b", np.zeros(127, np.float32))
    with pytest.raises(MttsError, match="tensor dense.bias is missing"):
        M.MOSNet({k: v for k, v in sd.items() if k != "dense.bias"}, 33, max_frames=8, max_utts=2, lib_path=emu_lib)
    h = C.c_void_p()
    assert net.lib.mtts_mosnet_create(33, 8, 2, 0, C.byref(h)) == 0                     # a handle nothing was loaded into
    n1 = np.asarray([3], np.int32)
    assert net.lib.mtts_mosnet_score(h, 1, _ptr(n1), _ptr(good), _ptr(us), _ptr(fs)) != 0
    assert "tensor conv.0.w has not been loaded" in net.lib.mtts_mosnet_last_error(h).decode()
    net.lib.mtts_mosnet_destroy(h)
    assert net.lib.mtts_mosnet_create(1, 8, 2, 0, C.byref(h)) != 0 and "n_freq" in net.lib.mtts_mosnet_last_error(None).decode()
    # waveforms: a 32-sample filter (n_freq 17) is not this network's front-end; a wav the reflection padding cannot read
    from meta_tts_amd.audio.stft import _Handle
    other = _Handle(32, 16, 1, 4096, 0, emu_lib)
    w, n, nf = _wav(1, 400), np.asarray([400], np.int32), np.zeros(1, np.int32)
    assert net.lib.mtts_mosnet_score_wavs(net.h, other.h, 1, _ptr(n), _ptr(w), 0, _ptr(us), _ptr(nf), None) != 0
    assert "filter_length 32, n_freq = 33 needs 64" in net.lib.mtts_mosnet_last_error(net.h).decode()
    other.close()
    with pytest.raises(MttsError, match="waveform too short for the reflection padding"):
        net.score_wavs([_wav(1, 32)])
    net.close()
    full = M.MOSNet(None, max_frames=8, max_utts=2, lib_path=emu_lib)
    with pytest.raises(MttsError, match="waveform too short for the reflection padding"):
        full.score_wavs([_wav(1, 256)])
    with pytest.raises(MttsError, match="no resampler loaded"):
        nn = np.asarray([600], np.int32)
        full._check(full.lib.mtts_mosnet_score_wavs(full.h, full.front().h, 1, _ptr(nn), _ptr(_wav(1, 600)), 1, _ptr(us), _ptr(nf), None))
    assert np.isfinite(full.score_wavs([_wav(1, 600)])[0]).all()                           # the handle stays usable
    full.close()


# ---- 9. NeuralMOS -------------------------------------------------------------------------------------------------------------------------
def _result_tree(tmp_path, n_speaker=2, n_sample=2):
    """A result tree in the reference's layout (tests/data_tree.py writes feature trees, which do not fit here) with empty files; the
    waveforms live in the returned dict and come through `wav_loader` as (waveform, rate): real files at 16 kHz, the others at 22 050 Hz."""
    dirs = {k: tmp_path / k for k in ("recon", "real", "meta", "dvec")}
    wavs, sq = {}, []
    for s in range(n_speaker):
        for k in range(n_sample):
            data_id, qid = s * n_sample + k, f"spk{s:02d}_utt{k}"
            sq.append({"qry_id": [qid]})
            files = {dirs["real"] / f"spk{s:02d}" / f"{qid}.wav": 16000,
                     dirs["recon"] / "audio" / "Testing" / f"test_{data_id:03d}" / f"{qid}.recon.wav": 22050}
            for step in (0, 5):
                files[dirs["meta"] / "audio" / "Testing" / f"test_{data_id:03d}" / f"{qid}.step_5-FTstep_{step}.synth.wav"] = 22050
            for j, (p, rate) in enumerate(files.items()):
                p.parent.mkdir(parents=True, exist_ok=True)
                p.write_bytes(b"")
                wavs[str(p)] = (_wav(10 * data_id + j, 600 + 150 * j + 40 * data_id, 0.03 + 0.02 * j), rate)
    (dirs["recon"] / "test_SQids.json").write_text(json.dumps(sq))
    cfg = E.EvalConfig("Toy", {k: str(v) for k, v in dirs.items()}, n_speaker, n_sample, [("meta", [0, 5]), ("dvec", [0])], work_dir=str(tmp_path))
    return cfg, wavs


def test_neural_mos_on_a_result_tree(emu_lib, tmp_path):
    from scipy import stats
    cfg, wavs = _result_tree(tmp_path)
    net = M.MOSNet(M.synthetic_state_dict(1, 33), 33, max_frames=256, max_utts=8, lib_path=emu_lib)
    read = []

    def loader(p):
        read.append(p)
        return wavs[p]

    ev = E.NeuralMOS(cfg, net, wav_loader=loader)
    assert list(ev.file_list) == ["real", "recon", "meta_step0", "meta_step5"]            # dvec is one of the three modes left out
    with open(cfg.path("csv", "mosnet_real.csv"), "w") as f:                              # an existing csv is kept, its files are not read
        f.write("test_id, mos\n" + "".join(f"test_{i:03}, {3.0 + 0.25 * i}\n" for i in range(4)))
    done = ev.compute_mosnet()
    assert list(done) == ["recon", "meta_step0", "meta_step5"] and not any(p in read for p in ev.file_list["real"])
    for mode, scores in done.items():
        lines = open(cfg.path("csv", f"mosnet_{mode}.csv")).read().splitlines()
        assert lines[0] == "test_id, mos" and lines[1:] == [f"test_{i:03}, {float(s)}" for i, s in enumerate(scores)] and len(scores) == 4
        want = net.score_wavs([wavs[p][0] for p in ev.file_list[mode]], source_rate=22050)[0]
        assert np.array_equal(scores, want) and np.isfinite(scores).all() and len(set(scores.tolist())) == 4
    assert ev.compute_mosnet() == {}
    rows = ev.add_up("mosnet")
    lines = open(cfg.path("txt", "mosnet.txt")).read().splitlines()
    assert [r[0] for r in rows] == list(ev.file_list) and lines == [f"{m}, {mean}, {ci}" for m, mean, ci in rows]
    data = [3.0, 3.25, 3.5, 3.75]
    m, h = ev.get_mean_confidence_interval(data)
    assert (rows[0][1], rows[0][2]) == (m, h) and m == np.mean(data)
    assert abs(h - stats.sem(np.array(data)) * stats.t.ppf((1 + 0.95) / 2.0, 3)) < 1e-12
    for df, p in ((1, 0.975), (3, 0.975), (15, 0.995), (607, 0.975)):
        assert abs(E._student_t_ppf(p, df) - stats.t.ppf(p, df)) < 1e-9 * stats.t.ppf(p, df)
    # the basename check, and a missing wav
    bad = dict(wavs)
    victim = ev.file_list["meta_step5"][2]
    os.remove(victim)
    with pytest.raises(MttsError, match="mode meta_step5: test sample 2 has no"):
        E.NeuralMOS(cfg, net, wav_loader=lambda p: bad[p])
    other = victim.replace("spk01_utt0", "spk01_uttX")
    open(other, "wb").close()
    bad[other] = wavs[victim]
    os.remove(cfg.path("csv", "mosnet_meta_step5.csv"))
    with pytest.raises(MttsError, match="test sample 2 is spk01_uttX, the real file is spk01_utt0"):
        E.NeuralMOS(cfg, net, wav_loader=lambda p: bad[p]).compute_mosnet()
    net.close()


# ---- the MI355X ---------------------------------------------------------------------------------------------------------------------------
FULL_T = (37, 5, 1, 130)


def _gpu_case():
    return M.synthetic_state_dict(1), _mags(7, 257, FULL_T)


@pytest.mark.gpu
def test_gpu_full_width_ragged_batch():
    """T = 130 spans several time tiles of every convolution instance (tiles are 4, 12 and 32 rows), 1 and 5 are shorter than a tile."""
    sd, mags = _gpu_case()
    net = M.MOSNet(sd, max_frames=256, max_utts=8)
    whole = net.score_magnitudes(mags)
    _check("gpu n_freq 257", _refs("gpu_full", sd, mags, 257), *whole)
    for i, m in enumerate(mags):
        u, f = net.score_magnitudes([m])
        assert u[0] == whole[0][i] and np.array_equal(f[0], whole[1][i]), i
    assert _same(net.score_magnitudes(mags), whole)
    net.close()


@pytest.mark.gpu
def test_gpu_cuts_are_bit_identical():
    sd, mags = _gpu_case()
    net = M.MOSNet(sd, max_frames=256, max_utts=8)
    whole = net.score_magnitudes(mags)
    for cut in (40, 140, 1000):
        assert _same(net.score_magnitudes(mags, frames_per_call=cut), whole), cut
    net.close()


GPU_WAV_N = (3200, 8000, 16000, 24000)


def _gpu_wavs():
    return [_wav(20 + i, n, amp) for i, (n, amp) in enumerate(zip(GPU_WAV_N, (0.02, 0.05, 0.09, 0.14)))]   # (amplitudes that keep the scores apart)


@pytest.mark.gpu
def test_gpu_score_wavs():
    """The oracle reads float64 numpy magnitudes; e32 carries the front-end's precision too: the float32 oracle reads a float32 numpy STFT."""
    sd, wavs = M.synthetic_state_dict(1), _gpu_wavs()
    net = M.MOSNet(sd, max_frames=256, max_utts=8)
    utt, frames = net.score_wavs(wavs)
    assert [len(f) for f in frames] == [n // 256 + 1 for n in GPU_WAV_N]
    mags64 = [MO.stft_magnitude(w, dtype=np.float64) for w in wavs]
    mags32 = [MO.stft_magnitude(w, dtype=np.float32) for w in wavs]
    _check("gpu wavs", _refs("gpu_wavs", sd, mags64, 257, mags32), utt, frames)
    src = [_wav(30 + i, n, 0.04) for i, n in enumerate((5000, 12000, 30000))]          # at 22 050 Hz
    assert _same(net.score_wavs(src, source_rate=22050), net.score_wavs(net.resampler(22050).resample_batch(src)))
    net.close()


@pytest.mark.gpu
def test_gpu_narrow_chain_ragged_batch():
    _narrow(None)
