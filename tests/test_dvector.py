"""d-vector speaker encoder (csrc/dvector.h through include/mtts.h: mtts_dvector_*) against oracle/dvector_oracle.py — torch's own
nn.LSTM / nn.Linear (the operators the reference's GE2E class is made of, speaker_encoder.py:11-31) and the utterance reduction of
speaker_encoder.py:71-76.  Small shapes through the SIMT emulator on CPU, the reference's shapes (40 mels, 160 frames, 3 x 256)
on the MI355X.

The configurations below NEW_CONFIGS are the ones DVector::init accepts and nothing else runs (one frame, one layer, an embedding that does
not fill its last wavefront, 1024 hidden units, one partial per utterance).  They are compared with the oracle in float64, under the rule of
test_dvector_kernels.py: the bound of an output is 8 x the distance between the float64 oracle and the same oracle in float32, capped at
the 2e-4 (forward) / 2e-3 of the largest entry (gradients) of the two original cases; each comparison prints a DVEC_CHAIN line first."""
import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from meta_tts_amd import speaker_encoder as se
from oracle import dvector_oracle as orc


def _bounded(name, got, ref, ref32, cap, floor):
    """|got - ref| <= min(8 x |ref32 - ref|, cap), all relative to max(floor, max|ref|) (module docstring)."""
    ref, ref32 = np.asarray(ref, np.float64), np.asarray(ref32, np.float64)
    assert np.isfinite(ref).all(), name                      # (a partial whose ReLU units are all dead has no embedding: not these inputs)
    scale = max(floor, float(np.abs(ref).max()))
    dist = float(np.abs(ref - ref32).max()) / scale
    bound = min(8.0 * dist, cap)
    err = float(np.abs(np.asarray(got, np.float64) - ref).max()) / scale
    print(f"DVEC_CHAIN {name} err {err:.3e} f32_restatement {dist:.3e} bound {bound:.3e} max|ref| {np.abs(ref).max():.3e}")
    assert err <= bound, f"{name}: {err:.3e} > {bound:.3e} (relative to {scale:.3e})"


def _case(seed, n_utts, frames, cfg, one_partial=False):
    g = np.random.RandomState(seed)
    counts = g.randint(1, 4, size=n_utts)
    if one_partial:
        counts[:] = 1
    n = int(counts.sum())
    mels = g.standard_normal((n, frames, cfg["n_mels"])).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(counts)])
    slices = [slice(int(off[i]), int(off[i + 1])) for i in range(n_utts)]
    return mels, slices


def _run(lib_path, cfg, frames, seed, n_utts, dtype=torch.float32, one_partial=False):
    """dtype: the oracle's.  float32: the two original cases and their assertions; float64: the restatement rule of the module docstring."""
    sd = se.synthetic_state_dict(seed, **cfg)
    enc = se.DVectorEncoder(sd, max_partials=64, max_utts=16, frames=frames, lib_path=lib_path, **cfg)
    mels, slices = _case(seed + 1, n_utts, frames, cfg, one_partial)
    out, part = enc.embed(mels, slices, return_partials=True)
    ref_p = orc.partial_embeds(sd, mels, dtype=dtype, **cfg).numpy()
    ref = orc.speaker_embeds(sd, mels, slices, dtype=dtype, **cfg).numpy()
    if dtype == torch.float32:
        np.testing.assert_allclose(part, ref_p, rtol=2e-4, atol=2e-5)
        np.testing.assert_allclose(out, ref, rtol=2e-4, atol=2e-5)
    else:
        tag = f"{'gpu' if lib_path is None else 'emu'} {_tag(cfg, frames)}"
        _bounded(tag + ".partials", part, ref_p, orc.partial_embeds(sd, mels, **cfg).numpy(), 2e-4, 1.0)
        _bounded(tag + ".out", out, ref, orc.speaker_embeds(sd, mels, slices, **cfg).numpy(), 2e-4, 1.0)
    np.testing.assert_allclose(np.linalg.norm(out, axis=1), 1.0, rtol=1e-5)
    # __call__ keeps the reference's (ref_mels, ref_slices) signature
    np.testing.assert_array_equal(enc((mels, slices)), out)
    with pytest.raises(ValueError):
        enc.embed(mels, slices[:-1])
    enc.close()


def test_dvector_emulator_small():
    _run(ge.build_emulator(), dict(n_mels=8, hidden=64, emb=64, layers=2), frames=7, seed=3, n_utts=3)


def test_state_dict_names_and_errors():
    cfg = dict(n_mels=8, hidden=64, emb=64, layers=1)
    sd = se.synthetic_state_dict(0, **cfg)
    ck = {"model.speaker_emb.model." + k: v for k, v in sd.items()}          # the reference checkpoint's prefix
    enc = se.DVectorEncoder(ck, max_partials=4, max_utts=2, frames=5, lib_path=ge.build_emulator(), **cfg)
    assert set(enc.state_dict()) == set(sd)
    bad = dict(sd)
    bad["linear.weight"] = np.zeros((3, 3), np.float32)
    with pytest.raises(ValueError):
        enc.load_state_dict(bad)
    with pytest.raises(ValueError):
        enc.embed(np.zeros((1, 6, 8), np.float32), [slice(0, 1)])            # wrong frame count
    with pytest.raises(Exception, match="at least one partial"):
        enc.embed(np.zeros((2, 5, 8), np.float32), [slice(0, 2), slice(2, 2)])   # an utterance without partial utterances
    with pytest.raises(ValueError):
        enc.embed(np.zeros((5, 5, 8), np.float32), [slice(0, 5)])            # more partials than the encoder was created for
    enc.close()


def test_refused_loads_leave_the_handle_unchanged():
    import ctypes as C
    cfg = dict(n_mels=8, hidden=64, emb=64, layers=1)
    enc = se.DVectorEncoder(se.synthetic_state_dict(0, **cfg), max_partials=4, max_utts=2, frames=5, lib_path=ge.build_emulator(), **cfg)
    mels, slices = np.random.RandomState(1).standard_normal((3, 5, 8)).astype(np.float32), [slice(0, 1), slice(1, 3)]
    before = enc.embed(mels, slices)
    junk = np.ones(8, np.float32)

    def load(name, n):
        rc = enc.lib.mtts_dvector_load(enc.h, name.encode(), junk.ctypes.data_as(C.c_void_p), n)
        return rc, enc.lib.mtts_dvector_last_error(enc.h).decode()

    rc, msg = load("lstm.weight_ih_l1", 4)
    assert rc != 0 and msg == "unknown d-vector tensor lstm.weight_ih_l1"
    rc, msg = load("linear.bias", 8)
    assert rc != 0 and msg == "size mismatch for linear.bias: 8 floats given, 64 expected"
    np.testing.assert_array_equal(enc.embed(mels, slices), before)
    enc.close()


@pytest.mark.gpu
def test_dvector_gpu_reference_shapes():
    ge.build_device()
    _run(None, dict(n_mels=40, hidden=256, emb=256, layers=3), frames=160, seed=11, n_utts=5)


def _oracle_grads(sd, cfg, mels, slices, dout, dtype):
    """The oracle's modules in `dtype`, the utterance embeddings and, in the parameters' .grad, the gradient of sum(emb * dout)."""
    lstm, linear = orc.build(sd, dtype=dtype, **cfg)
    _, (hidden, _) = lstm(torch.from_numpy(mels).to(dtype))
    raw = torch.relu(linear(hidden[-1]))
    pe = raw / torch.norm(raw, dim=1, keepdim=True)
    emb = torch.stack([torch.nn.functional.normalize(pe[sl].mean(dim=0), dim=0) for sl in slices])
    (emb * torch.from_numpy(dout).to(dtype)).sum().backward()
    grads = {f"lstm.{n}": p.grad.numpy() for n, p in lstm.named_parameters()}
    grads.update({f"linear.{n}": p.grad.numpy() for n, p in linear.named_parameters()})
    return lstm, linear, emb.detach().numpy(), grads


def _train_case(lib_path, cfg, frames, seed, n_utts, tol, dtype=torch.float32, one_partial=False):
    """Back-propagation through time of the trained variants (speaker_emb: encoder / scratch_encoder) against torch autograd of the
    oracle (nn.LSTM + nn.Linear), then one joint-norm-clipped Adam step against torch.optim.Adam.  dtype: as in _run (float64: `tol` is the
    cap of the restatement rule)."""
    import ctypes as C
    sd = se.synthetic_state_dict(seed, **cfg)
    enc = se.DVectorEncoder(sd, max_partials=64, max_utts=16, frames=frames, lib_path=lib_path, **cfg)
    enc.enable_training()
    mels, slices = _case(seed + 1, n_utts, frames, cfg, one_partial)
    g = np.random.RandomState(seed + 2)
    dout = g.standard_normal((n_utts, cfg["emb"])).astype(np.float32)
    out = enc((mels, slices))                                   # training forward
    enc.backward(dout)
    lstm, linear, emb, ref = _oracle_grads(sd, cfg, mels, slices, dout, dtype)
    if dtype == torch.float32:
        np.testing.assert_allclose(out, emb, rtol=2e-4, atol=2e-5)
        for name, r in ref.items():
            got = enc.export(name, 1)
            assert np.abs(got - r).max() <= tol * np.abs(r).max() + 1e-7, (name, np.abs(got - r).max(), np.abs(r).max())
    else:
        tag = f"{'gpu' if lib_path is None else 'emu'} {_tag(cfg, frames)}"
        _, _, emb32, ref32 = _oracle_grads(sd, cfg, mels, slices, dout, torch.float32)
        _bounded(tag + ".out(train)", out, emb, emb32, 2e-4, 1.0)
        for name, r in ref.items():
            got = enc.export(name, 1)
            if not np.any(r):                                   # one frame: h_0 = 0, the recurrent weights have no gradient at all
                assert frames == 1 and name.startswith("lstm.weight_hh") and not np.any(got), name
            else:
                _bounded(f"{tag}.grad({name})", got, r, ref32[name], tol, 1e-30)
    # Adam with the clip coefficient of a joint norm (here: the encoder alone, handed over as a device scalar)
    total = float(np.sqrt(sum((r.astype(np.float64) ** 2).sum() for r in ref.values())))
    max_norm = 0.5 * total
    lib = enc.lib
    norm = np.array([total], np.float32)
    if lib_path is None:
        tn = torch.from_numpy(norm).cuda()
        ptr = C.c_void_p(tn.data_ptr())
    else:
        ptr = norm.ctypes.data_as(C.c_void_p)
    enc.adam_step(ptr, max_norm, 1e-2)
    params = list(lstm.parameters()) + list(linear.parameters())
    torch.nn.utils.clip_grad_norm_(params, max_norm)
    opt = torch.optim.Adam(params, lr=1e-2, betas=(0.9, 0.98), eps=1e-9)
    opt.step()
    # first Adam step: w -= lr * g / (|g| + eps) — entries whose (clipped) gradient is of the order of eps = 1e-9 move by a
    # rounding-dependent fraction of the step, so compare where |g| >> eps
    for n, p in [(f"lstm.{n}", p) for n, p in lstm.named_parameters()] + [("linear.weight", linear.weight)]:
        if not np.any(ref[n]):        # (the one-frame case above) no gradient: Adam leaves the weights as they were
            np.testing.assert_array_equal(enc.export(n), sd[n])
            continue
        live = np.abs(p.grad.numpy()) > 1e-6
        assert live.mean() > 0.2      # rows of dead ReLU units have no gradient at all
        np.testing.assert_allclose(enc.export(n)[live], p.detach().numpy()[live], rtol=1e-4, atol=5e-6, err_msg=n)
    # the updated weights are the ones the next forward uses
    out2 = enc.embed(mels, slices)
    ref2 = orc.speaker_embeds({k: enc.export(k) for k in sd}, mels, slices, **cfg).numpy()
    np.testing.assert_allclose(out2, ref2, rtol=2e-4, atol=2e-5)
    enc.close()


def test_dvector_training_emulator_small():
    _train_case(ge.build_emulator(), dict(n_mels=8, hidden=64, emb=64, layers=2), frames=7, seed=4, n_utts=3, tol=2e-4)


@pytest.mark.gpu
def test_dvector_training_gpu_reference_shapes():
    ge.build_device()
    _train_case(None, dict(n_mels=40, hidden=256, emb=256, layers=3), frames=160, seed=12, n_utts=4, tol=2e-3)


# ---- the configurations nothing else runs (module docstring) -----------------------------------------------------------------------------
# Seeds 21 (forward) / 22 (training).  With four embedding units a partial's ReLU units are all dead under one seed in eight or so, and then it
# has no embedding (0 / 0); 22 is such a seed, so that configuration trains with 35, the next one that leaves three of the four units live in
# every partial (21 does too) — a property of the weights, read off the float64 oracle.
NEW_CONFIGS = {   # id -> (cfg, frames, n_utts, one partial per utterance, training seed)
    "one_frame_one_layer_emb100": (dict(n_mels=8, hidden=64, emb=100, layers=1), 1, 3, False, 22),
    "two_frames_emb4_one_partial": (dict(n_mels=12, hidden=128, emb=4, layers=2), 2, 3, True, 35),
    "hidden1024_emb68": (dict(n_mels=8, hidden=1024, emb=68, layers=1), 3, 2, False, 22),
}


def _tag(cfg, frames):
    return f"chain[{cfg['n_mels']}/{cfg['hidden']}/{cfg['emb']}/{cfg['layers']} layers/{frames} frames]"


@pytest.mark.parametrize("which", sorted(NEW_CONFIGS))
def test_dvector_emulator_unusual_configurations(which):
    cfg, frames, n_utts, one, _ = NEW_CONFIGS[which]
    _run(ge.build_emulator(), cfg, frames, seed=21, n_utts=n_utts, dtype=torch.float64, one_partial=one)


@pytest.mark.parametrize("which", sorted(NEW_CONFIGS))
def test_dvector_training_emulator_unusual_configurations(which):
    cfg, frames, n_utts, one, seed = NEW_CONFIGS[which]
    _train_case(ge.build_emulator(), cfg, frames, seed=seed, n_utts=n_utts, tol=2e-3, dtype=torch.float64, one_partial=one)


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(NEW_CONFIGS))
def test_dvector_gpu_unusual_configurations(which):
    ge.build_device()
    cfg, frames, n_utts, one, _ = NEW_CONFIGS[which]
    _run(None, cfg, frames, seed=21, n_utts=n_utts, dtype=torch.float64, one_partial=one)


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(NEW_CONFIGS))
def test_dvector_training_gpu_unusual_configurations(which):
    ge.build_device()
    cfg, frames, n_utts, one, seed = NEW_CONFIGS[which]
    _train_case(None, cfg, frames, seed=seed, n_utts=n_utts, tol=2e-3, dtype=torch.float64, one_partial=one)


def test_create_refuses_an_embedding_size_that_is_no_multiple_of_four():
    """The weight-gradient GEMM reads dz [N][emb] with float4 loads, and dz_s / linT / the bias column sums are sized alike: emb % 4 is refused
    as n_mels % 4 and hidden % 64 are."""
    import ctypes as C
    from meta_tts_amd import _lib
    lib = _lib.load(ge.build_emulator())
    for emb in (6, 101, 255):
        h = C.c_void_p()
        assert lib.mtts_dvector_create(8, 64, 1, emb, 4, 5, 2, 0, C.byref(h)) == -1 and not h.value
        assert lib.mtts_dvector_last_error(None).decode() == "unsupported d-vector configuration (n_mels % 4, hidden % 64 <= 1024, emb % 4 <= 256)"
    h = C.c_void_p()
    assert lib.mtts_dvector_create(8, 64, 1, 8, 4, 5, 2, 0, C.byref(h)) == 0 and h.value
    lib.mtts_dvector_destroy(h)
