"""GE2E training of the d-vector encoder — csrc/ge2e.h, the mtts_ge2e_loss and mtts_dvector_ge2e_* entries of include/mtts.h and
meta_tts_amd/ge2e.py — against ge2e_oracle.py: the definition of include/mtts.h in float64 torch, gradients by autograd.  Parity with any
published GE2E code is UNPINNED (no such code is in the reference tree); what is pinned is that definition.  Every test runs through the
SIMT emulator on the CPU; the ones marked gpu run the same calls through libmtts.so on the MI355X.

Tolerances are not chosen (the rule of test_dvector_kernels.py / test_dvector.py::_bounded): a device result may be at most 8 x as far from
the float64 oracle as the same oracle evaluated in float32 is, relative to the largest reference entry (for the loss and the similarities:
to max(1, that)), capped at 2e-4 for the loss and the similarities and at 2e-3 for gradients and what the optimizer makes of them.  A
float32 restatement that lands closer than 1e-7 (under one float32 ulp, 2^-23 = 1.19e-7, of the largest entry: chance, not precision) counts
as 1e-7.  Every comparison prints a GE2E_DIST line (err, f32_restatement, bound, max|ref|) before it asserts.  dL/dw and dL/db are compared as
one two-entry gradient: dL/db is a sum of softmax-minus-onehot rows, zero but for rounding.

The measured figures, emulator and MI355X, are in the README paragraph "GE2E training of the speaker encoder"."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import ge2e_oracle as GO
from meta_tts_amd import speaker_encoder as se
from meta_tts_amd.ge2e import GE2ETrainer, SpeakerBatchSampler, batch_eer, mels_from_wavs
from oracle_util import Dev
from test_kernel_entries import dev  # noqa: F401  (the emu / gpu fixture)

F32 = np.float32
CAP_VALUE, CAP_GRAD, FLOOR = 2e-4, 2e-3, 1e-7


def _close(where, name, got, ref, ref32, cap, scale_floor=0.0):
    ref, ref32 = np.asarray(ref, np.float64), np.asarray(ref32, np.float64).reshape(np.shape(ref))
    got = np.asarray(got, np.float64).reshape(ref.shape)
    assert np.isfinite(ref).all() and np.abs(ref).max() > 0, name
    scale = max(scale_floor, float(np.abs(ref).max()))
    dist = float(np.abs(ref - ref32).max()) / scale
    bound = min(8.0 * max(dist, FLOOR), cap)
    err = float(np.abs(got - ref).max()) / scale
    print(f"GE2E_DIST {where} {name} err {err:.3e} f32_restatement {dist:.3e} bound {bound:.3e} max|ref| {np.abs(ref).max():.3e}")
    assert np.isfinite(got).all(), name
    assert err <= bound, f"{name}: {err:.3e} > {bound:.3e} (relative to {scale:.3e})"


def _where(d):
    return "gpu" if d.gpu else "emu"


# ---- 1. the loss kernels alone -----------------------------------------------------------------------------------------------------------
# (2, 2, 4): the smallest legal shape, the exclusive centroid is the other utterance; (2, 5, 12): one foreign column per row; (5, 3, 256): full
# width; (70, 4, 64): N over one wavefront and over four 16-speaker slabs, a partly filled last slab; (7, 64, 32): M at its limit.
SHAPES = [(2, 2, 4), (3, 2, 8), (2, 5, 12), (5, 3, 256), (70, 4, 64), (7, 64, 32)]
SCALARS = [(10.0, -5.0), (1.5, 0.25)]


def _unit_rows(g, rows, E):
    e = np.abs(g.standard_normal((rows, E))) + 1e-3
    return (e / np.linalg.norm(e, axis=1, keepdims=True)).astype(F32)


@functools.lru_cache(maxsize=None)
def _emb(N, M, E, kind="random"):
    g = np.random.RandomState(1000 * N + 10 * M + E)
    e = _unit_rows(g, N * M, E)
    if kind == "identical":      # every speaker's utterances are one vector: u is parallel to e, the projection of path (c) annihilates
        e = np.repeat(_unit_rows(g, N, E), M, axis=0)
    if kind == "clustered":      # speakers apart, utterances near their speaker: the three gradient paths are of one size (test 2c)
        centre = np.repeat(_unit_rows(g, N, E), M, axis=0)
        e = centre + 1.5 * _unit_rows(g, N * M, E)
        e = (e / np.linalg.norm(e, axis=1, keepdims=True)).astype(F32)
    return e


@functools.lru_cache(maxsize=None)
def _refs(N, M, E, w, b, kind="random"):
    e = _emb(N, M, E, kind)
    return GO.loss(e, N, M, w, b), GO.loss(e, N, M, w, b, dtype=torch.float32)


def _call(d, N, M, E, e, w, b, want_sim=True):
    P, lib = d.ptr, d.lib
    nbytes = int(lib.mtts_ge2e_ws_bytes(N, M, E))
    assert nbytes > 0
    ws = d.empty((nbytes + 3) // 4, fill=7)
    loss3, demb, sim = d.empty(3, fill=7), d.empty((N * M, E), fill=7), d.empty((N * M, N), fill=7)
    rc = lib.mtts_ge2e_loss(N, M, E, P(d.put(e)), w, b, P(loss3), P(demb), P(sim) if want_sim else None, P(ws), nbytes, None)
    assert rc == 0, lib.mtts_dvector_last_error(None).decode()
    return np.array(d.get(loss3)), np.array(d.get(demb)), np.array(d.get(sim))


def _compare(d, tag, got, ref, r32):
    loss3, demb, sim = got
    _close(_where(d), tag + ".L", loss3[0], ref["L"], r32["L"], CAP_VALUE, 1.0)
    _close(_where(d), tag + ".sim", sim, ref["sim"], r32["sim"], CAP_VALUE, 1.0)
    _close(_where(d), tag + ".dw_db", loss3[1:], [ref["dw"], ref["db"]], [r32["dw"], r32["db"]], CAP_GRAD)
    _close(_where(d), tag + ".demb", demb, ref["demb"], r32["demb"], CAP_GRAD)


@pytest.mark.parametrize("w,b", SCALARS)
@pytest.mark.parametrize("N,M,E", SHAPES)
def test_loss_and_gradients_against_float64_autograd(dev, N, M, E, w, b):
    ref, r32 = _refs(N, M, E, w, b)
    _compare(dev, f"loss[{N}x{M}x{E},w={w},b={b}]", _call(dev, N, M, E, _emb(N, M, E), w, b), ref, r32)


# ---- 2. the three gradient paths, separately ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M,E", SHAPES)
def test_flat_softmax(dev, N, M, E):
    """w = 1e-3: every softmax row is flat to 1e-3, so g is (1 / N - onehot) / (N M) and the paths are weighted by the shapes alone."""
    ref, r32 = _refs(N, M, E, 1e-3, 0.0)
    soft = np.exp(ref["sim"] - ref["sim"].max(axis=1, keepdims=True))
    assert np.abs(soft / soft.sum(axis=1, keepdims=True) - 1.0 / N).max() < 1e-3      # the precondition, on the oracle
    _compare(dev, f"flat[{N}x{M}x{E}]", _call(dev, N, M, E, _emb(N, M, E), 1e-3, 0.0), ref, r32)


@pytest.mark.parametrize("N,M,E", SHAPES)
def test_identical_utterances_annihilate_the_exclusive_path(dev, N, M, E):
    e = _emb(N, M, E, "identical")
    ref, r32 = _refs(N, M, E, 10.0, -5.0, "identical")
    only_c = GO.loss(e, N, M, 10.0, -5.0, detach=("a", "c"))["demb"]               # path (c) alone
    assert np.abs(only_c).max() <= 1e-12 * np.abs(ref["demb"]).max()                # the precondition, on the oracle
    _compare(dev, f"identical[{N}x{M}x{E}]", _call(dev, N, M, E, e, 10.0, -5.0), ref, r32)


@pytest.mark.parametrize("N,M,E", SHAPES[:-1] + [(7, 5, 32)])
def test_every_path_carries_a_tenth_of_the_gradient(dev, N, M, E):
    """The entry computes the whole loss (a single row's loss cannot be asked of it), so the paths are told apart by their size: on these
    inputs the oracle's contribution of each path alone — autograd with the other two detached — is at least 10 % of the total norm, and the
    three add up to the total.  A kernel that lost one of them, or weighted it wrongly, misses the bound by orders of magnitude.  The shapes
    are those of test 1 but for the last, where (7, 5, 32) stands in for (7, 64, 32): path (c) carries 1 / (M - 1) and the parts of a
    speaker's utterances perpendicular to their centroid cancel in its sum, so at M = 64 it is under 6 % of the norm on any inputs tried
    (w 3 .. 30, spread 0.6 .. 4); M at its limit is in the three tests above."""
    w, b = 3.0, 0.0
    e = _emb(N, M, E, "clustered")
    ref, r32 = _refs(N, M, E, w, b, "clustered")
    paths = {p: GO.loss(e, N, M, w, b, detach=tuple(sorted(set("acx") - {p})))["demb"] for p in "acx"}
    total = np.linalg.norm(ref["demb"])
    assert np.abs(sum(paths.values()) - ref["demb"]).max() <= 1e-12 * np.abs(ref["demb"]).max()
    share = {p: float(np.linalg.norm(v) / total) for p, v in paths.items()}
    print(f"GE2E_PATHS [{N}x{M}x{E}] a {share['a']:.3f} b {share['c']:.3f} c {share['x']:.3f}")
    assert min(share.values()) >= 0.10, share
    _compare(dev, f"paths[{N}x{M}x{E}]", _call(dev, N, M, E, e, w, b), ref, r32)


# ---- 3. determinism ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M,E", [(5, 3, 256), (70, 4, 64)])
def test_two_calls_give_the_same_bits(dev, N, M, E):
    e = _emb(N, M, E)
    a, c = _call(dev, N, M, E, e, 10.0, -5.0), _call(dev, N, M, E, e, 10.0, -5.0)
    for x, y in zip(a, c):
        assert np.array_equal(x, y)
    no_sim = _call(dev, N, M, E, e, 10.0, -5.0, want_sim=False)                      # the similarities are optional and change nothing else
    assert np.array_equal(no_sim[0], a[0]) and np.array_equal(no_sim[1], a[1]) and np.all(no_sim[2] == 7)


# ---- 4. refusals (host-side checks: the emulator build runs the same code) ---------------------------------------------------------------
def test_bad_arguments_are_refused_without_a_launch():
    d = Dev(False)
    P, lib = d.ptr, d.lib
    N, M, E = 3, 2, 8
    e = d.put(_emb(N, M, E))
    nbytes = int(lib.mtts_ge2e_ws_bytes(N, M, E))
    outs = [d.empty(3, fill=7), d.empty((4 * M * 2, 260), fill=7), d.empty((N * M, N), fill=7), d.empty((nbytes + 3) // 4, fill=7)]

    def refused(args, word):
        a = dict(n=N, m=M, E=E, w=10.0, ws=nbytes, demb=P(outs[1]))
        a.update(args)
        rc = lib.mtts_ge2e_loss(a["n"], a["m"], a["E"], P(e), a["w"], -5.0, P(outs[0]), a["demb"], P(outs[2]), P(outs[3]), a["ws"], None)
        msg = lib.mtts_dvector_last_error(None).decode()
        assert rc == -1 and msg.startswith("mtts_ge2e_loss: ") and word in msg, (args, msg)
        assert all(np.all(o == 7) for o in outs), args

    refused(dict(n=1), "n_spk")
    refused(dict(n=1025), "n_spk")
    refused(dict(m=1), "n_utt")
    refused(dict(m=65), "n_utt")
    refused(dict(E=6), "E ")
    refused(dict(E=260), "E ")
    refused(dict(w=0.0), "w ")
    refused(dict(w=float("inf")), "w ")
    refused(dict(ws=nbytes - 1), "ws_bytes")
    refused(dict(demb=None), "demb")
    assert lib.mtts_ge2e_ws_bytes(1, 2, 8) == 0 and lib.mtts_ge2e_ws_bytes(2, 2, 6) == 0
    assert lib.mtts_ge2e_loss(N, M, E, P(e), 10.0, -5.0, P(outs[0]), P(outs[1]), P(outs[2]), P(outs[3]), nbytes, None) == 0   # the template is a valid call


TINY = dict(n_mels=8, hidden=64, layers=2, emb=16)


def test_handle_refusals():
    enc = se.DVectorEncoder(se.synthetic_state_dict(1, **TINY), max_partials=8, max_utts=6, frames=6, lib_path=ge.build_emulator(), **TINY)
    lib, mels = enc.lib, np.zeros((8, 6, 8), F32)

    def fb(n, m):
        rc = lib.mtts_dvector_ge2e_forward_backward(enc.h, mels.ctypes.data_as(C.c_void_p), 0, n, m, None, None)
        return rc, lib.mtts_dvector_last_error(enc.h).decode()

    assert lib.mtts_dvector_ge2e_enable(enc.h, 10.0, -5.0) == -1                     # enable_training first
    assert "enable_training" in lib.mtts_dvector_last_error(enc.h).decode()
    enc.enable_training()
    assert fb(3, 2) == (-1, "mtts_dvector_ge2e_enable first")
    assert lib.mtts_dvector_ge2e_step(enc.h, 1e-4, 0.9, 0.999, 1e-8, 3.0, 0.01) == -1
    assert lib.mtts_dvector_ge2e_enable(enc.h, 0.0, -5.0) == -1 and "w " in lib.mtts_dvector_last_error(enc.h).decode()
    assert lib.mtts_dvector_ge2e_enable(enc.h, 10.0, -5.0) == 0
    rc, msg = fb(4, 2)
    assert rc == -1 and "max_utts" in msg
    rc, msg = fb(1, 2)
    assert rc == -1 and "n_spk" in msg
    rc, msg = fb(3, 1)
    assert rc == -1 and "n_utt" in msg
    assert lib.mtts_dvector_ge2e_step(enc.h, 1e-4, 0.9, 0.999, 1e-8, 3.0, 0.01) == -1   # nothing to apply
    assert "forward_backward" in lib.mtts_dvector_last_error(enc.h).decode()
    assert fb(3, 2)[0] == 0
    enc.close()


# ---- 5. the chained step against the oracle ----------------------------------------------------------------------------------------------
BIG = dict(n_mels=40, hidden=256, layers=3, emb=256)
# which -> (cfg, frames, N, M, weight seed, scale of the mels, w0, b0): the joint gradient norm of the oracle lies below max_norm = 3 in the
# "below" cases and above it in the "clipped" ones (asserted on the oracle; the gradient grows with the similarity scale w0, which is an input of the step like the mels)
CHAIN = {
    "emu-below": (TINY, 6, 3, 2, 5, 1.0, 2.0, -1.0),         # oracle norm 1.50
    "emu-clipped": (TINY, 6, 3, 2, 5, 1.0, 10.0, -5.0),      # 7.15
    "gpu-below": (BIG, 40, 8, 5, 7, 1.0, 10.0, -5.0),        # 0.026: random weights embed all utterances almost alike
    "gpu-clipped": (BIG, 40, 8, 5, 8, 1.0, 2000.0, -5.0),    # 8.75
}
MAX_NORM, SCALE, LR = 3.0, 0.01, 1e-4


@functools.lru_cache(maxsize=None)
def _chain_case(which):
    cfg, frames, N, M, seed, amp, w0, b0 = CHAIN[which]
    sd = se.synthetic_state_dict(seed, **cfg)
    mels = (amp * np.random.RandomState(seed + 100).standard_normal((N * M, frames, cfg["n_mels"]))).astype(F32)
    ref, r32 = GO.chain(sd, cfg, mels, N, M, w0, b0), GO.chain(sd, cfg, mels, N, M, w0, b0, dtype=torch.float32)
    steps = []
    for r, dt in ((ref, np.float64), (r32, np.float32)):
        params = dict({k: v for k, v in sd.items()}, w=np.array([w0]), b=np.array([b0]))
        grads = dict(r["grads"], w=np.array([r["dw"]]), b=np.array([r["db"]]))
        zeros = {k: np.zeros_like(np.asarray(v, np.float64)) for k, v in params.items()}
        steps.append(GO.trainer_step(params, grads, zeros, zeros, 1, lr=LR, max_norm=MAX_NORM, scalar_grad_scale=SCALE, dtype=dt))
    return sd, mels, ref, r32, steps


def _chain(which, lib_path):
    cfg, frames, N, M, seed, amp, w0, b0 = CHAIN[which]
    sd, mels, ref, r32, (st64, st32) = _chain_case(which)
    norm = st64[3]
    print(f"GE2E_NORM {which} joint gradient norm of the oracle {norm:.4f} (max_norm {MAX_NORM})")
    assert (norm > 1.2 * MAX_NORM) if which.endswith("clipped") else (norm < 0.8 * MAX_NORM)
    where = "gpu" if lib_path is None else "emu"
    enc = se.DVectorEncoder(sd, max_partials=N * M, max_utts=N * M, frames=frames, lib_path=lib_path, **cfg)
    tr = GE2ETrainer(enc, N, M, lr=LR, max_norm=MAX_NORM, scalar_grad_scale=SCALE, init_w=w0, init_b=b0)
    loss, sim = tr.forward_backward(mels, return_loss=True, return_sim=True)
    _close(where, f"chain[{which}].L", loss, ref["L"], r32["L"], CAP_VALUE, 1.0)
    _close(where, f"chain[{which}].sim", sim, ref["sim"], r32["sim"], CAP_VALUE, 1.0)
    _close(where, f"chain[{which}].dw_db", tr.scalars("grad"), [ref["dw"], ref["db"]], [r32["dw"], r32["db"]], CAP_GRAD)
    grads = {n: enc.export(n, 1) for n in sd}
    for n in sd:
        _close(where, f"chain[{which}].grad({n})", grads[n], ref["grads"][n], r32["grads"][n], CAP_GRAD)
    if lib_path is None:       # the same step from a stack that is already on the device: the same bits
        t = torch.from_numpy(mels).cuda()
        assert tr.forward_backward_device(t.data_ptr(), return_loss=True) == loss
        torch.cuda.synchronize()
        for n in sd:
            assert np.array_equal(enc.export(n, 1), grads[n]), n
    tr.step()
    wb = {k: tr.scalars(k) for k in ("value", "adam_m", "adam_v")}
    for i, (what, key) in enumerate((("param", "value"), ("adam_m", "adam_m"), ("adam_v", "adam_v"))):
        for n in sd:
            _close(where, f"step[{which}].{what}({n})", enc.export(n, (0, 2, 3)[i]), st64[i][n], st32[i][n], CAP_GRAD)
        pair = lambda st: [st[i]["w"][0], st[i]["b"][0]]             # (w, b) as one two-entry tensor: b's gradient is rounding noise alone
        _close(where, f"step[{which}].{what}(w_b)", wb[key], pair(st64), pair(st32), CAP_GRAD)
    assert tr.similarity_weight == wb["value"][0] and tr.similarity_bias == wb["value"][1]
    assert set(tr.encoder_state_dict()) == set(sd)                                     # w and b are not tensors of the encoder
    enc.close()


@pytest.mark.parametrize("which", ["emu-below", "emu-clipped"])
def test_chained_step_emulator(which):
    _chain(which, ge.build_emulator())


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["gpu-below", "gpu-clipped"])
def test_chained_step_gpu(which):
    ge.build_device()
    _chain(which, None)


# ---- 6. the existing backward is untouched -----------------------------------------------------------------------------------------------
def _backward_bits(lib_path, cfg, frames):
    sd = se.synthetic_state_dict(2, **cfg)
    enc = se.DVectorEncoder(sd, max_partials=12, max_utts=6, frames=frames, lib_path=lib_path, **cfg)
    enc.enable_training()
    g = np.random.RandomState(3)
    mels, slices = g.standard_normal((7, frames, cfg["n_mels"])).astype(F32), [slice(0, 2), slice(2, 3), slice(3, 7)]
    dout = g.standard_normal((3, cfg["emb"])).astype(F32)

    def run():
        out = enc.embed_train(mels, slices)
        enc.backward(dout)
        return [out] + [enc.export(n, 1) for n in sd]

    before = run()
    GE2ETrainer(enc, 3, 2).forward_backward(g.standard_normal((6, frames, cfg["n_mels"])).astype(F32))   # enables, and runs a GE2E pass in between
    for x, y in zip(before, run()):
        assert np.array_equal(x, y)
    enc.close()


def test_host_dout_backward_is_the_same_bits_after_ge2e_enable():
    _backward_bits(ge.build_emulator(), TINY, 6)


@pytest.mark.gpu
def test_host_dout_backward_is_the_same_bits_after_ge2e_enable_gpu():
    ge.build_device()
    _backward_bits(None, dict(n_mels=40, hidden=256, layers=3, emb=256), 20)


# ---- 7. training moves the right way -----------------------------------------------------------------------------------------------------
N_TRAIN, M_TRAIN, FRAMES, NOISE, TRAIN_SEED, TRAIN_STEPS, TRAIN_LR = 3, 2, 6, 0.3, 0, 40, 1e-2


def _synthetic_corpus(seed):
    """Four speakers: a fixed random spectral envelope each, plus per-frame noise."""
    g = np.random.RandomState(seed)
    env = g.standard_normal((4, TINY["n_mels"]))
    return {f"spk{k}": [(env[k] + NOISE * g.standard_normal((FRAMES + 4, TINY["n_mels"]))).astype(F32) for _ in range(4)] for k in range(4)}


def test_training_lowers_the_loss():
    sampler = SpeakerBatchSampler(_synthetic_corpus(TRAIN_SEED), N_TRAIN, M_TRAIN, FRAMES, seed=TRAIN_SEED)
    batches = [sampler.draw()[0] for _ in range(TRAIN_STEPS)]
    sd = se.synthetic_state_dict(9, **TINY)
    host = GO.Trainer(sd, TINY, N_TRAIN, M_TRAIN, lr=TRAIN_LR)
    ref = [host.train_step(m) for m in batches]
    ref_loss = [l for l, _ in ref]
    ref_eer = [batch_eer(s, N_TRAIN, M_TRAIN) for _, s in ref]
    print(f"GE2E_TRAIN oracle loss {ref_loss[0]:.4f} -> {ref_loss[-1]:.4f}, EER {ref_eer[0]:.3f} -> {ref_eer[-1]:.3f}")
    assert ref_loss[-1] < 0.25 * ref_loss[0] and ref_eer[-1] == 0.0                    # the precondition, on the oracle
    enc = se.DVectorEncoder(sd, max_partials=6, max_utts=6, frames=FRAMES, lib_path=ge.build_emulator(), **TINY)
    tr = GE2ETrainer(enc, N_TRAIN, M_TRAIN, lr=TRAIN_LR)
    got = [tr.train_step(m, return_eer=True) for m in batches]
    print(f"GE2E_TRAIN device loss {got[0][0]:.4f} -> {got[-1][0]:.4f}, EER {got[0][1]:.3f} -> {got[-1][1]:.3f}")
    assert abs(got[0][0] - ref_loss[0]) <= CAP_VALUE * max(1.0, ref_loss[0])           # the first step is the same problem; later ones drift apart
    assert got[0][1] == ref_eer[0]
    assert got[-1][0] < 0.5 * got[0][0]
    assert tr.steps == TRAIN_STEPS
    enc.close()


# ---- 8. checkpoint -----------------------------------------------------------------------------------------------------------------------
def test_checkpoint_continues_bit_identically():
    lib_path = ge.build_emulator()
    sampler = SpeakerBatchSampler(_synthetic_corpus(1), N_TRAIN, M_TRAIN, FRAMES, seed=1)
    batches = [sampler.draw()[0] for _ in range(4)]
    sd = se.synthetic_state_dict(9, **TINY)
    mk = lambda s: se.DVectorEncoder(s, max_partials=6, max_utts=6, frames=FRAMES, lib_path=lib_path, **TINY)
    enc = mk(sd)
    tr = GE2ETrainer(enc, N_TRAIN, M_TRAIN, lr=1e-3)
    for m in batches[:3]:
        tr.train_step(m)
    ck = {k: np.array(v) for k, v in tr.state_dict().items()}
    assert {"similarity_weight", "similarity_bias", "adam_m.similarity_weight", "adam_v.similarity_bias", "step", "adam_m.linear.weight"} <= set(ck)
    assert int(ck["step"][0]) == 3 and float(ck["similarity_weight"][0]) != 10.0
    enc2 = mk(None)
    tr2 = GE2ETrainer(enc2, N_TRAIN, M_TRAIN, lr=1e-3)
    tr2.load_state_dict(ck)
    a, b = tr.train_step(batches[3]), tr2.train_step(batches[3])
    assert a == b
    s1, s2 = tr.state_dict(), tr2.state_dict()
    assert set(s1) == set(s2)
    for k in s1:
        assert np.array_equal(s1[k], s2[k]), k
    # the encoder's part loads into a plain encoder, which embeds what the trainer's encoder embeds
    plain = mk(tr.encoder_state_dict())
    assert set(tr.encoder_state_dict()) == set(sd)
    slices = [slice(i, i + 1) for i in range(6)]
    assert np.array_equal(plain.embed(batches[0], slices), enc.embed(batches[0], slices))
    for e in (enc, enc2, plain):
        e.close()


def test_encoder_state_and_step_count_follow_the_trainer():
    """The encoder's own state_dict() is current after a step (exported on demand, not the weights it was created with), and an encoder that
    has already taken optimizer steps continues bit-identically from a checkpoint: handle, trainer and checkpoint hold one step count."""
    lib_path = ge.build_emulator()
    sampler = SpeakerBatchSampler(_synthetic_corpus(2), N_TRAIN, M_TRAIN, FRAMES, seed=2)
    batches = [sampler.draw()[0] for _ in range(3)]
    sd = se.synthetic_state_dict(9, **TINY)
    mk = lambda: se.DVectorEncoder(sd, max_partials=6, max_utts=6, frames=FRAMES, lib_path=lib_path, **TINY)
    enc = mk()
    enc.enable_training()
    enc.set_optimizer_step(5)                                    # an encoder with a history: GE2ETrainer(step=5) says so
    tr = GE2ETrainer(enc, N_TRAIN, M_TRAIN, lr=1e-3, step=5)
    tr.train_step(batches[0])
    now = enc.state_dict()                                       # the encoder's own method, not the trainer's
    assert all(np.array_equal(now[n], enc.export(n, 0)) for n in sd) and any(not np.array_equal(now[n], sd[n]) for n in sd)
    tr.train_step(batches[1])
    ck = {k: np.array(v) for k, v in tr.state_dict().items()}
    assert int(ck["step"][0]) == 7 and tr.steps == 7
    enc2 = mk()
    tr2 = GE2ETrainer(enc2, N_TRAIN, M_TRAIN, lr=1e-3)
    tr2.load_state_dict(ck)
    assert tr.train_step(batches[2]) == tr2.train_step(batches[2])
    s1, s2 = tr.state_dict(), tr2.state_dict()
    for k in s1:
        assert np.array_equal(s1[k], s2[k]), k
    fresh = mk()                                                 # the same two steps counted from 0: another bias correction, other weights
    tr3 = GE2ETrainer(fresh, N_TRAIN, M_TRAIN, lr=1e-3)
    tr3.train_step(batches[0])
    assert not np.array_equal(fresh.state_dict()["linear.weight"], now["linear.weight"])
    for e in (enc, enc2, fresh):
        e.close()


def test_mels_from_wavs_is_the_packed_front_end():
    from meta_tts_amd import evaluation as E
    emb = E.SpeakerEmbedder(lib_path=ge.build_emulator(), encoder=False)
    g = np.random.RandomState(4)
    wavs = [(0.1 * g.standard_normal(n)).astype(F32) for n in (1600, 2405)]
    mels = mels_from_wavs(emb, wavs)
    ref = emb.wav_to_mel_spectrogram(wavs)
    assert [m.shape for m in mels] == [(n // 160 + 1, 40) for n in (1600, 2405)]
    for m, r in zip(mels, ref):
        assert m.dtype == F32 and m.flags["C_CONTIGUOUS"] and np.array_equal(m, r)
    SpeakerBatchSampler({"a": mels, "b": mels}, 2, 2, 8).draw()   # what the sampler is fed
    emb.close()


# ---- 9. sampler --------------------------------------------------------------------------------------------------------------------------
def test_sampler():
    g = np.random.RandomState(0)
    corpus = {f"s{k}": [np.full((int(g.randint(6, 15)), 4), 100 * k + u, F32) for u in range(5)] for k in range(6)}
    for k in corpus:                                   # mark every frame with its own index, so a window can be located
        for mel in corpus[k]:
            mel[:, 1] = np.arange(mel.shape[0])
    a, b = SpeakerBatchSampler(corpus, 4, 3, 6, seed=5), SpeakerBatchSampler(corpus, 4, 3, 6, seed=5)
    other = SpeakerBatchSampler(corpus, 4, 3, 6, seed=6)
    same, differs = True, False
    for _ in range(5):
        (ma, pa), (mb, pb), (mo, _) = a.draw(), b.draw(), other.draw()
        same &= np.array_equal(ma, mb) and pa == pb
        differs |= not np.array_equal(ma, mo)
        assert ma.shape == (12, 6, 4) and ma.dtype == F32
        spk = [p[0] for p in pa]
        assert spk == [s for s in spk[::3] for _ in range(3)] and len(set(spk[::3])) == 4          # speaker-major, distinct speakers
        for j in range(4):
            assert len({p[1] for p in pa[3 * j:3 * j + 3]}) == 3                                     # distinct utterances
        for row, (s, u, t0) in zip(ma, pa):
            mel = a.usable[s][u]
            assert 0 <= t0 <= mel.shape[0] - 6 and np.array_equal(row, mel[t0:t0 + 6])               # the window lies inside its utterance
            assert np.all(row[:, 0] == mel[0, 0]) and np.array_equal(row[:, 1], np.arange(t0, t0 + 6))
    assert same and differs
    with pytest.raises(ValueError, match="6 speakers"):
        SpeakerBatchSampler(corpus, 7, 3, 6)
    short = dict(corpus, s3=corpus["s3"][:2] + [np.zeros((5, 4), F32)] * 3)
    with pytest.raises(ValueError, match="speaker s3 "):
        SpeakerBatchSampler(short, 4, 3, 6)
