"""Kernel-level C-ABI entries of the d-vector speaker encoder — csrc/dvector.h: lstm_recurrent / lstm_bptt, dvec_head / dvec_head_bwd,
dvec_utterance / dvec_utterance_bwd — against the float64 restatement of dvector_kernel_oracle.py on the same seeded float32 inputs.  As in
test_kernel_entries.py every test runs twice: through the SIMT emulator on the CPU and, marked gpu, through libmtts.so on the MI355X.  The
entries go through the launchers DVector::forward / backward use (test_row_launchers.py), so what is pinned here is the product's launch.

Tolerances are not chosen (the rule of test_tangent_entries.py): for every output the bound is 8 x the distance between the float64 reference
and the same reference evaluated in float32 on the same inputs, relative to max(1, max|ref|), and never looser than the 2e-5 of the
kernel-entry tests.  Every comparison prints a DVEC_DIST line (err, f32_restatement, bound, max|ref|) before it asserts.

Shapes are the smallest at which a path exists: H = 64 (one wavefront) .. 1024 (the whole 2 * 1024 / 4 * 1024-float LDS arrays), T = 1 (no
recurrence, c_prev = 0), even and odd T (which of the two LDS state buffers the last step wrote), E = 4 / 100 / 68 (a partly filled last
wavefront: the j < E guards and the per-wavefront partial sums), one and several partials per utterance.

The bounds are a few 1e-7: the kernels meet them because the recurrent dot products are added in partial sums of 32 terms (not H or 4H terms
one after the other) and the head accumulates in float64 — with serial float32 sums the H = 1024 cases and the four-output head miss them."""
import functools

import numpy as np
import pytest
import torch

import dvector_kernel_oracle as KO
from oracle_util import Dev
from test_kernel_entries import dev  # noqa: F401  (the emu / gpu fixture)

F32 = np.float32
CAP = 2e-5


def _close(dev, name, got, ref, ref32, cap=CAP):
    """|got - ref| against the bound derived from the float32 restatement (module docstring); prints the figures before it asserts."""
    got = np.asarray(got, np.float64).reshape(ref.shape)
    scale = max(1.0, float(np.abs(ref).max()))
    dist = float(np.abs(ref - ref32).max()) / scale
    bound = min(8.0 * dist, cap)
    err = float(np.abs(got - ref).max()) / scale
    print(f"DVEC_DIST {'gpu' if dev.gpu else 'emu'} {name} err {err:.3e} f32_restatement {dist:.3e} bound {bound:.3e} max|ref| {np.abs(ref).max():.3e}")
    assert np.isfinite(got).all(), name
    assert err <= bound, f"{name}: {err:.3e} > {bound:.3e} (relative to max(1, max|ref|) = {scale:.3e})"


def _randn(g, *shape):
    return g.standard_normal(shape).astype(F32)


# ---- lstm_recurrent -> lstm_bptt ---------------------------------------------------------------------------------------------------------
# (1, 1, 64): no recurrence, only h0; (3, 2, 64): even T; (2, 7, 128): odd T, two wavefronts; (5, 4, 256); (2, 3, 1024): a full workgroup.
LSTM_SHAPES = [(1, 1, 64), (3, 2, 64), (2, 7, 128), (5, 4, 256), (2, 3, 1024)]
LSTM_MODES = {"top": (False, True), "middle": (True, False), "single": (True, True)}   # mode -> (dh_ext given, dh_last given)
SAT_OFFSET = 120.0   # |x| > 88: expf(-x) overflows to inf on one side and underflows to 0 on the other


def _saturation(N, T, H):
    """+-120 on all four gates of every fourth hidden unit (j % 4 == 1), the sign alternating with the unit and the gate."""
    add = np.zeros((N, T, 4 * H), F32)
    for q in range(4):
        for j in range(1, H, 4):
            add[:, :, q * H + j] = SAT_OFFSET if (j // 4 + q) % 2 == 0 else -SAT_OFFSET
    return add


@functools.lru_cache(maxsize=None)
def _lstm_case(N, T, H, mode, saturated=False):
    g = np.random.RandomState(7919 * H + 31 * T + N)
    xp = _randn(g, N, T, 4 * H)
    if saturated:
        xp = xp + _saturation(N, T, H)
    whh = (_randn(g, 4 * H, H) / np.sqrt(H)).astype(F32)   # 1 / sqrt(H): the states stay O(1)
    ext, last = LSTM_MODES[mode]
    i = dict(xp=xp, whh=whh, whhT=np.ascontiguousarray(whh.T), dh_ext=_randn(g, N, T, H) if ext else None, dh_last=_randn(g, N, H) if last else None)
    args = (i["xp"], i["whh"], i["dh_ext"], i["dh_last"])
    return i, KO.lstm_layer(*args), KO.lstm_layer(*args, dtype=torch.float32)


def _run_lstm(dev, N, T, H, mode, saturated=False, compare=True):
    i, ref, r32 = _lstm_case(N, T, H, mode, saturated)
    P, lib = dev.ptr, dev.lib
    xp, whhT, whh = dev.put(i["xp"]), dev.put(i["whhT"]), dev.put(i["whh"])
    opt = lambda k: P(dev.put(i[k])) if i[k] is not None else None
    gates, cseq, hprev = dev.empty((N, T, 4 * H), fill=5), dev.empty((N, T, H), fill=5), dev.empty((N, T, H), fill=5)
    hseq, hlast, dgates = dev.empty((N, T, H), fill=5), dev.empty((N, H), fill=5), dev.empty((N, T, 4 * H), fill=5)
    # gates / cseq go from kernel to kernel on the device, as in DVector
    assert lib.mtts_lstm_recurrent(N, T, H, P(xp), P(whhT), P(hseq), P(hlast), P(gates), P(cseq), P(hprev), None) == 0
    assert lib.mtts_lstm_bptt(N, T, H, P(gates), P(cseq), opt("dh_ext"), opt("dh_last"), P(whh), P(dgates), None) == 0
    got = {k: np.array(dev.get(v)) for k, v in dict(gates=gates, cseq=cseq, hprev=hprev, hseq=hseq, hlast=hlast, dgates=dgates).items()}
    tag = f"lstm[{N}x{T}x{H},{mode}{',saturated' if saturated else ''}]"
    for k in ("gates", "cseq", "hprev", "hseq", "hlast", "dgates") if compare else ():
        _close(dev, f"{tag}.{k}", got[k], ref[k], r32[k])
    assert np.all(got["hprev"][:, 0] == 0)                                             # the state before the first step
    assert np.array_equal(got["hprev"][:, 1:], got["hseq"][:, :-1])                    # bit for bit: one register, stored twice
    assert np.array_equal(got["hlast"], got["hseq"][:, -1])
    return i, ref, got, (xp, whhT)


@pytest.mark.parametrize("mode", sorted(LSTM_MODES))
@pytest.mark.parametrize("N,T,H", LSTM_SHAPES)
def test_lstm_recurrent_then_bptt(dev, N, T, H, mode):
    _run_lstm(dev, N, T, H, mode)


@pytest.mark.parametrize("N,T,H", LSTM_SHAPES)
def test_lstm_inference_launch_gives_the_same_final_state(dev, N, T, H):
    """gates / cseq / hprev / hseq all null (the top layer of DVector's frozen forward): the same hlast, bit for bit."""
    i, ref, got, (xp, whhT) = _run_lstm(dev, N, T, H, "top", compare=False)   # (compared in the test above)
    hlast = dev.empty((N, H), fill=5)
    assert dev.lib.mtts_lstm_recurrent(N, T, H, dev.ptr(xp), dev.ptr(whhT), None, dev.ptr(hlast), None, None, None, None) == 0
    assert np.array_equal(dev.get(hlast), got["hlast"])


def test_lstm_saturated_gates(dev):
    """Pre-activations of +-120 on a quarter of the units: dv_sigmoid's expf(-x) overflows to inf (x < -88) or underflows to 0.  Nothing may
    turn NaN or infinite, the gates are exactly 0 / 1 (+-1 for g) wherever the float64 reference rounds to that in float32, and the gradient
    of such a pre-activation is exactly 0."""
    N, T, H = 2, 7, 128
    i, ref, got, _ = _run_lstm(dev, N, T, H, "single", saturated=True)
    for k, v in got.items():
        assert np.isfinite(v).all(), k
    sat = _saturation(N, T, H) != 0
    assert sat.mean() == 0.25
    want = ref["gates"].astype(F32)
    assert np.all(np.isin(want[sat], (0.0, 1.0, -1.0)))            # (the reference itself rounds to the limits on every offset entry)
    assert set(np.unique(want[sat])) == {0.0, 1.0, -1.0}
    assert np.array_equal(got["gates"][sat], want[sat])
    assert np.all(got["dgates"][sat] == 0)
    assert np.abs(got["dgates"][~sat]).max() > 1e-3                # (the other units still carry a gradient)


# ---- dvec_head -> dvec_head_bwd ----------------------------------------------------------------------------------------------------------
# E = 4: one wavefront with 60 idle lanes; 64: exactly one; 100: two, the second partly filled; 256: four full; 68 with H = 1024: 128 threads
# stage 1024 hidden values and write 1024 columns of dh_last.
HEAD_SHAPES = [(1, 64, 4), (3, 64, 64), (2, 128, 100), (4, 256, 256), (2, 1024, 68)]
KINK = 1e-4   # no pre-activation of the ReLU this close to 0: float32 and float64 then agree on which units are dead


@functools.lru_cache(maxsize=None)
def _head_case(N, H, E, dead_row):
    """Biases of the spread of W h, so about half of the units are dead.  dead_row: one more row n = N whose units are ALL dead — hidden unit 0
    carries a weight of -50 to every output and is 1 in that row only (0 in the others, which therefore do not see it).  The seed moves on
    until no pre-activation lies within KINK of the ReLU's kink (a property of the inputs, checked on the float64 reference)."""
    for seed in range(100 * H + E, 100 * H + E + 50):
        g = np.random.RandomState(seed)
        rows = N + (1 if dead_row else 0)
        hlast = np.tanh(_randn(g, rows, H)).astype(F32)             # hidden states lie in (-1, 1)
        w = (_randn(g, E, H) / np.sqrt(H)).astype(F32)
        bias = (0.6 * _randn(g, E)).astype(F32)
        if dead_row:
            hlast[:, 0] = 0
            hlast[N, 0] = 1
            w[:, 0] = -50
        dpart = _randn(g, rows, E)
        ref = KO.head(hlast, w, bias, dpart)
        if np.abs(ref["z"]).min() > KINK and (ref["z"][:N] > 0).any(axis=1).all():   # (and every ordinary row keeps a live unit)
            break
    else:
        raise AssertionError("no seed keeps the pre-activations away from the kink")
    i = dict(hlast=hlast, w=w, wT=np.ascontiguousarray(w.T), bias=bias, dpart=dpart)
    return i, ref, KO.head(hlast, w, bias, dpart, dtype=torch.float32)


@pytest.mark.parametrize("dead_row", [False, True], ids=["", "dead_row"])
@pytest.mark.parametrize("N,H,E", HEAD_SHAPES)
def test_dvec_head_then_backward(dev, N, H, E, dead_row):
    i, ref, r32 = _head_case(N, H, E, dead_row)
    rows = N + (1 if dead_row else 0)
    P, lib = dev.ptr, dev.lib
    d = {k: dev.put(v) for k, v in i.items()}
    part, eraw, dz, dh = dev.empty((rows, E), fill=5), dev.empty((rows, E), fill=5), dev.empty((rows, E), fill=5), dev.empty((rows, H), fill=5)
    assert lib.mtts_dvec_head(rows, H, E, P(d["hlast"]), P(d["wT"]), P(d["bias"]), P(part), P(eraw), None) == 0
    assert lib.mtts_dvec_head_bwd(rows, H, E, P(eraw), P(d["dpart"]), P(d["w"]), P(dz), P(dh), None) == 0
    got = {k: np.array(dev.get(v)) for k, v in dict(part=part, eraw=eraw, dz=dz, dh_last=dh).items()}
    dead = ref["z"] <= 0
    if E >= 64:
        assert 0.3 < dead[:N].mean() < 0.7
    tag = f"head[{N}x{H}x{E}{',dead_row' if dead_row else ''}]"
    for k in ("part", "eraw", "dz", "dh_last"):
        _close(dev, f"{tag}.{k}", got[k][:N], ref[k][:N], r32[k][:N])
    assert np.all(got["dz"][dead] == 0) and np.all(got["eraw"][dead] == 0)
    np.testing.assert_allclose(np.linalg.norm(got["part"][:N].astype(np.float64), axis=1), 1.0, atol=1e-6)
    if dead_row:
        # raw / ||raw|| = 0 / 0: NaN in the reference and in the kernel, in that row alone (the comparisons above saw the other rows)
        assert dead[N].all() and np.isnan(ref["part"][N]).all()
        assert np.isnan(got["part"][N]).all()
        assert np.all(got["eraw"][N] == 0) and np.all(got["dz"][N] == 0) and np.all(got["dh_last"][N] == 0)   # nothing passes a dead ReLU
        # an inference launch (no eraw) gives the same rows
        part2 = dev.empty((rows, E), fill=5)
        assert lib.mtts_dvec_head(rows, H, E, P(d["hlast"]), P(d["wT"]), P(d["bias"]), P(part2), None, None) == 0
        assert np.array_equal(np.array(dev.get(part2))[:N], got["part"][:N])


# ---- dvec_utterance -> dvec_utterance_bwd ------------------------------------------------------------------------------------------------
UTT_OFFSETS = {"one": [0, 1], "ragged": [0, 1, 4, 6], "two": [0, 3, 4]}


@functools.lru_cache(maxsize=None)
def _utt_case(E, which, cancel):
    """Random partials (the entries take arbitrary inputs: not unit vectors, not non-negative).  cancel: one more utterance of two partials p
    and -p, whose mean is an exact zero — the nrm <= 1e-12 branch of both kernels."""
    g = np.random.RandomState(17 * E + len(which))
    off = list(UTT_OFFSETS[which])
    part = _randn(g, off[-1], E)
    if cancel:
        p = _randn(g, 1, E)
        part = np.concatenate([part, p, -p])
        off.append(off[-1] + 2)
    off = np.asarray(off, np.int32)
    dout = _randn(g, len(off) - 1, E)
    return dict(part=part, off=off, dout=dout), KO.utterance(part, off, dout), KO.utterance(part, off, dout, dtype=torch.float32)


@pytest.mark.parametrize("cancel", [False, True], ids=["", "zero_mean"])
@pytest.mark.parametrize("which", sorted(UTT_OFFSETS))
@pytest.mark.parametrize("E", [4, 100, 256])
def test_dvec_utterance_then_backward(dev, E, which, cancel):
    i, ref, r32 = _utt_case(E, which, cancel)
    B, n = len(i["off"]) - 1, int(i["off"][-1])
    P, lib = dev.ptr, dev.lib
    d = {k: dev.put(v) for k, v in i.items()}
    out, dpart = dev.empty((B, E), fill=5), dev.empty((n, E), fill=5)
    assert lib.mtts_dvec_utterance(B, E, P(d["part"]), P(d["off"]), P(out), None) == 0
    assert lib.mtts_dvec_utterance_bwd(B, E, P(d["part"]), P(d["off"]), P(d["dout"]), P(dpart), None) == 0
    got_out, got_dp = np.array(dev.get(out)), np.array(dev.get(dpart))
    Bn, nn = (B - 1, n - 2) if cancel else (B, n)          # the ordinary utterances and their partials
    tag = f"utterance[E={E},{which}{',zero_mean' if cancel else ''}]"
    _close(dev, tag + ".out", got_out[:Bn], ref["out"][:Bn], r32["out"][:Bn])
    _close(dev, tag + ".dpart", got_dp[:nn], ref["dpart"][:nn], r32["dpart"][:nn])
    np.testing.assert_allclose(np.linalg.norm(got_out[:Bn].astype(np.float64), axis=1), 1.0, atol=1e-6)
    if cancel:
        assert np.all(got_out[Bn] == 0) and np.all(ref["out"][Bn] == 0)
        # F.normalize's clamp: d out / d mean = 1 / 1e-12, and the mean's 1 / count (values of 1e12: compared on their own, the bound is relative)
        want = np.repeat(i["dout"][Bn:].astype(np.float64) / 1e-12 / 2, 2, axis=0)
        assert np.abs(ref["dpart"][nn:] - want).max() <= 1e-12 * np.abs(want).max()
        _close(dev, tag + ".dpart(zero mean)", got_dp[nn:], ref["dpart"][nn:], r32["dpart"][nn:])


# ---- refusals (host-side argument checks: the emulator build runs the same code) --------------------------------------------------------------
BAD_H = (0, -64, 32, 63, 65, 100, 1088, 2048)
BAD_E = (0, -4, 2, 3, 6, 101, 258, 260, 512)
# name -> (argument template: ints as they are, "i" an input pointer, "o" an output pointer; positions that may be null; position of H, of E)
ENTRIES = {
    "mtts_lstm_recurrent": ([2, 3, 64, "i", "i", "o", "o", "o", "o", "o"], {5, 7, 8, 9}, 2, None),
    "mtts_lstm_bptt": ([2, 3, 64, "i", "i", "i", "i", "i", "o"], {5, 6}, 2, None),
    "mtts_dvec_head": ([2, 64, 8, "i", "i", "i", "o", "o"], {7}, 1, 2),
    "mtts_dvec_head_bwd": ([2, 64, 8, "i", "i", "i", "o", "o"], set(), 1, 2),
    "mtts_dvec_utterance": ([2, 8, "i", "off", "o"], set(), None, 1),
    "mtts_dvec_utterance_bwd": ([2, 8, "i", "off", "i", "o"], set(), None, 1),
}
SENTINEL = 5.0


def _refusals(dev, name):
    template, optional, h_at, e_at = ENTRIES[name]
    fn = getattr(dev.lib, name)
    outs = []

    def arg(v):
        if v == "off":
            return dev.ptr(dev.put(np.array([0, 1, 2], np.int32)))
        if v == "i":
            return dev.ptr(dev.put(np.full(2 * 3 * 4 * 64, 0.25, F32)))
        if v == "o":
            outs.append(dev.empty(2 * 3 * 4 * 64, fill=SENTINEL))
            return dev.ptr(outs[-1])
        return v
    good = [arg(v) for v in template] + [None]                        # (the stream)

    def refused(args, why):
        assert fn(*args) == -1, f"{name}: {why}"
        assert all(np.all(o == SENTINEL) for o in outs), f"{name}: {why} wrote an output"

    def with_(k, v):
        return [v if j == k else a for j, a in enumerate(good)]
    for k, v in enumerate(template):
        if isinstance(v, str) and k not in optional:
            refused(with_(k, None), f"argument {k} null")
    refused(with_(0, 0), "N / B = 0")
    refused(with_(0, -1), "N / B < 0")
    if h_at is not None:
        for h in BAD_H:
            refused(with_(h_at, h), f"H = {h}")
    if e_at is not None:
        for e in BAD_E:
            refused(with_(e_at, e), f"E = {e}")
    if name.startswith("mtts_lstm"):
        refused(with_(1, 0), "T = 0")
        refused(with_(1, -3), "T < 0")
    if name == "mtts_lstm_recurrent":                                # gates / cseq / hprev: all three or none
        for keep in ((7,), (8,), (9,), (7, 8), (7, 9), (8, 9)):
            refused([None if (j in (7, 8, 9) and j not in keep) else a for j, a in enumerate(good)], f"training arrays {keep} only")
    assert fn(*good) == 0, name                                      # the template itself is a valid call ...
    assert not any(np.all(o == SENTINEL) for o in outs), name        # ... that writes every output


def test_bad_arguments_are_refused_without_a_launch():
    dev = Dev(False)
    for name in sorted(ENTRIES):
        _refusals(dev, name)
