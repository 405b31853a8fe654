"""Attention forward and backward in the layout the engine launches (engine.h: fft_fwd / fft_bwd) through mtts_attn_packed_fwd / _bwd: every
(sequence, head) of ragged lengths in ONE launch sized by the longest, Q / K / V as column slices of one [rows][3 d] buffer, O as a slice of
[rows][d], sequences at arbitrary row offsets, the P matrices packed back to back — with the plan's own descriptors (attn_group_descs) and
against a plain float64 numpy reference per (sequence, head):
    S = Q K^T / sqrt(dk), P = softmax(S), O = P V;  dV = P^T dO, dP = dO V^T, dS = P o (dP - rowsum(dP o P)) / sqrt(dk), dQ = dS K, dK = dS^T Q
(the backward is fed the device's own P, as in the engine, and so is its reference).  Each case runs path 0 (the engine's route: the fused
kernel where it serves the launch) and path 1 (GEMM, softmax, GEMM) in both row layouts: sequences G + i (max_len + G) with guard rows, and
back to back, where a read past L that is used lands in the next sequence's data.

What makes it bite: guard rows of qkv and dO hold 1e30 (the engine's hold bias values, not zeros); O and gqkv are prefilled with 7.0 and every
row outside a sequence must still hold it; P and dS are prefilled with NaN.  The NaN prefill is the entry's contract, not a relaxation
(include/mtts.h): the pad columns [L, ldS) of P are written, zero, by the softmax of either path (attention.h phase B: `c < ldS`;
rowops.h: softmax_fwd_kernel stores v = 0 for L <= c < ldS) and those of dS by softmax_bwd_kernel, BEFORE the NN products that read whole
float4s of a row (O = P V, dQ = dS K: the last K-slice loads up to (K + 3) & ~3) — so nothing depends on what the buffers held; the test
checks the zeros as well.

Gates.  Unit-normal inputs: the forward keeps tests/test_kernel_entries.py's 3e-6 on P and 2e-5 on O.  The backward tensors and the
large-logit variants: max(4 err32, 8 eps32 max|ref|) per tensor and case, err32 = max abs error of the same formulas in float32 torch on the
CPU against the float64 reference on the same inputs (4: a sequential MFMA chain of length dk or L <= 1025 against torch's blocked sums).

Observed err_kernel / err32 (worst of the two layouts and the two paths; emulator / MI355X):
case                     P             O            dS            dQ            dK            dV
h2dk16         1.10 / 1.28   1.01 / 1.10   1.67 / 0.98   1.74 / 1.13   1.00 / 1.00   1.00 / 1.00
h2dk32         0.86 / 0.89   1.09 / 1.10   1.07 / 1.36   1.00 / 1.00   1.28 / 1.21   1.00 / 1.34
h1dk64         0.66 / 0.92   0.97 / 0.99   1.15 / 0.74   1.00 / 1.28   1.06 / 1.19   1.00 / 1.68
h1dk128        2.06 / 1.49   2.64 / 1.66   0.38 / 0.76   1.45 / 1.42   1.32 / 1.32   1.32 / 1.03
h2dk16_L1025   1.24 / 2.04   1.35 / 2.43   1.00 / 1.61   1.10 / 2.07   1.65 / 2.28   2.06 / 1.74
h2dk24         1.00 / 2.08   1.00 / 1.35   1.21 / 1.98   0.88 / 1.07   1.16 / 1.00   1.00 / 0.95
h2dk16_big     1.00 / 1.35   1.00 / 0.94   0.78 / 0.64   0.75 / 0.88   0.54 / 0.56   1.00 / 1.00
h2dk32_big     1.33 / 1.33   1.06 / 1.12   1.00 / 1.00   0.88 / 0.90   0.99 / 0.98   1.00 / 0.93
(the two forward routes came out bit-identical on both arms in every case; P and O of the unit-normal cases are gated by the fixed
tolerances above, their ratios are listed for comparison.)  Every case runs on both arms: the slowest emulator case (h1dk128) takes 2.2 s,
the whole file 18 s on the emulator and under 2 s on the MI355X.
"""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from test_kernel_entries import Dev

G = 4
EPS32 = float(np.finfo(np.float32).eps)
SENTINEL = np.float32(1e30)

# name: (heads, dk, lens in this order)
CASES = {
    "h2dk16": (2, 16, (33, 1, 128, 31, 32, 65, 64)),   # the 128 tile class; 1-4 key chunks (wavefronts without a chunk in phase A); query tiles that return early; dk < 32
    "h2dk32": (2, 32, (129, 7, 352, 200)),             # the 352 class and its edge; 11 chunks (the c += 8 loop wraps); one odd trip each of chunk and block
    "h1dk64": (1, 64, (353, 608, 40)),                 # the 608 class on both edges
    "h1dk128": (1, 128, (609, 1024, 3)),               # the 1024 class, NJ = 16
    "h2dk16_L1025": (2, 16, (1025, 20)),               # beyond attn_fused_ok: path 0 falls back to the three launches
    "h2dk24": (2, 24, (50, 9)),                        # a head width that is not fused
    # large-logit variants: q scaled until the largest logit exceeds exp's fp32 range, plus one sequence of 37 equal keys (uniform rows)
    "h2dk16_big": (2, 16, (33, 1, 128, 31, 32, 65, 64, 37)),
    "h2dk32_big": (2, 32, (129, 7, 352, 200, 37)),
}
FWD_ATOL = {"P": 3e-6, "O": 2e-5}   # unit-normal inputs (tests/test_kernel_entries.py: test_sdpa_and_softmax)


def _groups(heads, lens):
    """(sequence, head, L, ldS, offset of the group's matrix in P / dS) in group order n = seq * heads + head"""
    out, so = [], 0
    for i, L in enumerate(lens):
        ldS = (L + 3) & ~3
        for hh in range(heads):
            out.append((i, hh, L, ldS, so))
            so += L * ldS
    return out, so


def _t32(x):
    return torch.from_numpy(np.array(x, dtype=np.float32))   # (a copy: the cached inputs are read-only)


@functools.lru_cache(maxsize=None)
def case_data(name):
    """Per-sequence inputs of a case and its forward references (float64, and float32 torch for err32): computed once, shared by both layouts
    and both arms, never modified."""
    heads, dk, lens = CASES[name]
    big = name.endswith("_big")
    d = heads * dk
    g = np.random.RandomState(zlib.crc32(name.encode()) & 0x7fffffff)
    qkv = [g.standard_normal((L, 3 * d)).astype(np.float32) for L in lens]
    dO = [g.standard_normal((L, d)).astype(np.float32) for L in lens]
    groups, _ = _groups(heads, lens)
    sl = lambda i, blk, hh: qkv[i][:, blk * d + hh * dk: blk * d + (hh + 1) * dk]
    if big:
        qkv[-1][:, d:2 * d] = qkv[-1][0, d:2 * d]   # the last sequence: equal keys
        top = max(float((sl(i, 0, hh).astype(np.float64) @ sl(i, 1, hh).astype(np.float64).T).max()) for i, hh, *_ in groups) / np.sqrt(dk)
        for x in qkv:
            x[:, :d] *= np.float32(120.0 / top)
    P64, O64, e32, mx, top_logit = [], [], {"P": 0.0, "O": 0.0}, {"P": 0.0, "O": 0.0}, -np.inf
    for i, hh, L, ldS, so in groups:
        q, k, v = (sl(i, b, hh).astype(np.float64) for b in range(3))
        S = q @ k.T / np.sqrt(dk)
        top_logit = max(top_logit, float(S.max()))
        E = np.exp(S - S.max(axis=1, keepdims=True))
        P = E / E.sum(axis=1, keepdims=True)
        O = P @ v
        tq, tk, tv = (_t32(sl(i, b, hh)) for b in range(3))
        tP = torch.softmax(tq @ tk.T / np.sqrt(dk), dim=1)
        tO = tP @ tv
        for t, ref, got in (("P", P, tP), ("O", O, tO)):
            e32[t] = max(e32[t], float(np.abs(got.numpy() - ref).max()))
            mx[t] = max(mx[t], float(np.abs(ref).max()))
        P64.append(P); O64.append(O)
    for x in qkv + dO:
        x.setflags(write=False)
    return dict(heads=heads, dk=dk, lens=lens, qkv=qkv, dO=dO, groups=groups, P64=P64, O64=O64, e32=e32, mx=mx, top_logit=top_logit, big=big)


def backward_refs(cd, qkv_of, P_dev, dO_of):
    """float64 reference and float32-torch yardstick of the backward for the device's own probabilities: per group (dS, dQ, dK, dV) in float64,
    err32 and max|ref| per tensor over the case."""
    dk = cd["dk"]
    refs, e32, mx = [], dict.fromkeys(("dS", "dQ", "dK", "dV"), 0.0), dict.fromkeys(("dS", "dQ", "dK", "dV"), 0.0)
    for n, (i, hh, L, ldS, so) in enumerate(cd["groups"]):
        q, k, v = (qkv_of(i, b, hh) for b in range(3))
        do, p = dO_of(i, hh), P_dev[n]

        def chain(q, k, v, do, p, sqrt_dk):   # numpy float64 or torch float32: the same expressions
            dV = p.T @ do
            dP = do @ v.T
            dS = p * (dP - (dP * p).sum(1)[:, None]) / sqrt_dk
            return dS, dS @ k, dS.T @ q, dV

        r64 = chain(*(x.astype(np.float64) for x in (q, k, v, do, p)), np.sqrt(dk))
        r32 = chain(*(_t32(x) for x in (q, k, v, do, p)), float(np.sqrt(dk)))
        for t, a, b in zip(("dS", "dQ", "dK", "dV"), r64, r32):
            e32[t] = max(e32[t], float(np.abs(b.numpy() - a).max()))
            mx[t] = max(mx[t], float(np.abs(a).max()))
        refs.append(r64)
    return refs, e32, mx


def _layout(lens, kind):
    if kind == "guard":    # the encoder's rectangle: G guard rows before, between and after
        m = max(lens)
        return [G + i * (m + G) for i in range(len(lens))], G + len(lens) * (m + G)
    row0 = [int(x) for x in np.cumsum((0,) + tuple(lens[:-1]))]   # back to back, no gap (G sentinel rows close the buffer)
    return row0, sum(lens) + G


def _params():
    for name in CASES:
        for kind in ("guard", "packed"):
            for gpu in (False, True):
                yield pytest.param(name, kind, gpu, id=f"{name}-{kind}-{'gpu' if gpu else 'emu'}", marks=[pytest.mark.gpu] if gpu else [])


@pytest.mark.parametrize("name,kind,gpu", list(_params()))
def test_packed_attention_fwd_bwd(name, kind, gpu):
    if gpu:
        ge.build_device()
    dev = Dev(gpu)
    cd = case_data(name)
    heads, dk, lens, groups = cd["heads"], cd["dk"], cd["lens"], cd["groups"]
    d, n_seq = heads * dk, len(lens)
    if cd["big"]:
        assert cd["top_logit"] > 89.0   # beyond exp's fp32 range: only the max-subtraction keeps the softmax finite
    row0, rows = _layout(lens, kind)
    qkv = np.full((rows, 3 * d), SENTINEL, np.float32)
    dO = np.full((rows, d), SENTINEL, np.float32)
    inseq = np.zeros(rows, bool)
    for i, L in enumerate(lens):
        qkv[row0[i]: row0[i] + L], dO[row0[i]: row0[i] + L], inseq[row0[i]: row0[i] + L] = cd["qkv"][i], cd["dO"][i], True
    n_mat = sum(L * ldS for _, _, L, ldS, _ in groups)
    lib, ptr = dev.lib, dev.ptr
    ws_bytes = int(lib.mtts_attn_packed_ws_bytes(n_seq, heads))
    ws = dev.empty((ws_bytes + 3) // 4)
    c_lens, c_row0 = (C.c_int * n_seq)(*lens), (C.c_int * n_seq)(*row0)
    d_qkv, d_dO = dev.put(qkv), dev.put(dO)
    out = {}
    for path in (0, 1):
        P, O = dev.empty(n_mat, fill=np.nan), dev.empty((rows, d), fill=7.0)
        assert lib.mtts_attn_packed_fwd(n_seq, heads, dk, c_lens, c_row0, path, ptr(d_qkv), ptr(P), ptr(O), ptr(ws), ws_bytes, None) == 0
        dS, gq = dev.empty(n_mat, fill=np.nan), dev.empty((rows, 3 * d), fill=7.0)
        assert lib.mtts_attn_packed_bwd(n_seq, heads, dk, c_lens, c_row0, ptr(d_qkv), ptr(P), ptr(d_dO), ptr(dS), ptr(gq), ptr(ws), ws_bytes, None) == 0
        out[path] = tuple(np.array(dev.get(x)) for x in (P, O, dS, gq))

    qkv_of = lambda i, blk, hh: cd["qkv"][i][:, blk * d + hh * dk: blk * d + (hh + 1) * dk]
    dO_of = lambda i, hh: cd["dO"][i][:, hh * dk: (hh + 1) * dk]
    mat = lambda flat, L, ldS, so: flat[so: so + L * ldS].reshape(L, ldS)
    fwd_gate = {t: (max(4 * cd["e32"][t], 8 * EPS32 * cd["mx"][t]) if cd["big"] else FWD_ATOL[t]) for t in ("P", "O")}
    failures = []
    for path in (0, 1):
        P, O, dS, gq = out[path]
        # canaries: nothing outside the sequences is written, nothing non-finite comes out of them
        assert np.all(O[~inseq] == 7.0) and np.all(gq[~inseq] == 7.0), "a row outside every sequence was written"
        assert np.isfinite(O[inseq]).all() and np.isfinite(gq[inseq]).all(), "a product consumed guard rows, pad columns or stale memory"
        P_dev = []
        err = dict.fromkeys(("P", "O", "dS", "dQ", "dK", "dV"), 0.0)
        for n, (i, hh, L, ldS, so) in enumerate(groups):
            p = mat(P, L, ldS, so)
            assert np.isfinite(p[:, :L]).all(), (n, "P")
            assert np.all(p[:, L:] == 0), (n, "pad columns of P are not zero")
            P_dev.append(p[:, :L])
            err["P"] = max(err["P"], float(np.abs(p[:, :L] - cd["P64"][n]).max()))
            err["O"] = max(err["O"], float(np.abs(O[row0[i]: row0[i] + L, hh * dk: (hh + 1) * dk] - cd["O64"][n]).max()))
        refs, e32, mx = backward_refs(cd, qkv_of, P_dev, dO_of)
        for n, (i, hh, L, ldS, so) in enumerate(groups):
            s = mat(dS, L, ldS, so)
            assert np.isfinite(s[:, :L]).all(), (n, "dS")
            assert np.all(s[:, L:] == 0), (n, "pad columns of dS are not zero")
            r = slice(row0[i], row0[i] + L)
            got = (s[:, :L],) + tuple(gq[r, blk * d + hh * dk: blk * d + (hh + 1) * dk] for blk in range(3))   # dQ | dK | dV: each block its own gradient
            for t, a, b in zip(("dS", "dQ", "dK", "dV"), got, refs[n]):
                err[t] = max(err[t], float(np.abs(a - b).max()))
        gate = dict(fwd_gate, **{t: max(4 * e32[t], 8 * EPS32 * mx[t]) for t in e32})
        y32 = dict(cd["e32"], **e32)
        for t in err:
            print(f"RATIO {'gpu' if gpu else 'emu'} {name} {kind} path{path} {t} err={err[t]:.3e} err32={y32[t]:.3e} ratio={err[t] / max(y32[t], 1e-300):.2f} gate={gate[t]:.3e}")
            if not err[t] <= gate[t]:
                failures.append((path, t, err[t], gate[t]))
    # the two forward routes agree within the same gates (not bit for bit: the fused kernel sums in another order)
    for t, k in (("P", 0), ("O", 1)):
        a, b = out[0][k], out[1][k]
        if t == "P":
            diff = max(float(np.abs(mat(a, L, ldS, so)[:, :L] - mat(b, L, ldS, so)[:, :L]).max()) for _, _, L, ldS, so in groups)
        else:
            diff = float(np.abs(a[inseq] - b[inseq]).max())
        print(f"PATHS {'gpu' if gpu else 'emu'} {name} {kind} {t} diff={diff:.3e} gate={fwd_gate[t]:.3e}")
        if not diff <= fwd_gate[t]:
            failures.append(("0 vs 1", t, diff, fwd_gate[t]))
    assert not failures, failures


@pytest.mark.parametrize("gpu", [pytest.param(False, id="emu"), pytest.param(True, id="gpu", marks=pytest.mark.gpu)])
def test_packed_attention_rejects_bad_arguments(gpu):
    if gpu:
        ge.build_device()
    dev = Dev(gpu)
    lib, ptr = dev.lib, dev.ptr
    heads, dk, lens, row0 = 2, 16, (5, 3), (4, 13)
    d, rows = heads * dk, 20
    ws_bytes = int(lib.mtts_attn_packed_ws_bytes(2, heads))
    assert ws_bytes > 0 and lib.mtts_attn_packed_ws_bytes(8, 2) > ws_bytes
    ws, qkv, O, P = dev.empty((ws_bytes + 3) // 4), dev.empty((rows, 3 * d)), dev.empty((rows, d)), dev.empty(5 * 8 * 2 + 3 * 4 * 2)
    ci = lambda v: (C.c_int * len(v))(*v)
    fwd = lambda n_seq=2, dk=dk, lens=lens, qkv=qkv, wsb=ws_bytes, path=0: lib.mtts_attn_packed_fwd(
        n_seq, heads, dk, ci(lens), ci(row0), path, ptr(qkv), ptr(P), ptr(O), ptr(ws), wsb, None)
    bwd = lambda n_seq=2, dk=dk, lens=lens, dO=O, wsb=ws_bytes: lib.mtts_attn_packed_bwd(
        n_seq, heads, dk, ci(lens), ci(row0), ptr(qkv), ptr(P), ptr(dO), ptr(P), ptr(qkv), ptr(ws), wsb, None)
    assert fwd() == 0
    for call in (fwd, bwd):
        assert call(n_seq=0) == -1
        assert call(dk=18) == -1
        assert call(lens=(5, 0)) == -1
        assert call(wsb=ws_bytes - 1) == -1
    assert fwd(qkv=None) == -1 and bwd(dO=None) == -1
    assert fwd(path=2) == -1
    assert lib.mtts_attn_packed_fwd(2, heads, dk, None, ci(row0), 0, ptr(qkv), ptr(P), ptr(O), ptr(ws), ws_bytes, None) == -1
