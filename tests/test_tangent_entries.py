"""Kernel-level C-ABI entries of the second-order (tangent) row kernels — csrc/tangent.h: ln_jvp_fwd / ln_jvp_bwd, softmax_jvp_bwd,
bn_jvp_apply / bn_jvp_bwd, rowdot_jvp / rowdot_jvp_bwd, and ColArgs modes 5 / 6 of csrc/rowops.h — against the float64 autograd reference of
tangent_oracle.py on the same seeded float32 inputs.  As in test_kernel_entries.py every test runs twice: through the SIMT emulator on the
CPU and, marked gpu, through libmtts.so on the MI355X.

Tolerances are not chosen: for every output the bound is 8 x the distance between the float64 reference and the same reference evaluated
in float32 on the same inputs (the restatement's own rounding; 8 covers another summation tree), relative to max(1, max|ref|), and never
looser than the 2e-5 the primal kernel-entry tests use for backward outputs."""
import functools

import numpy as np
import pytest
import torch

import tangent_oracle as TO
from test_kernel_entries import Dev, dev  # noqa: F401  (the emu / gpu fixture)

F32 = np.float32


def _close(dev, name, got, ref, ref32):
    """|got - ref| against the bound derived from the float32 restatement (module docstring); prints the figures before it asserts."""
    got = np.asarray(got, np.float64).reshape(ref.shape)
    scale = max(1.0, float(np.abs(ref).max()))
    dist = float(np.abs(ref - ref32).max()) / scale
    bound = min(8.0 * dist, 2e-5)
    err = float(np.abs(got - ref).max()) / scale
    print(f"TANGENT_DIST {'gpu' if dev.gpu else 'emu'} {name} err {err:.3e} f32_restatement {dist:.3e} bound {bound:.3e} max|ref| {np.abs(ref).max():.3e}")
    assert err <= bound, f"{name}: {err:.3e} > {bound:.3e} (relative to max(1, max|ref|) = {scale:.3e})"


def _randn(g, *shape):
    return g.standard_normal(shape).astype(F32)


# ---- LayerNorm chain: layernorm_fwd -> layernorm_jvp_full -> layernorm_jvp_bwd ---------------------------------------------------------
# (5, 48) one partial workgroup; (37, 256) NV = 1 full; (19, 260) NV = 4 with a ragged last float4 group; (11, 1024) NV = 4 full;
# (419, 32) 53 chunks of 8 rows: colfinal_fold's lanes 0-4 take the four-deep loop, lanes 5-15 only the tail loop.
LN_CASES = [  # rows, C, mask, tgamma (and tbeta), relu_on_z, two_launch
    (5, 48, 1, 1, 0, 0), (5, 48, 0, 0, 1, 1),
    (37, 256, 1, 0, 1, 0), (37, 256, 0, 1, 0, 1),
    (19, 260, 1, 1, 1, 0), (19, 260, 0, 0, 0, 1),
    (11, 1024, 0, 1, 1, 1), (11, 1024, 1, 0, 0, 0),
    (419, 32, 1, 1, 0, 0), (419, 32, 1, 1, 1, 1), (419, 32, 0, 0, 0, 1),
    (1, 48, 1, 1, 0, 0), (1, 48, 0, 0, 1, 1), (1, 48, 0, 1, 0, 0),   # one row: masked, live on the two-launch route, live on the kernel's own partials
    (9, 32, 1, 1, 1, 0), (9, 32, 0, 0, 0, 1),          # one row past an 8-row workgroup: a partial last chunk of the fold
]


@functools.lru_cache(maxsize=None)
def _ln_case(rows, Cc, with_mask, with_tg, relu):
    g = np.random.RandomState(1000 * rows + Cc + 7 * with_mask + 3 * with_tg + relu)
    off = np.where(g.rand(rows) < 0.5, -0.5, 0.5).astype(F32)          # row means of about +-0.5: about half of z is negative
    i = dict(a=_randn(g, rows, Cc) + off[:, None], ta=_randn(g, rows, Cc), tres=_randn(g, rows, Cc),
             gamma=(1 + 0.1 * g.standard_normal(Cc)).astype(F32), beta=(0.1 * g.standard_normal(Cc)).astype(F32),
             tgamma=_randn(g, Cc), tbeta=_randn(g, Cc), mask=(g.rand(rows) > 0.3).astype(np.uint8), dy=_randn(g, rows, Cc), tgy=_randn(g, rows, Cc))
    i["mask"][min(1, rows - 1)] = 0   # one masked row for sure (rows = 1: the only row, when the case uses the mask)
    i["tz"] = i["ta"] + i["tres"]   # float32 sum: what the kernel stores (asserted bit-exact) and differentiates along
    args = (i["a"], i["tz"], i["gamma"], i["beta"], i["tgamma"] if with_tg else None, i["tbeta"] if with_tg else None,
            i["mask"] if with_mask else None, i["dy"], i["tgy"], relu)
    return i, TO.layernorm(*args), TO.layernorm(*args, dtype=torch.float32)


@pytest.mark.parametrize("rows,Cc,with_mask,with_tg,relu,two_launch", LN_CASES)
def test_layernorm_tangent_chain(dev, rows, Cc, with_mask, with_tg, relu, two_launch):
    i, ref, r32 = _ln_case(rows, Cc, with_mask, with_tg, relu)
    d = {k: dev.put(v) for k, v in i.items()}
    P = dev.ptr
    opt = lambda k, on: P(d[k]) if on else None
    z, y, st = dev.empty((rows, Cc)), dev.empty((rows, Cc)), dev.empty((rows, 2))
    ty, tz, tst = dev.empty((rows, Cc), fill=5), dev.empty((rows, Cc), fill=5), dev.empty((rows, 2), fill=5)
    dz, tgz, hg, hb = dev.empty((rows, Cc), fill=5), dev.empty((rows, Cc), fill=5), dev.empty(Cc, fill=5), dev.empty(Cc, fill=5)
    dz0, dg0, db0 = dev.empty((rows, Cc)), dev.empty(Cc), dev.empty(Cc)
    ws = dev.ws(rows)
    lib = dev.lib
    # z / stats / tz / tstats go from kernel to kernel on the device, as in the engine
    assert lib.mtts_layernorm_fwd(rows, Cc, P(d["a"]), None, P(d["gamma"]), P(d["beta"]), opt("mask", with_mask), P(z), P(y), P(st), P(ws), None) == 0
    assert lib.mtts_layernorm_jvp_full(rows, Cc, P(d["ta"]), P(d["tres"]), P(z), P(st), P(d["gamma"]), opt("tgamma", with_tg), opt("tbeta", with_tg),
                                       opt("mask", with_mask), P(ty), P(tz), P(tst), P(ws), None) == 0
    assert lib.mtts_layernorm_jvp_bwd(rows, Cc, P(d["dy"]), P(d["tgy"]), P(z), P(st), P(tz), P(tst), P(d["gamma"]), opt("tgamma", with_tg),
                                      opt("mask", with_mask), relu, two_launch, P(dz), P(tgz), P(hg), P(hb), P(ws), None) == 0
    assert np.array_equal(dev.get(tz), i["tz"])                      # tz_out = ta + tres, one float32 add: exact
    tag = f"ln[{rows}x{Cc},two_launch={two_launch}]"
    _close(dev, tag + ".tstats", dev.get(tst), ref["tstats"], r32["tstats"])
    _close(dev, tag + ".ty", dev.get(ty), ref["ty"], r32["ty"])
    got_dz, got_tgz = dev.get(dz).copy(), dev.get(tgz).copy()
    _close(dev, tag + ".dz", got_dz, ref["dz"], r32["dz"])
    _close(dev, tag + ".tgz", got_tgz, ref["tgz"], r32["tgz"])
    _close(dev, tag + ".hgamma", dev.get(hg), ref["hgamma"], r32["hgamma"])
    _close(dev, tag + ".hbeta", dev.get(hb), ref["hbeta"], r32["hbeta"])
    if with_mask:
        off = i["mask"] == 0
        assert off.any() and np.all(got_dz[off] == 0) and np.all(got_tgz[off] == 0)
    if not relu:
        # the primal half against the primal kernel on the same inputs.  Not the same bits: layernorm_bwd_kernel sums a lane's float4 as
        # (x + y) + (z + w) and divides by C, ln_jvp_bwd_kernel adds the four in order and multiplies by 1 / C — two summation orders of one
        # formula, so the two stay within the bound each has against the reference (one bound, not the two added).
        assert lib.mtts_layernorm_bwd(rows, Cc, P(d["dy"]), P(z), P(st), P(d["gamma"]), opt("mask", with_mask), P(dz0), P(dg0), P(db0), P(ws), None) == 0
        _close(dev, tag + ".dz(layernorm_bwd)", dev.get(dz0), ref["dz"], r32["dz"])
        scale = max(1.0, float(np.abs(ref["dz"]).max()))
        bound = min(8.0 * float(np.abs(ref["dz"] - r32["dz"]).max()) / scale, 2e-5)
        assert float(np.abs(dev.get(dz0).astype(np.float64) - got_dz).max()) / scale <= bound


# ---- softmax -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _softmax_case(n_mat, L):
    g = np.random.RandomState(31 * L + n_mat)
    i = dict(S=_randn(g, n_mat, L, L), tS=_randn(g, n_mat, L, L), dP=_randn(g, n_mat, L, L), tgP=_randn(g, n_mat, L, L))
    return i, TO.softmax(i["S"], i["tS"], i["dP"], i["tgP"], 0.25), TO.softmax(i["S"], i["tS"], i["dP"], i["tgP"], 0.25, dtype=torch.float32)


@pytest.mark.parametrize("n_mat,L", [(3, 5), (2, 64), (2, 65), (1, 130), (1, 333)])
def test_softmax_tangent_backward(dev, n_mat, L):
    i, ref, r32 = _softmax_case(n_mat, L)
    ldS = (L + 3) & ~3

    def padded(v, fill):
        o = np.full((n_mat, L, ldS), fill, F32)
        o[:, :, :L] = v
        return o
    Pm, tPm = dev.put(padded(ref["P"], 0)), dev.put(padded(ref["tP"], 0))   # the float64 f and its jvp, rounded to float32
    dP, tgP = dev.put(padded(i["dP"], 7)), dev.put(padded(i["tgP"], 7))
    ws = dev.ws(1, n_mat)
    P = dev.ptr
    assert dev.lib.mtts_softmax_jvp_bwd(n_mat, L, P(Pm), P(tPm), P(dP), P(tgP), 0.25, P(ws), None) == 0
    gd, gt = dev.get(dP), dev.get(tgP)
    _close(dev, f"softmax[{n_mat}x{L}].dS", gd[:, :, :L], ref["dS"], r32["dS"])
    _close(dev, f"softmax[{n_mat}x{L}].tgS", gt[:, :, :L], ref["tgS"], r32["tgS"])
    assert np.all(gd[:, :, L:] == 0) and np.all(gt[:, :, L:] == 0)


# ---- BatchNorm chain: batchnorm_fwd -> batchnorm_bwd -> batchnorm_jvp -> batchnorm_jvp_bwd ---------------------------------------------
# rows = G + B * (T + G) with 4 guard rows between the sequences (test_kernel_entries.py).  (2, 800, 16): 1612 rows = 51 chunks of 32, the
# four-deep loop of colfinal_fold under modes 3 and 6 and the pair merge under mode 2.
def _rect(B, T, G=4):
    rows = G + B * (T + G)
    inrect = np.zeros(rows, np.uint8)
    for b in range(B):
        inrect[G + b * (T + G): G + b * (T + G) + T] = 1
    return rows, inrect


@functools.lru_cache(maxsize=None)
def _bn_case(B, T, Cc, do_tanh, with_tg):
    rows, inrect = _rect(B, T)
    g = np.random.RandomState(B * 100 + T + Cc + with_tg)
    # (the rows outside the rectangle hold values too: no kernel may read them)
    i = dict(x=_randn(g, rows, Cc) + 0.5, tx=_randn(g, rows, Cc), gamma=(1 + 0.1 * g.standard_normal(Cc)).astype(F32),
             beta=(0.1 * g.standard_normal(Cc)).astype(F32), tgamma=_randn(g, Cc), tbeta=_randn(g, Cc), dy=_randn(g, rows, Cc),
             tgy=_randn(g, rows, Cc), inrect=inrect)
    sel = inrect.astype(bool)
    args = (i["x"][sel], i["tx"][sel], i["gamma"], i["beta"], i["tgamma"] if with_tg else None, i["tbeta"] if with_tg else None,
            i["dy"][sel], i["tgy"][sel], do_tanh)
    return i, sel, TO.batchnorm(*args), TO.batchnorm(*args, dtype=torch.float32)


@pytest.mark.parametrize("with_tg", [1, 0])
@pytest.mark.parametrize("B,T,Cc,do_tanh", [(3, 21, 48, 1), (1, 9, 80, 0), (2, 40, 512, 1), (2, 800, 16, 1)])
def test_batchnorm_tangent_chain(dev, B, T, Cc, do_tanh, with_tg):
    i, sel, ref, r32 = _bn_case(B, T, Cc, do_tanh, with_tg)
    rows, n_in = len(sel), B * T
    d = {k: dev.put(v) for k, v in i.items()}
    P = dev.ptr
    opt = lambda k: P(d[k]) if with_tg else None
    st, y, dx0, dgm, dbt = dev.empty(3 * Cc), dev.empty((rows, Cc)), dev.empty((rows, Cc)), dev.empty(Cc), dev.empty(Cc)
    tsum, ta = dev.empty(2 * Cc, fill=5), dev.empty((rows, Cc), fill=5)
    dx, tdx, hg, hb = dev.empty((rows, Cc), fill=5), dev.empty((rows, Cc), fill=5), dev.empty(Cc, fill=5), dev.empty(Cc, fill=5)
    ws = dev.ws(rows)
    lib = dev.lib
    assert lib.mtts_batchnorm_fwd(rows, Cc, P(d["x"]), P(d["inrect"]), P(d["gamma"]), P(d["beta"]), do_tanh, P(st), P(y), P(ws), None) == 0
    assert lib.mtts_batchnorm_bwd(rows, n_in, Cc, P(d["dy"]), P(y), P(d["x"]), P(st), P(d["inrect"]), P(d["gamma"]), do_tanh, P(dx0), P(dgm), P(dbt),
                                  P(ws), None) == 0
    assert lib.mtts_batchnorm_jvp(rows, n_in, Cc, P(d["x"]), P(d["tx"]), P(st), P(d["gamma"]), opt("tgamma"), opt("tbeta"), P(y), P(d["inrect"]),
                                  do_tanh, P(tsum), P(ta), P(ws), None) == 0
    assert lib.mtts_batchnorm_jvp_bwd(rows, n_in, Cc, P(d["dy"]), P(d["tgy"]), P(y), P(ta), P(d["x"]), P(d["tx"]), P(st), P(tsum), P(d["gamma"]),
                                      opt("tgamma"), P(dgm), P(dbt), P(d["inrect"]), do_tanh, P(dx), P(tdx), P(hg), P(hb), P(ws), None) == 0
    tag = f"bn[{B}x{T}x{Cc},tanh={do_tanh}]"
    _close(dev, tag + ".tsum", dev.get(tsum), ref["tsum"], r32["tsum"])
    for name, buf in (("ta", ta), ("dx", dx), ("tdx", tdx)):
        got = dev.get(buf)
        _close(dev, f"{tag}.{name}", got[sel], ref[name], r32[name])
        assert np.all(got[~sel] == 0), name
    _close(dev, tag + ".hgamma", dev.get(hg), ref["hgamma"], r32["hgamma"])
    _close(dev, tag + ".hbeta", dev.get(hb), ref["hbeta"], r32["hbeta"])


# ---- 256 -> 1 projection ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_t", [1, 0])
@pytest.mark.parametrize("rows,Cc", [(6, 32), (41, 256)])
def test_rowdot_tangent(dev, rows, Cc, with_t):
    g = np.random.RandomState(rows + Cc + with_t)
    valid = (g.rand(rows) > 0.3).astype(np.uint8)
    valid[1] = 0
    x, tx, w, tw, tb = _randn(g, rows, Cc) + 0.5, _randn(g, rows, Cc), _randn(g, Cc), _randn(g, Cc), _randn(g, 1)
    # the gradient of a prediction is zero on its invalid rows (the loss masks them), which is why the backward kernel takes no mask
    dout, tgout = _randn(g, rows) * valid, _randn(g, rows) * valid
    args = (x, tx, w, tw if with_t else None, tb if with_t else None, valid, dout, tgout)
    ref, r32 = TO.rowdot(*args), TO.rowdot(*args, dtype=torch.float32)
    P = dev.ptr
    dw, dtw = dev.put(w), dev.put(tw)
    tout, dx, tdx = dev.empty(rows, fill=5), dev.empty((rows, Cc), fill=5), dev.empty((rows, Cc), fill=5)
    ws = dev.ws(rows)
    assert dev.lib.mtts_rowdot_jvp(rows, Cc, P(dev.put(x)), P(dev.put(tx)), P(dw), P(dtw) if with_t else None, P(dev.put(tb)) if with_t else None,
                                   P(dev.put(valid)), P(tout), P(ws), None) == 0
    assert dev.lib.mtts_rowdot_jvp_bwd(rows, Cc, P(dev.put(dout)), P(dev.put(tgout)), P(dw), P(dtw) if with_t else None, P(dx), P(tdx), P(ws), None) == 0
    tag = f"rowdot[{rows}x{Cc}]"
    got = dev.get(tout)
    _close(dev, tag + ".tout", got, ref["tout"], r32["tout"])
    assert np.all(got[valid == 0] == 0)
    _close(dev, tag + ".dx", dev.get(dx), ref["dx"], r32["dx"])
    _close(dev, tag + ".tdx", dev.get(tdx), ref["tdx"], r32["tdx"])


# ---- bad arguments -----------------------------------------------------------------------------------------------------------------------
# name -> (argument template, positions of the optional pointers); "p" a valid device pointer, ints / floats as they are
ENTRIES = {
    "mtts_layernorm_jvp_full": ([8, 32] + ["p"] * 13, {3, 7, 8, 9, 11, 12, 14}),
    "mtts_layernorm_jvp_bwd": ([8, 32] + ["p"] * 9 + [0, 0] + ["p"] * 6, {9, 10, 18}),
    "mtts_softmax_jvp_bwd": ([1, 8, "p", "p", "p", "p", 0.25, "p", "p"], {8}),
    "mtts_batchnorm_jvp": ([8, 8, 32] + ["p"] * 8 + [1] + ["p"] * 4, {7, 8, 15}),
    "mtts_batchnorm_jvp_bwd": ([8, 8, 32] + ["p"] * 13 + [1] + ["p"] * 6, {12, 22}),
    "mtts_rowdot_jvp": ([8, 32] + ["p"] * 9, {5, 6, 10}),
    "mtts_rowdot_jvp_bwd": ([8, 32] + ["p"] * 8, {5, 9}),
}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_bad_arguments_are_rejected(dev, name):
    template, optional = ENTRIES[name]
    fn = getattr(dev.lib, name)
    ws = dev.ws(8, 1)
    bufs = []

    def arg(k, v):
        if v != "p":
            return v
        if k == len(template) - 1:
            return None                                    # the stream
        if k == len(template) - 2:
            return dev.ptr(ws)
        bufs.append(dev.empty(8 * 32, fill=1))             # 1.0f as float, non-zero as a mask byte
        return dev.ptr(bufs[-1])
    good = [arg(k, v) for k, v in enumerate(template)]
    assert fn(*good) == 0
    dev.get(bufs[0])                                       # (drain the queue before the next call's descriptor upload)
    for k, v in enumerate(template):
        if v == "p" and k not in optional:
            assert fn(*[None if j == k else a for j, a in enumerate(good)]) != 0, f"argument {k} null"
    if name == "mtts_softmax_jvp_bwd":                     # no channel count: the matrix count and length instead
        assert fn(0, *good[1:]) != 0 and fn(good[0], 0, *good[2:]) != 0
    else:
        c_at = 1 if template[2] == "p" else 2
        for bad_c in (30, 0, 1028):
            assert fn(*[bad_c if j == c_at else a for j, a in enumerate(good)]) != 0, f"C = {bad_c}"
        assert fn(0, *good[1:]) != 0
