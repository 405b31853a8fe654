"""The embedding and variance-adaptor row kernels of csrc/rowops.h, one at a time through their multi-task C entries (include/mtts.h:
mtts_rows_*), against numpy / torch restatements of the reference formulas written out here: transformer/Models.py:89-91 (embedding +
positions), speaker_encoder.py:62-65 and base_adaptor.py:64-70 (speaker vectors), fastspeech2.py:65-68 (speaker add), modules.py:83,94
(bucketize + embedding), modules.py:244-248 (the 256 -> 1 projection), modules.py:132-136 (duration rounding), modules.py:128-137,167-190
(length regulator on the frame rectangle).

Every case runs with 1 task and with 3 ragged tasks whose task stride is larger than rows * C: inputs behind a task's rows are NaN, outputs
behind them hold a sentinel that must survive.  Gathers, copies and single adds / multiplies are compared bit for bit with the same fp32
expression; reductions of n terms against float64 within n * 2^-24 * sum|terms| + one fp32 ulp (rowtask_util.sum_bound).  The same checks run
on the SIMT emulator and, marked gpu, on the device."""
import ctypes as C

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from oracle_util import Dev
from rowtask_util import ISENT, ROWSETS, SENT, assert_within, i32, i64, pack, stride_of, sum_bound, unpack

F32 = np.float32
CS = [32, 80, 256, 260]   # 80: no multiple of 64 (segsum's column blocks); 260: a second trip of the c += 256 loop


@pytest.fixture(params=[pytest.param(False, id="emu"), pytest.param(True, id="gpu", marks=pytest.mark.gpu)])
def dev(request):
    if request.param:
        ge.build_device()
    return Dev(request.param)


class Lay:
    """per-task arrays of one launch: row arrays get capacity max(rows) + 2 rows and a gap behind it"""

    def __init__(self, dev, rows):
        self.dev, self.rows, self.T, self.cap = dev, tuple(rows), len(rows), max(rows) + 2

    def rowf(self, parts, width, fill=np.nan):      # float [rows[t]][width] inputs (NaN behind the rows) or outputs (fill = SENT)
        st = stride_of(self.cap * width)
        return self.dev.put(pack(parts, st, fill, F32)), st

    def rowi(self, parts, dtype, fill, st):         # per-row ints / bytes at the shared "row" stride
        return self.dev.put(pack(parts, st, fill, dtype))

    def flat(self, parts, fill=np.nan, dtype=F32, gap=8):   # per-task arrays that are no row arrays (tables, parameters)
        st = stride_of(max(np.asarray(p).size for p in parts), gap)
        return self.dev.put(pack(parts, st, fill, dtype)), st

    def out(self, width):
        return self.rowf([np.zeros(0)] * self.T, width, SENT)

    def got(self, buf, st, width):
        parts, rest = unpack(self.dev.get(buf), st, [(r, width) if width else (r,) for r in self.rows])
        return parts, rest


def launch(dev, fn, lay, *args):
    ws = dev.ws(max(lay.rows))
    lay.ws = ws
    return fn(lay.T, i32(lay.rows), *args, dev.ptr(ws), None)


@pytest.mark.parametrize("Cc", CS)
@pytest.mark.parametrize("tasks", [1, 3])
def test_embed_pos(dev, tasks, Cc):
    """invalid rows are 0; a valid row with token 0 reads table row 0 (the engine keeps the padding row zero, the kernel does not special-case it)"""
    g = np.random.RandomState(10 * Cc + tasks)
    L, P, V, NP = Lay(dev, ROWSETS[tasks]), dev.ptr, 11, 13
    emb = [g.standard_normal((V, Cc)).astype(F32) for _ in L.rows]
    pos = g.standard_normal((NP, Cc)).astype(F32)
    tok = [g.randint(0, V, r) for r in L.rows]
    row_t = [g.randint(0, NP, r) for r in L.rows]
    valid = [(g.rand(r) > 0.3).astype(np.uint8) for r in L.rows]
    for t in range(tasks):
        valid[t][0], tok[t][0] = 1, 0
    if L.rows[0] > 2:
        valid[0][2] = 0
    d_emb, e_ts = L.flat(emb)
    r_ts = stride_of(L.cap, 4)
    out, o_ts = L.out(Cc)
    assert launch(dev, dev.lib.mtts_rows_embed_pos, L, Cc, P(d_emb), P(dev.put(pos)), P(L.rowi(tok, np.int32, 0, r_ts)), P(L.rowi(row_t, np.int32, 0, r_ts)),
                  P(L.rowi(valid, np.uint8, 1, r_ts)), P(out), i64([e_ts, r_ts, o_ts])) == 0
    got, rest = L.got(out, o_ts, Cc)
    assert np.all(rest == SENT)
    for t in range(tasks):
        ref = (emb[t][tok[t]] + pos[row_t[t]]) * valid[t][:, None].astype(F32)
        np.testing.assert_array_equal(got[t], ref)
        assert np.all(got[t][valid[t] == 0] == 0)


@pytest.mark.parametrize("Cc", CS)
@pytest.mark.parametrize("average", [0, 1])
@pytest.mark.parametrize("tasks", [1, 3])
def test_speaker_vec_and_table_grad(dev, tasks, average, Cc):
    """table mode with a speaker repeated inside the batch; averaged mode with a duplicated support id (hits = 2); unreferenced table rows: exactly 0"""
    g = np.random.RandomState(7 * Cc + 3 * tasks + average)
    Bs = {1: (4,), 3: (4, 1, 3)}[tasks]
    L, P, NS, NI = Lay(dev, Bs), dev.ptr, 7, 5
    table = [g.standard_normal((NS, Cc)).astype(F32) for _ in Bs]
    ids = []
    for t, B in enumerate(Bs):
        a = np.zeros(NI + 1, np.int64)
        if average:
            n = min(4, B + 1)                      # support ids: n of them, the first one twice when n > 1
            a[:n] = g.choice(np.arange(1, NS), n, replace=False)
            if n > 1:
                a[1] = a[0]
            a[NI] = n
        else:
            a[:B] = g.randint(0, NS, B)
            if B > 2:
                a[2] = a[0]
        ids.append(a)
    d_tab, t_ts = L.flat(table)
    d_ids, i_ts = L.flat(ids, 0, np.int32, gap=3)
    spk, s_ts = L.out(Cc)
    assert launch(dev, dev.lib.mtts_rows_speaker_vec, L, Cc, P(d_tab), P(d_ids), NI, average, P(spk), i64([t_ts, i_ts, s_ts])) == 0
    got, rest = L.got(spk, s_ts, Cc)
    assert np.all(rest == SENT)
    for t, B in enumerate(Bs):
        if average:
            rows = table[t][ids[t][:ids[t][NI]]].astype(np.float64)
            n = len(rows)
            ref = np.broadcast_to(rows.mean(0), (B, Cc))
            assert_within(got[t], ref, sum_bound(n, np.abs(rows).sum(0) / n, ref), "speaker_vec")
        else:
            np.testing.assert_array_equal(got[t], table[t][ids[t][:B]])
    # the transpose
    dspk = [g.standard_normal((B, Cc)).astype(F32) for B in Bs]
    d_dspk, d_ts = L.rowf(dspk, Cc)
    dt, dt_ts = L.flat([np.full((NS, Cc), SENT, F32)] * tasks, SENT)
    assert launch(dev, dev.lib.mtts_rows_speaker_table_grad, L, Cc, NS, P(d_dspk), P(d_ids), NI, average, P(dt), i64([d_ts, i_ts, dt_ts])) == 0
    gd, rest = unpack(dev.get(dt), dt_ts, [(NS, Cc)] * tasks)
    assert np.all(rest == SENT)
    for t, B in enumerate(Bs):
        d64 = dspk[t].astype(np.float64)
        ref, mag = np.zeros((NS, Cc)), np.zeros((NS, Cc))
        if average:
            n = int(ids[t][NI])
            for v in range(NS):
                hits = int((ids[t][:n] == v).sum())
                ref[v], mag[v] = d64.sum(0) * hits / n, np.abs(d64).sum(0) * hits / n
            assert hits_of(ids[t][:n]) == (2 if n > 1 else 1)
        else:
            for b in range(B):
                ref[ids[t][b]] += d64[b]
                mag[ids[t][b]] += np.abs(d64[b])
        assert_within(gd[t], ref, sum_bound(B, mag, ref), "speaker_table_grad")
        used = np.zeros(NS, bool)
        used[ids[t][:(ids[t][NI] if average else B)]] = True
        assert np.all(gd[t][~used] == 0) and (~used).any()


def hits_of(a):
    return int(np.bincount(a).max())


@pytest.mark.parametrize("Cc", CS)
@pytest.mark.parametrize("tasks", [1, 3])
def test_add_rowvec_fill_padded_gather_and_rect(dev, tasks, Cc):
    """at most one rounding per element: bit-for-bit equality with the fp32 numpy expression"""
    g = np.random.RandomState(5 * Cc + tasks)
    L, P, NB = Lay(dev, ROWSETS[tasks]), dev.ptr, 3
    r_ts = stride_of(L.cap, 4)
    x = [g.standard_normal((r, Cc)).astype(F32) for r in L.rows]
    inrect = [(g.rand(r) > 0.3).astype(np.uint8) for r in L.rows]
    for t in range(tasks):
        inrect[t][0] = 1
    inrect[0][3] = 0
    d_x, x_ts = L.rowf(x, Cc)
    d_in = L.rowi(inrect, np.uint8, 1, r_ts)
    # add_rowvec
    vec = [g.standard_normal((NB, Cc)).astype(F32) for _ in L.rows]
    row_b = [g.randint(0, NB, r) for r in L.rows]
    d_vec, v_ts = L.flat(vec)
    out, o_ts = L.out(Cc)
    assert launch(dev, dev.lib.mtts_rows_add_rowvec, L, Cc, P(d_x), P(d_vec), P(L.rowi(row_b, np.int32, 0, r_ts)), P(d_in), P(out), i64([x_ts, v_ts, r_ts, o_ts])) == 0
    got, rest = L.got(out, o_ts, Cc)
    assert np.all(rest == SENT)
    for t in range(tasks):
        np.testing.assert_array_equal(got[t], (x[t] + vec[t][row_b[t]]) * inrect[t][:, None].astype(F32))
    # fill_padded_rows, in place: valid rows keep their values, padded in-rect rows take the bias, the rest 0
    valid = [(m & (g.rand(len(m)) > 0.4)).astype(np.uint8) for m in inrect]
    valid[0][0] = 1
    bias = [g.standard_normal(Cc).astype(F32) for _ in L.rows]
    X, X_ts = L.rowf(x, Cc, SENT)
    d_b, b_ts = L.flat(bias)
    assert launch(dev, dev.lib.mtts_rows_fill_padded, L, Cc, P(X), P(d_b), P(d_in), P(L.rowi(valid, np.uint8, 0, r_ts)), i64([X_ts, b_ts, r_ts])) == 0
    got, rest = L.got(X, X_ts, Cc)
    assert np.all(rest == SENT)
    for t in range(tasks):
        ref = np.where(valid[t][:, None] != 0, x[t], np.where(inrect[t][:, None] != 0, bias[t][None, :], F32(0)))
        np.testing.assert_array_equal(got[t], ref)
    # gather_rows with -1 entries: the source space has its own (larger) row count
    NSRC = 14
    src = [g.standard_normal((NSRC, Cc)).astype(F32) for _ in L.rows]
    rowmap = [g.randint(-1, NSRC, r) for r in L.rows]
    rowmap[0][1], rowmap[0][4] = -1, NSRC - 1
    d_src, s_ts = L.flat(src)
    out, o_ts = L.out(Cc)
    assert launch(dev, dev.lib.mtts_rows_gather, L, Cc, P(d_src), P(L.rowi(rowmap, np.int32, 0, r_ts)), P(out), i64([s_ts, r_ts, o_ts])) == 0
    got, rest = L.got(out, o_ts, Cc)
    assert np.all(rest == SENT)
    for t in range(tasks):
        np.testing.assert_array_equal(got[t], np.where(rowmap[t][:, None] >= 0, src[t][np.maximum(rowmap[t], 0)], F32(0)))
    # length_regulate_rect: rectangle row -> packed frame (r2f, -1: padded) -> phoneme row (f_src, -1: none)
    NF = 10
    f_src = [g.randint(-1, NSRC, NF) for _ in L.rows]
    r2f = [g.randint(-1, NF, r) for r in L.rows]
    for t in range(tasks):
        f_src[t][0], f_src[t][1] = -1, 5
    r2f[0][:4] = [0, -1, 1, NF - 1]
    d_f, f_ts = L.flat(f_src, 0, np.int32, gap=2)
    out, o_ts = L.out(Cc)
    assert launch(dev, dev.lib.mtts_rows_length_regulate_rect, L, Cc, P(d_src), P(d_f), P(L.rowi(r2f, np.int32, 0, r_ts)), P(out),
                  i64([s_ts, f_ts, r_ts, o_ts])) == 0
    got, rest = L.got(out, o_ts, Cc)
    assert np.all(rest == SENT)
    for t in range(tasks):
        s = np.where(r2f[t] >= 0, f_src[t][np.maximum(r2f[t], 0)], -1)
        np.testing.assert_array_equal(got[t], np.where(s[:, None] >= 0, src[t][np.maximum(s, 0)], F32(0)))


@pytest.mark.parametrize("Cc", CS)
@pytest.mark.parametrize("control", [1.0, 1.3])
@pytest.mark.parametrize("tasks", [1, 3])
def test_bucket_embed_add(dev, tasks, control, Cc):
    """torch.bucketize(val * control, bins, right=False) with the product in fp32: values below the first boundary, above the last (index nb)
    and exactly ON boundaries (the boundaries are built as fp32 products u_k * control, so val = u_k lands on one for either control)"""
    g = np.random.RandomState(3 * Cc + tasks + int(control * 10))
    rows = {1: (41,), 3: (41, 1, 18)}[tasks]
    L, P, nb = Lay(dev, rows), dev.ptr, 15
    c32 = F32(control)
    u = np.sort(g.uniform(-2, 2, nb).astype(F32))
    bins = (u * c32).astype(F32)
    assert np.all(np.diff(bins) > 0)
    val = []
    for r in rows:
        v = (g.uniform(-2.5, 2.5, r).astype(F32))
        special = np.concatenate([u[[0, 3, 7, nb - 1]], [F32(-9.0), F32(9.0), np.nextafter(u[3], F32(9)), np.nextafter(u[3], F32(-9))]]).astype(F32)
        v[:min(r, len(special))] = special[:min(r, len(special))]
        val.append(v)
    x = [g.standard_normal((r, Cc)).astype(F32) for r in rows]
    table = [g.standard_normal((nb + 1, Cc)).astype(F32) for _ in rows]
    inrect = [(g.rand(r) > 0.2).astype(np.uint8) for r in rows]
    for t in range(tasks):
        inrect[t][0] = 1
    inrect[0][:8], inrect[0][9] = 1, 0
    r_ts = stride_of(L.cap, 4)
    d_x, x_ts = L.rowf(x, Cc)
    d_val, v_ts = L.rowf(val, 1)
    d_tab, t_ts = L.flat(table)
    idx_out = L.rowi([np.zeros(0)] * tasks, np.int32, ISENT, r_ts)
    out, o_ts = L.out(Cc)
    assert launch(dev, dev.lib.mtts_rows_bucket_embed_add, L, Cc, P(d_x), P(d_val), C.c_float(control), P(dev.put(bins)), nb, P(d_tab), P(L.rowi(inrect, np.uint8, 1, r_ts)),
                  P(idx_out), P(out), i64([x_ts, v_ts, t_ts, r_ts, o_ts])) == 0
    got, rest = L.got(out, o_ts, Cc)
    gi, irest = unpack(dev.get(idx_out), r_ts, [(r,) for r in rows])
    assert np.all(rest == SENT) and np.all(irest == ISENT)
    seen = set()
    for t in range(tasks):
        idx = torch.bucketize(torch.from_numpy(val[t] * c32), torch.from_numpy(bins), right=False).numpy()
        seen |= set(idx[inrect[t] != 0].tolist())
        np.testing.assert_array_equal(gi[t], np.where(inrect[t] != 0, idx, -1))
        np.testing.assert_array_equal(got[t], (x[t] + table[t][idx]) * inrect[t][:, None].astype(F32))
    assert {0, nb} <= seen
    on = torch.bucketize(torch.from_numpy(u[[0, 3, 7, nb - 1]] * c32), torch.from_numpy(bins), right=False).numpy()
    np.testing.assert_array_equal(on, [0, 3, 7, nb - 1])     # a value ON boundary k belongs to bucket k (right=False)
    np.testing.assert_array_equal(gi[0][:4], on)


@pytest.mark.parametrize("Cc", CS)
@pytest.mark.parametrize("tasks", [1, 3])
def test_rowdot_fwd_bwd(dev, tasks, Cc):
    g = np.random.RandomState(11 * Cc + tasks)
    L, P = Lay(dev, ROWSETS[tasks]), dev.ptr
    r_ts = stride_of(L.cap, 4)
    x = [g.standard_normal((r, Cc)).astype(F32) for r in L.rows]
    par = [g.standard_normal(Cc + 4).astype(F32) for _ in L.rows]     # w [C] and, behind it, the bias: one parameter block per task
    valid = [(g.rand(r) > 0.3).astype(np.uint8) for r in L.rows]
    for t in range(tasks):
        valid[t][0] = 1
    valid[0][2] = 0
    d_x, x_ts = L.rowf(x, Cc)
    d_par, p_ts = L.flat(par)
    d_b = d_par[Cc:]                                                   # b[t] = par[t][C]: the same stride as w
    out, o_ts = L.out(1)
    assert launch(dev, dev.lib.mtts_rows_rowdot, L, Cc, P(d_x), P(d_par), P(d_b), P(L.rowi(valid, np.uint8, 1, r_ts)), P(out), i64([x_ts, p_ts, r_ts, o_ts])) == 0
    got, rest = L.got(out, o_ts, 0)
    assert np.all(rest == SENT)
    for t in range(tasks):
        w, b = par[t][:Cc].astype(np.float64), float(par[t][Cc])
        terms = x[t].astype(np.float64) * w[None]
        ref = np.where(valid[t] != 0, terms.sum(1) + b, 0.0)
        assert_within(got[t], ref, sum_bound(Cc + 1, np.abs(terms).sum(1) + abs(b), ref), "rowdot")
        assert np.all(got[t][valid[t] == 0] == 0)
    # backward: one multiply per element
    dout = [g.standard_normal(r).astype(F32) * v for r, v in zip(L.rows, valid)]   # (0 on invalid rows, as the loss gradient leaves it)
    d_do, do_ts = L.rowf(dout, 1)
    dx, dx_ts = L.out(Cc)
    assert launch(dev, dev.lib.mtts_rows_rowdot_bwd, L, Cc, P(d_do), P(d_par), P(dx), i64([do_ts, p_ts, dx_ts])) == 0
    got, rest = L.got(dx, dx_ts, Cc)
    assert np.all(rest == SENT)
    for t in range(tasks):
        np.testing.assert_array_equal(got[t], dout[t][:, None] * par[t][None, :Cc])
        assert np.all(got[t][valid[t] == 0] == 0)


@pytest.mark.parametrize("Cc", CS)
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("tasks", [1, 3])
def test_segsum_rows(dev, tasks, accumulate, Cc):
    """segment lengths 0, 1, 4, 5, 8, 9, 23 around the kernel's 4-lane, two-sums-per-lane walk; segments start at row 3; rows of X that belong
    to no segment are NaN, so a row read past a segment's end shows"""
    g = np.random.RandomState(13 * Cc + tasks + accumulate)
    lens = {1: [(0, 1, 4, 5, 8, 9, 23)], 3: [(0, 1, 4, 5, 8, 9, 23), (5,), (9, 0, 23, 4)]}[tasks]
    Bs = tuple(len(l) for l in lens)
    L, P = Lay(dev, Bs), dev.ptr
    X, start = [], []
    for l in lens:
        s, a, pieces = [], 3, [np.full((3, Cc), np.nan, F32)]
        for n in l:
            s.append(a)
            pieces += [g.standard_normal((n, Cc)).astype(F32), np.full((1, Cc), np.nan, F32)]   # a NaN row between two segments
            a += n + 1
        X.append(np.concatenate(pieces))
        start.append(s)
    d_X, X_ts = L.flat(X)
    g_ts = stride_of(max(Bs), 4)
    prev = [g.standard_normal((B, Cc)).astype(F32) for B in Bs]
    out, o_ts = L.rowf(prev, Cc, SENT)
    assert launch(dev, dev.lib.mtts_rows_segsum, L, Cc, P(d_X), P(L.rowi(start, np.int32, 0, g_ts)), P(L.rowi(lens, np.int32, 0, g_ts)), P(out), accumulate,
                  i64([X_ts, g_ts, o_ts])) == 0
    got, rest = L.got(out, o_ts, Cc)
    assert np.all(rest == SENT)
    for t, l in enumerate(lens):
        for b, n in enumerate(l):
            seg = X[t][start[t][b]: start[t][b] + n].astype(np.float64)
            ref, mag = seg.sum(0), np.abs(seg).sum(0)
            if accumulate:
                ref, mag = ref + prev[t][b], mag + np.abs(prev[t][b])
            assert_within(got[t][b], ref, sum_bound(n + accumulate, mag, ref), f"segsum len {n}")
            if n == 0 and not accumulate:
                assert np.all(got[t][b] == 0)


@pytest.mark.parametrize("d_control", [1.0, 0.7])
@pytest.mark.parametrize("tasks", [1, 3])
def test_duration_round(dev, tasks, d_control):
    """logd = log1p(k + f), k in 0 .. 60, f in [0.05, 0.45] u [0.55, 0.95]: exp(logd) - 1 is at least 0.05 from a rounding tie, 4 orders of
    magnitude above the error of an fp32 exp at 61, so round() is decided and no case is excluded.  Negative logd clamps to 0."""
    g = np.random.RandomState(tasks + int(d_control * 10))
    rows = {1: (70,), 3: (1100, 1, 70)}[tasks]     # 1100 rows: a second trip of the 4 x 256 grid-stride loop
    L, P = Lay(dev, rows), dev.ptr
    logd, want = [], []
    for r in rows:
        k = np.arange(r) % 61
        f = np.where(g.rand(r) < 0.5, g.uniform(0.05, 0.45, r), g.uniform(0.55, 0.95, r))
        ld = np.log1p(k + f)
        neg = np.arange(r) % 9 == 4
        ld[neg] = -g.uniform(0.1, 3.0, int(neg.sum()))
        ld = ld.astype(F32)
        logd.append(ld)
        rounded = np.round(np.exp(ld.astype(np.float64)) - 1.0)
        assert np.all(np.abs(np.exp(ld.astype(np.float64)) - 1.0 - rounded)[~neg] < 0.46)
        want.append(np.maximum(rounded.astype(F32) * F32(d_control), F32(0)))
    d_l, l_ts = L.rowf(logd, 1)
    out = dev.put(np.full(tasks * l_ts, SENT, F32))
    assert launch(dev, dev.lib.mtts_rows_duration_round, L, P(d_l), C.c_float(d_control), P(out), i64([l_ts])) == 0
    got, rest = L.got(out, l_ts, 0)
    assert np.all(rest == SENT)
    for t in range(tasks):
        np.testing.assert_array_equal(got[t], want[t])
        assert np.all(got[t] >= 0)


def test_bad_arguments_are_rejected(dev):
    L = Lay(dev, (4,))
    lib, P = dev.lib, dev.ptr
    ws = dev.ws(8)
    buf = dev.empty(4096)
    ib = dev.put(np.zeros(64, np.int32))
    bb = dev.put(np.ones(64, np.uint8))
    p, q, m, w = P(buf), P(ib), P(bb), P(ws)
    ts = i64([1024] * 5)
    ok = i32([4])
    calls = {
        "embed_pos": lambda t, n, Cc, a=p, s=ts, k=w: lib.mtts_rows_embed_pos(t, n, Cc, a, p, q, q, m, p, s, k, None),
        "speaker_vec": lambda t, n, Cc, a=p, s=ts, k=w: lib.mtts_rows_speaker_vec(t, n, Cc, a, q, 5, 0, p, s, k, None),
        "speaker_table_grad": lambda t, n, Cc, a=p, s=ts, k=w: lib.mtts_rows_speaker_table_grad(t, n, Cc, 3, a, q, 5, 0, p, s, k, None),
        "add_rowvec": lambda t, n, Cc, a=p, s=ts, k=w: lib.mtts_rows_add_rowvec(t, n, Cc, a, p, q, m, p, s, k, None),
        "bucket_embed_add": lambda t, n, Cc, a=p, s=ts, k=w: lib.mtts_rows_bucket_embed_add(t, n, Cc, a, p, 1.0, p, 3, p, m, q, p, s, k, None),
        "rowdot": lambda t, n, Cc, a=p, s=ts, k=w: lib.mtts_rows_rowdot(t, n, Cc, a, p, p, m, p, s, k, None),
        "rowdot_bwd": lambda t, n, Cc, a=p, s=ts, k=w: lib.mtts_rows_rowdot_bwd(t, n, Cc, a, p, p, s, k, None),
        "segsum": lambda t, n, Cc, a=p, s=ts, k=w: lib.mtts_rows_segsum(t, n, Cc, a, q, q, p, 0, s, k, None),
        "fill_padded": lambda t, n, Cc, a=p, s=ts, k=w: lib.mtts_rows_fill_padded(t, n, Cc, a, p, m, m, s, k, None),
        "gather": lambda t, n, Cc, a=p, s=ts, k=w: lib.mtts_rows_gather(t, n, Cc, a, q, p, s, k, None),
        "length_regulate_rect": lambda t, n, Cc, a=p, s=ts, k=w: lib.mtts_rows_length_regulate_rect(t, n, Cc, a, q, q, p, s, k, None),
    }
    for name, f in calls.items():
        assert f(1, ok, 30) != 0, name                    # C % 4
        assert f(1, ok, 1028) != 0, name                  # C > 1024
        assert f(0, ok, 32) != 0 and f(9, i32([4] * 9), 32) != 0, name   # tasks outside 1 .. 8
        assert f(1, None, 32) != 0 and f(1, i32([0]), 32) != 0 and f(1, i32([-1]), 32) != 0, name   # no / empty / negative row counts
        assert f(1, ok, 32, a=None) != 0, name            # a null array
        assert f(1, ok, 32, s=None) != 0 and f(1, ok, 32, s=i64([-4] * 5)) != 0, name   # no / negative strides
        assert f(1, ok, 32, k=None) != 0, name            # no scratch
    dr = lambda t, n, a=p, s=ts, k=w: lib.mtts_rows_duration_round(t, n, a, 1.0, p, s, k, None)
    assert dr(0, ok) != 0 and dr(9, i32([4] * 9)) != 0 and dr(1, None) != 0 and dr(1, ok, a=None) != 0 and dr(1, ok, s=None) != 0 and dr(1, ok, k=None) != 0
    assert np.all(dev.get(buf) == 0)                      # a refusal launches nothing
