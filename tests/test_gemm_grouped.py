"""mtts_gemm_f32_grouped: the grouped GEMM launcher (csrc/gemm.h: gemm_launch / gemm_batch_end) as the engine drives it — TASK- and
TABLE-mode groups, the fused epilogue, the column-sum tile, dilated A-taps, split-K on a caller-provided workspace, the two placements
and the multi-problem launch — each feature alone against float64 built from the same seeded fp32 inputs.  Two arms (oracle_util.Dev):
the SIMT emulator build on the CPU and, marked gpu, libmtts.so on the MI355X.

Every output buffer starts as the sentinel 7.0; what the operation must not write is asserted bit-equal to it afterwards, forced zeros
are asserted exactly 0.0, computed values meet the bounds of test_gpu_kernels.py (2e-5 single-source, 3e-5 dual-source, times
max(1, max |want|)).  Rows the kernel must not read (beyond a group's own M or K) hold NaN.

Contract pinned by (b) and (e): a group whose K (or M) is <= 0 is SKIPPED — its C and colsum keep their old contents, bias or not (gemm.h:
GemmArgs::dimptr).  That equals epilogue(0) only for an accumulating launch without bias; the engine never launches such a group (every
task of a plan has >= 1 utterance), and the task-per-XCD schedule gives it no workgroup."""
import ctypes as C

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from oracle_util import Dev

SENT = np.float32(7.0)
RELU, ACCUM, LRELU = 1, 2, 4
NT, NN, TN = 0, 1, 2
pad4 = lambda x: (x + 3) & ~3


class Group(C.Structure):
    _fields_ = [("a_off", C.c_longlong), ("b_off", C.c_longlong), ("c_off", C.c_longlong), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
                ("lda", C.c_int), ("ldb", C.c_int), ("ldc", C.c_int)]


class Desc(C.Structure):
    """include/mtts.h: mtts_gemm_desc"""
    _fields_ = ([(n, C.c_void_p) for n in ("A", "B", "C", "A2", "B2")] + [(n, C.c_longlong) for n in ("a_gs", "b_gs", "c_gs", "a2_gs", "b2_gs")] +
                [(n, C.c_void_p) for n in ("dimptr", "host_dims", "table")] +
                [("bias", C.c_void_p), ("bias_gs", C.c_longlong), ("rowmask", C.c_void_p), ("rowmask_gs", C.c_longlong),
                 ("relu_ref", C.c_void_p), ("relu_ref_gs", C.c_longlong), ("c_rowmap", C.c_void_p), ("c_rowmap_gs", C.c_longlong),
                 ("colsum", C.c_void_p), ("colsum_gs", C.c_longlong), ("colsum_w", C.c_void_p), ("colsum_w_gs", C.c_longlong)] +
                [(n, C.c_int) for n in ("form", "groups", "max_M", "max_N", "M", "N", "K", "lda", "ldb", "ldc", "dim_stride", "dim_sel", "dim_mult",
                                        "ld_relu", "flags")] +
                [("alpha", C.c_float), ("act_slope", C.c_float)] + [(n, C.c_int) for n in ("taps", "tap_k", "tap_bstride", "a_tap_k", "a_tap_rows")])


@pytest.fixture(params=[pytest.param(False, id="emu"), pytest.param(True, id="gpu", marks=pytest.mark.gpu)])
def dev(request):
    if request.param:
        ge.build_device()
    return Dev(request.param)


@pytest.fixture(params=[pytest.param(True, id="gpu", marks=pytest.mark.gpu)])
def gdev(request):
    """the forced LDS-DMA family (family 4064) exists in the device build only"""
    ge.build_device()
    return Dev(True)


def addr(dev, x, off=0):
    """address of element `off` of a 4-byte-element buffer"""
    if x is None:
        return None
    return (x.data_ptr() if dev.gpu else x.ctypes.data) + 4 * int(off)


def desc(dev, form, A, B, Cm, M, N, K, lda, ldb, ldc, groups=1, max_M=None, max_N=None, **kw):
    d = Desc()
    d.form, d.groups, d.M, d.N, d.K, d.lda, d.ldb, d.ldc = form, groups, M, N, K, lda, ldb, ldc
    d.max_M, d.max_N = (M if max_M is None else max_M), (N if max_N is None else max_N)
    d.alpha, d.act_slope, d.dim_stride, d.dim_mult = 1.0, 0.2, 1, 1
    d.A, d.B, d.C = (a if isinstance(a, int) else addr(dev, a) for a in (A, B, Cm))
    for k, v in kw.items():
        assert hasattr(d, k), k
        if isinstance(v, (int, float)) or v is None:
            setattr(d, k, v)
        elif k == "host_dims":
            setattr(d, k, v.ctypes.data)
        else:
            setattr(d, k, addr(dev, v))
    return d


def launch(dev, descs, family=0, ws=None):
    """-> [(split factor, placement)] per problem"""
    arr = (Desc * len(descs))(*descs)
    rep = (C.c_int * (2 * len(descs)))(*([-1] * (2 * len(descs))))
    rc = dev.lib.mtts_gemm_f32_grouped(C.addressof(arr), len(descs), family, dev.ptr(ws[0]) if ws else None, dev.ptr(ws[1]) if ws else None, rep, None)
    assert rc == 0
    if dev.gpu:
        torch.cuda.synchronize()
    return [(rep[2 * i], rep[2 * i + 1]) for i in range(len(descs))]


def close(tag, dev, got, want, dual=False):
    assert np.all(np.isfinite(got)), tag
    bound = (3e-5 if dual else 2e-5) * max(1.0, float(np.abs(want).max()) if want.size else 0.0)
    err = float(np.abs(got.astype(np.float64) - want).max()) if want.size else 0.0
    print("error/bound %s %s %.4f" % ("gpu" if dev.gpu else "emu", tag, err / bound))   # (shown with -s, and with a failure)
    assert err < bound, (tag, err, bound)


def untouched(x):
    return bool(np.all(x.view(np.uint32) == SENT.view(np.uint32)))


# ---- TASK-mode operands: group z at z * stride, rows beyond the group's own M / K are NaN, K-contiguous pad columns are 0 -------------
class Task:
    """`groups` problems of one form, common N, per-group M (forms 0 / 1) or K (form 2).  C is [groups][maxM + 3][ldc] with ldc = pad4(N) + 4:
    three gap rows between groups and >= 4 columns beyond N that must stay the sentinel."""

    def __init__(self, dev, g, form, Ms, N, Ks, bias=True, n_src=1):
        self.dev, self.form, self.G, self.N = dev, form, len(Ms), N
        self.Ms, self.Ks = list(Ms), list(Ks)
        G, mM, mK = self.G, max(Ms), max(Ks)
        self.mM, self.mK = mM, mK
        self.src, self.prod = [], [[None] * G for _ in range(n_src)]
        for s in range(n_src):
            if form == TN:
                A = g.standard_normal((G, mK, pad4(mM))).astype(np.float32)
                B = g.standard_normal((G, mK, pad4(N))).astype(np.float32)
            else:
                A = np.zeros((G, mM, pad4(mK)), np.float32)
                A[:, :, :mK] = g.standard_normal((G, mM, mK))
                if form == NT:
                    B = np.zeros((G, N, pad4(mK)), np.float32)
                    B[:, :, :mK] = g.standard_normal((G, N, mK))
                else:
                    B = g.standard_normal((G, mK, pad4(N))).astype(np.float32)
            for z in range(G):
                M, K = Ms[z], Ks[z]
                a, b = A[z].astype(np.float64), B[z].astype(np.float64)
                if form == NT:
                    self.prod[s][z] = a[:M, :K] @ b[:N, :K].T
                    A[z, M:] = np.nan
                elif form == NN:
                    self.prod[s][z] = a[:M, :K] @ b[:K, :N]
                    A[z, M:] = np.nan
                else:
                    self.prod[s][z] = a[:K, :M].T @ b[:K, :N]
                    A[z, K:] = np.nan
                    B[z, K:] = np.nan
            self.src.append((A, B, dev.put(A), dev.put(B)))
        self.lda, self.ldb = self.src[0][0].shape[2], self.src[0][1].shape[2]
        self.a_gs, self.b_gs = self.src[0][0][0].size, self.src[0][1][0].size
        self.ldc, self.crows = pad4(N) + 4, mM + 3
        self.bias = g.standard_normal((G, N)).astype(np.float32) if bias else None
        self.dbias = dev.put(self.bias) if bias else None

    def out(self, fill=None):
        return self.dev.put(np.full((self.G, self.crows, self.ldc), SENT, np.float32) if fill is None else fill)

    def desc(self, Cm, **kw):
        dual = len(self.src) > 1
        if dual:
            kw.update(A2=self.src[1][2], B2=self.src[1][3], a2_gs=self.a_gs, b2_gs=self.b_gs)
        if self.dbias is not None:
            kw.update(bias=self.dbias, bias_gs=self.N)
        return desc(self.dev, self.form, self.src[0][2], self.src[0][3], Cm, self.mM, self.N, self.mK, self.lda, self.ldb, self.ldc, groups=self.G,
                    a_gs=self.a_gs, b_gs=self.b_gs, c_gs=self.crows * self.ldc, **kw)

    def want(self, z, alpha=1.0):
        w = alpha * sum(p[z] for p in self.prod)
        return w + self.bias[z].astype(np.float64)[None, :] if self.bias is not None else w

    def check(self, tag, got, alpha=1.0, skip_empty_k=True):
        """every group equals its own float64 product; everything else is the sentinel"""
        dual = len(self.src) > 1
        for z in range(self.G):
            M = self.Ms[z] if not (skip_empty_k and self.Ks[z] <= 0) else 0
            if M:
                close(tag, self.dev, got[z, :M, :self.N], self.want(z, alpha), dual)
            assert untouched(got[z, M:]) and untouched(got[z, :, self.N:]), (tag, z)


def dims_dev(dev, vals, stride=3, mult=1):
    """per-group sizes as a meta table of `stride` ints per group (the other slots hold garbage) -> (device array, host values)"""
    t = np.full(len(vals) * stride, 99999, np.int32)
    assert all(v % mult == 0 for v in vals)
    t[::stride] = np.asarray(vals) // mult
    return dev.put(t), np.ascontiguousarray(t[::stride])


M_RAGGED = {2: [0, 65], 3: [65, 0, 130], 8: [64, 0, 65, 130, 1, 63, 130, 65]}
K_RAGGED = {1: [77], 2: [17, 0], 8: [100, 0, 1, 16, 17, 100, 17, 1]}


# ---- (a) TASK-mode groups, ragged M -----------------------------------------------------------------------------------------------------
def check_ragged_m(dev, form, groups, mult, family=0):
    g = np.random.RandomState(100 * form + groups + mult)
    Ms = M_RAGGED[groups] if mult == 1 else [130, 0, 64]   # (dim_mult = 2 cannot express an odd M: no 65-row group in that one case)
    t = Task(dev, g, form, Ms, 80, [36] * len(Ms))
    dd, _ = dims_dev(dev, Ms, 3, mult)
    out = t.out()
    rep = launch(dev, [t.desc(out, dimptr=dd, dim_stride=3, dim_sel=0, dim_mult=mult, max_M=130)], family)
    assert rep == [(1, 0)] or rep == [(1, 2)]
    t.check("a ragged M" + (" lds-dma" if family else ""), dev.get(out))


@pytest.mark.parametrize("form,groups,mult", [(f, n, 1) for f in (NT, NN) for n in (2, 3, 8)] + [(NT, 3, 2)])
def test_task_groups_ragged_m(dev, form, groups, mult):
    check_ragged_m(dev, form, groups, mult)


# ---- (b) TASK-mode groups, ragged K -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accum", [False, True])
@pytest.mark.parametrize("groups", [2, 8])
def test_task_groups_ragged_k(dev, groups, accum):
    """A group with K = 0 is skipped (module docstring): its C keeps the old contents, with and without ACCUM."""
    g = np.random.RandomState(200 + groups + accum)
    Ks = K_RAGGED[groups]
    t = Task(dev, g, TN, [70] * groups, 40, Ks)
    dd, _ = dims_dev(dev, Ks)
    out = t.out()
    launch(dev, [t.desc(out, dimptr=dd, dim_stride=3, dim_sel=2, flags=ACCUM if accum else 0)])
    got = dev.get(out)
    for z in range(groups):
        if Ks[z] == 0:
            assert untouched(got[z])
        else:
            close("b ragged K", dev, got[z, :70, :40], t.want(z) + (7.0 if accum else 0.0))
            assert untouched(got[z, 70:]) and untouched(got[z, :, 40:])


# ---- (c) TABLE mode ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [NT, NN])
def test_table_mode(dev, form):
    g = np.random.RandomState(300 + form)
    shapes = [(5, 7, 20), (65, 130, 36), (128, 64, 100)]
    # group 0 inherits the launch's leading dimensions (zeros in its record), groups 1 and 2 carry their own; group 1's are wider than needed
    lds = [(20, 20 if form == NT else 8, 8), (40, 40 if form == NT else 136, 140), (100, 100 if form == NT else 64, 64)]
    offs, sizes = [], [0, 0, 0]
    for (M, N, K), (lda, ldb, ldc) in zip(shapes, lds):
        o = (sizes[0] + 8, sizes[1] + 12, sizes[2] + 16)   # gaps in front of every group
        offs.append(o)
        sizes = [o[0] + M * lda, o[1] + (N if form == NT else K) * ldb, o[2] + M * ldc]
    A, B = (np.full(sizes[i] + 8, np.nan, np.float32) for i in (0, 1))
    want, tab = [], (Group * 3)()
    for z, ((M, N, K), (lda, ldb, ldc), (ao, bo, co)) in enumerate(zip(shapes, lds, offs)):
        a = np.zeros((M, lda), np.float32)
        a[:, :K] = g.standard_normal((M, K))
        b = np.zeros((N, ldb) if form == NT else (K, ldb), np.float32)
        if form == NT:
            b[:, :K] = g.standard_normal((N, K))
        else:
            b[:, :N] = g.standard_normal((K, N))
        A[ao:ao + a.size], B[bo:bo + b.size] = a.ravel(), b.ravel()
        want.append(a[:, :K].astype(np.float64) @ (b[:, :K].astype(np.float64).T if form == NT else b[:, :N].astype(np.float64)))
        tab[z] = Group(ao, bo, co, M, N, K, *((0, 0, 0) if z == 0 else (lda, ldb, ldc)))
    bias = g.standard_normal(130).astype(np.float32)
    out = dev.empty(sizes[2] + 16, fill=SENT)
    dt = dev.put(np.frombuffer(bytes(tab), np.uint8).copy())
    d = desc(dev, form, dev.put(A), dev.put(B), out, 128, 130, 100, lds[0][0], lds[0][1], lds[0][2], groups=3, table=dt, alpha=0.5, bias=dev.put(bias))
    assert launch(dev, [d]) == [(1, 0)]
    got = dev.get(out).copy()
    for z, ((M, N, K), (lda, ldb, ldc), (ao, bo, co)) in enumerate(zip(shapes, lds, offs)):
        blk = got[co:co + M * ldc].reshape(M, ldc)
        close("c table", dev, blk[:, :N], 0.5 * want[z] + bias[:N].astype(np.float64)[None, :])
        blk[:, :N] = SENT
    assert untouched(got)   # the gaps between the groups, the columns beyond every N


# ---- (d) fused epilogue -----------------------------------------------------------------------------------------------------------------
def check_epilogue(dev, feature, family=0, K=36, ws=None, want_split=False):
    M, N, G = 130, 70, 2
    g = np.random.RandomState(400 + len(feature) + K)
    t = Task(dev, g, NT, [M] * G, N, [K] * G)
    tag = "d epilogue" + (" lds-dma" if family else "") + (" split-K" if ws else "")
    kw, flags = {}, 0
    everything = feature == "all"
    mask = np.ones((G, M), np.uint8)
    ld_relu = N + 10                             # relu_ref's own leading dimension: neither ldc nor N
    assert ld_relu != t.ldc and ld_relu != pad4(N)
    ref = np.ones((G, M, ld_relu), np.float32)
    rmap = np.tile(np.arange(M, dtype=np.int32), (G, 1))
    if feature == "rowmask" or everything:
        mask = (g.rand(G, M) > 0.3).astype(np.uint8)
        mask[:, [0, 63, 64, M - 1]] = 0
        kw.update(rowmask=dev.put(mask), rowmask_gs=M)
    if feature == "relu_ref" or everything:
        ref = g.standard_normal((G, M, ld_relu)).astype(np.float32)
        ref[g.rand(G, M, ld_relu) < 0.1] = 0.0   # exact zeros: the value is kept only where relu_ref > 0
        ref[:, :, N:] = np.nan                   # (the columns beyond N are never read: NaN > 0 is false, a kept value would turn 0)
        kw.update(relu_ref=dev.put(ref), relu_ref_gs=M * ld_relu, ld_relu=ld_relu)
    if feature == "rowmap" or everything:
        for z in range(G):
            rmap[z] = g.permutation(M)
            rmap[z, g.permutation(M)[:M // 4]] = -1
        kw.update(c_rowmap=dev.put(rmap), c_rowmap_gs=M)
    slope = None
    if feature.startswith("lrelu"):
        slope = float(feature[5:])
        flags = LRELU
        kw.update(act_slope=slope)
    old = np.full((G, t.crows, t.ldc), SENT, np.float32)
    if everything:
        flags = ACCUM | RELU
        old[:, :M, :N] = g.standard_normal((G, M, N))
    out = t.out(old.copy())
    rep = launch(dev, [t.desc(out, flags=flags, alpha=0.5, **kw)], family, ws)
    assert (rep[0][0] >= 2) == want_split, rep
    got = dev.get(out)
    for z in range(G):
        v = t.want(z, 0.5)
        exp = old[z].astype(np.float64)
        written = np.zeros(t.crows, bool)
        for m in range(M):
            mo = rmap[z, m]
            if mo < 0:
                continue
            assert not written[mo]
            written[mo] = True
            r = v[m] + (exp[mo, :N] if everything else 0.0)     # accumulate first (read at the remapped row),
            if everything:
                r = np.maximum(r, 0.0)                         # then the activation,
            if slope is not None:
                r = np.where(r > 0, r, slope * r)
            keep = (ref[z, m, :N] > 0) & bool(mask[z, m])       # then relu_ref, then rowmask
            exp[mo, :N] = np.where(keep, r, 0.0)
            assert np.all(got[z, mo, :N][~keep] == 0.0), (tag, z, m)
        close(tag + " " + feature, dev, got[z, written, :N], exp[written, :N])
        rest = got[z].copy()
        rest[written, :N] = old[z][written, :N]
        assert np.array_equal(rest.view(np.uint32), old[z].view(np.uint32)), (tag, z)   # dropped rows, gap rows, columns >= N


@pytest.mark.parametrize("feature", ["rowmask", "relu_ref", "rowmap", "lrelu0.2", "lrelu0.01", "all"])
def test_epilogue(dev, feature):
    check_epilogue(dev, feature)


# ---- (e) column-sum tile ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [5, 65])
@pytest.mark.parametrize("N", [64, 70])
@pytest.mark.parametrize("groups", [1, 8])
def test_colsum_tile(dev, groups, N, M):
    g = np.random.RandomState(500 + groups + N + M)
    Ks = K_RAGGED[groups]
    mK = max(Ks)
    t = Task(dev, g, TN, [M] * groups, N, Ks)
    dd, _ = dims_dev(dev, Ks)
    w = (100.0 * g.standard_normal((groups, mK, 4))).astype(np.float32)   # columns 1..3: garbage that must be ignored
    w[:, :, 0] = g.rand(groups, mK) > 0.4
    for z in range(groups):
        w[z, Ks[z]:] = np.nan
    cs_ld = pad4(M) + 4
    cs = dev.empty((groups, cs_ld), fill=SENT)
    plain, out = t.out(), t.out()
    kw = dict(dimptr=dd, dim_stride=3, dim_sel=2)
    launch(dev, [t.desc(plain, **kw)])
    assert launch(dev, [t.desc(out, colsum=cs, colsum_gs=cs_ld, colsum_w=dev.put(w), colsum_w_gs=mK * 4, **kw)])[0][0] == 1   # (a launch with a column-sum tile never splits K)
    got, gcs = dev.get(out), dev.get(cs)
    t.check("e colsum C", got)
    assert np.array_equal(got.view(np.uint32), dev.get(plain).view(np.uint32))   # C as without the column-sum tile, bit for bit
    A = t.src[0][0]
    for z in range(groups):
        K = Ks[z]
        if K == 0:
            assert untouched(gcs[z])    # a skipped group (module docstring)
            continue
        want = (A[z, :K, :M].astype(np.float64) * w[z, :K, 0].astype(np.float64)[:, None]).sum(0)
        close("e colsum", dev, gcs[z, :M], want)
        assert untouched(gcs[z, M:])


# ---- (f) dilated A-taps -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cin,dil,dual", [(c, d, False) for c in (32, 64) for d in (1, 3, 9)] + [(32, 3, True)])
def test_dilated_a_taps(dev, Cin, dil, dual):
    L, Cout, taps = 97, 48, 3
    g = np.random.RandomState(600 + Cin + dil + dual)
    want = np.zeros((L, Cout))
    srcs = []
    for _ in range(2 if dual else 1):
        x = np.zeros((L + 2 * dil, Cin), np.float32)
        x[dil:dil + L] = g.standard_normal((L, Cin))
        w = g.standard_normal((Cout, taps, Cin)).astype(np.float32)   # B[n][tap * Cin + cin]
        want += torch.nn.functional.conv1d(torch.from_numpy(x.T.astype(np.float64))[None], torch.from_numpy(w.astype(np.float64)).permute(0, 2, 1),
                                           dilation=dil)[0].T.numpy()
        srcs.append((dev.put(x), dev.put(w)))
    bias = g.standard_normal(Cout).astype(np.float32)
    out = dev.empty((L + 3, Cout + 4), fill=SENT)
    kw = dict(A2=srcs[1][0], B2=srcs[1][1]) if dual else {}
    d = desc(dev, NT, srcs[0][0], srcs[0][1], out, L, Cout, taps * Cin, Cin, taps * Cin, Cout + 4, a_tap_k=Cin, a_tap_rows=dil, bias=dev.put(bias), **kw)
    assert launch(dev, [d])[0][0] == 1
    got = dev.get(out)
    close("f dilated taps", dev, got[:L, :Cout], want + bias.astype(np.float64)[None, :], dual)
    assert untouched(got[L:]) and untouched(got[:, Cout:])


# ---- (g) split-K on the caller's workspace ----------------------------------------------------------------------------------------------
_WS = {}


def splitk_ws(dev):
    """(slab, counters) of the sizes the launcher's bounds assume, one per arm: the slab holds the sentinel, the counters zero"""
    if dev.gpu not in _WS:
        _WS[dev.gpu] = (dev.empty(int(dev.lib.mtts_gemm_splitk_ws_bytes()) // 4, fill=SENT), dev.empty(int(dev.lib.mtts_gemm_splitk_ctr_bytes()) // 4, np.int32))
    slab, ctr = _WS[dev.gpu]
    slab[:] = float(SENT)
    ctr[:] = 0
    return slab, ctr


def slab_tile(slab, slot, S):
    """the 64 x 64 tile that slab_combine hands to the epilogue: the S partial tiles of `slot` summed in split order, in fp32.

    This pins an INTERNAL layout, defined in csrc/gemm.h by splitk_combine / slab_combine (the slab: [slot][split][r4][thread][4 floats],
    slot = group * tiles + tile) and by the accumulator-to-C mapping of gemm_epilogue (row / column of accumulator r of a thread).  A
    deliberate re-layout of the slab has to change this function with it; the in-order sum it proves is the property that must stay."""
    part = slab[slot * S * 4096:(slot + 1) * S * 4096].reshape(S, 4, 256, 4)   # [split][r4][thread][e]: accumulator 4 r4 + e of the thread
    acc = np.zeros((4, 256, 4), np.float32)
    for s in range(S):
        acc = acc + part[s]
    tid = np.arange(256)
    wave, lane = tid >> 6, tid & 63
    tile = np.zeros((64, 64), np.float32)
    for r4 in range(4):
        for e in range(4):
            r = 4 * r4 + e
            tile[(wave // 2) * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), (wave % 2) * 32 + (lane & 31)] = acc[r4, :, e]
    return tile


def check_workspace_tail(dev, ws, slots, S):
    slab, ctr = dev.get(ws[0]), dev.get(ws[1])
    assert untouched(slab[slots * S * 4096:])
    assert not np.any(ctr)    # beyond `slots`: never touched; the used ones: re-armed by the last arriver


SPLIT_S = {(False, 530): 2, (False, 1100): 4, (False, 2100): 8, (True, 530): 4, (True, 1100): 8, (True, 2100): 8}   # gemm_batch_end's rule, K-loop of a dual problem = 2 K


def check_splitk(dev, form, dual, K, family=0):
    M, N = 70, 40
    g = np.random.RandomState(700 + form + 10 * dual + K)
    t = Task(dev, g, form, [M], N, [K], n_src=2 if dual else 1)
    tag = "g split-K" + (" lds-dma" if family else "")
    ws = splitk_ws(dev)
    out = t.out()
    S = SPLIT_S[(dual, K)]
    assert launch(dev, [t.desc(out, alpha=0.5)], family, ws)[0][0] == S
    first = dev.get(out).copy()
    t.check(tag, first, 0.5)
    check_workspace_tail(dev, ws, 2, S)
    # the same call again on the same workspace, counters not re-zeroed: the last arriver re-armed them and sums in split order
    out2 = t.out()
    assert launch(dev, [t.desc(out2, alpha=0.5)], family, ws)[0][0] == S
    assert np.array_equal(dev.get(out2).view(np.uint32), first.view(np.uint32))
    check_workspace_tail(dev, ws, 2, S)
    # alpha = 1, no bias: C is the sum of the slab's partial tiles IN SPLIT ORDER, bit for bit (whichever workgroup arrived last)
    t.dbias = t.bias = None
    out3 = t.out()
    assert launch(dev, [t.desc(out3)], family, ws)[0][0] == S
    got, slab = dev.get(out3), dev.get(ws[0])
    for m_tile in range(2):
        rows = min(64, M - 64 * m_tile)
        tile = slab_tile(slab, m_tile, S)
        assert np.array_equal(got[0, 64 * m_tile:64 * m_tile + rows, :N].view(np.uint32), tile[:rows, :N].view(np.uint32)), (tag, m_tile)
    # without a workspace K is not split, and the result still matches
    out4 = t.out()
    assert launch(dev, [t.desc(out4)], family)[0][0] == 1
    t.check(tag + " (S = 1)", dev.get(out4))


@pytest.mark.parametrize("K", [530, 1100, 2100])
@pytest.mark.parametrize("form,dual", [(NT, False), (NN, False), (TN, False), (NT, True)])
def test_splitk(dev, form, dual, K):
    check_splitk(dev, form, dual, K)


def test_splitk_ragged_groups(dev):
    g = np.random.RandomState(777)
    Ms = [65, 0, 130]
    t = Task(dev, g, NT, Ms, 40, [1100] * 3)
    dd, _ = dims_dev(dev, Ms)
    ws = splitk_ws(dev)
    for _ in range(2):
        out = t.out()
        (S, place), = launch(dev, [t.desc(out, dimptr=dd, dim_stride=3, dim_sel=0)], 0, ws)
        assert S >= 2
        t.check("g split-K groups", dev.get(out))
        check_workspace_tail(dev, ws, 3 * 3, S)


def test_splitk_full_epilogue(dev):
    check_epilogue(dev, "all", K=1100, ws=splitk_ws(dev), want_split=True)


# ---- (h) placement changes nothing ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [NT, TN])
def test_task_per_xcd_schedule_is_placement_only(dev, form):
    g = np.random.RandomState(800 + form)
    if form == NT:
        dims = M_RAGGED[8]
        t = Task(dev, g, NT, dims, 80, [36] * 8)
    else:
        dims = K_RAGGED[8]
        t = Task(dev, g, TN, [70] * 8, 40, dims)
    dd, hd = dims_dev(dev, dims)
    kw = dict(dimptr=dd, dim_stride=3, dim_sel=form)
    a, b = t.out(), t.out()
    assert launch(dev, [t.desc(a, host_dims=hd, **kw)]) == [(1, 1)]
    assert launch(dev, [t.desc(b, **kw)])[0] in [(1, 0), (1, 2)]
    ga, gb = dev.get(a), dev.get(b)
    t.check("h schedule", ga)
    assert np.array_equal(ga.view(np.uint32), gb.view(np.uint32))


@pytest.mark.parametrize("K,split", [(100, False), (1100, True)])
def test_panel_order(dev, K, split):
    g = np.random.RandomState(850 + K)
    t = Task(dev, g, NT, [33, 33], 130, [K, K])   # N K > M lda: the B operand is the bigger one
    ws = splitk_ws(dev) if split else None
    out = t.out()
    (S, place), = launch(dev, [t.desc(out)], 0, ws)
    assert place == 2 and (S >= 2) == split
    t.check("h panel order", dev.get(out))
    if split:
        check_workspace_tail(dev, ws, 2 * 3, S)


# ---- (i) multi-problem launch -----------------------------------------------------------------------------------------------------------
def multi_problems(dev, g):
    """-> [(name, descriptor factory(out...), buffers factory, checker)] of six independent problems"""
    probs = []
    # NT with a row mask
    t0 = Task(dev, g, NT, [70, 70], 40, [36, 36])
    mask = (g.rand(2, 70) > 0.3).astype(np.uint8)
    dmask = dev.put(mask)

    def chk0(o):
        got = dev.get(o[0])
        for z in range(2):
            close("i multi NT", dev, got[z, :70, :40], t0.want(z) * mask[z][:, None])
            assert np.all(got[z, :70, :40][mask[z] == 0] == 0.0) and untouched(got[z, 70:]) and untouched(got[z, :, 40:])
    probs.append((lambda: [t0.out()], lambda o: t0.desc(o[0], rowmask=dmask, rowmask_gs=70), chk0))
    # NN with the conv input-gradient tap walk (mtts_conv1d_f32 mode 1)
    L, Cin, Cout, k = 97, 32, 48, 3
    dy = np.zeros((L + 2, Cout), np.float32)
    dy[1:1 + L] = g.standard_normal((L, Cout))
    w = g.standard_normal((Cout, k, Cin)).astype(np.float32)
    x64 = torch.zeros(1, Cin, L, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv1d(x64, torch.from_numpy(w.astype(np.float64)).permute(0, 2, 1), padding=1).backward(torch.from_numpy(dy[1:1 + L].T.astype(np.float64))[None])
    dx = x64.grad[0].T.numpy()
    ddy, dw = dev.put(dy), dev.put(w)

    def chk1(o):
        got = dev.get(o[0])
        close("i multi NN taps", dev, got[:L, :Cin], dx)
        assert untouched(got[L:]) and untouched(got[:, Cin:])
    probs.append((lambda: [dev.empty((L + 3, Cin + 4), fill=SENT)],
                  lambda o: desc(dev, NN, addr(dev, ddy, 0), dw, o[0], L, Cin, k * Cout, Cout, k * Cin, Cin + 4, taps=k, tap_k=Cout, tap_bstride=Cin), chk1))
    # TN with the column-sum tile, 8 ragged groups
    Ks = K_RAGGED[8]
    t2 = Task(dev, g, TN, [65] * 8, 70, Ks)
    dd, _ = dims_dev(dev, Ks)
    cw = np.zeros((8, 100, 4), np.float32)
    cw[:, :, 0] = g.rand(8, 100) > 0.4
    dcw = dev.put(cw)

    def chk2(o):
        t2.check("i multi TN", dev.get(o[0]))
        cs = dev.get(o[1])
        for z in range(8):
            if Ks[z]:
                close("i multi colsum", dev, cs[z, :65], (t2.src[0][0][z, :Ks[z], :65].astype(np.float64) * cw[z, :Ks[z], 0:1]).sum(0))
                assert untouched(cs[z, 65:])
            else:
                assert untouched(cs[z])
    probs.append((lambda: [t2.out(), dev.empty((8, 72), fill=SENT)],
                  lambda o: t2.desc(o[0], dimptr=dd, dim_stride=3, dim_sel=2, colsum=o[1], colsum_gs=72, colsum_w=dcw, colsum_w_gs=400), chk2))
    # dual-source NT
    t3 = Task(dev, g, NT, [33], 130, [100], n_src=2)
    probs.append((lambda: [t3.out()], lambda o: t3.desc(o[0], alpha=0.5), lambda o: t3.check("i multi dual", dev.get(o[0]), 0.5)))
    # (the cap of six) ragged-M NN groups and a plain TN
    Ms = [65, 0, 130]
    t4 = Task(dev, g, NN, Ms, 80, [36] * 3)
    dd4, _ = dims_dev(dev, Ms)
    probs.append((lambda: [t4.out()], lambda o: t4.desc(o[0], dimptr=dd4, dim_stride=3, dim_sel=0), lambda o: t4.check("i multi NN", dev.get(o[0]))))
    t5 = Task(dev, g, TN, [70], 40, [530])
    probs.append((lambda: [t5.out()], lambda o: t5.desc(o[0]), lambda o: t5.check("i multi TN plain", dev.get(o[0]))))
    return probs


@pytest.mark.parametrize("n", [4, 6])
def test_multi_problem_launch(dev, n):
    g = np.random.RandomState(900)
    probs = multi_problems(dev, g)[:n]
    outs = [p[0]() for p in probs]
    rep = launch(dev, [p[1](o) for p, o in zip(probs, outs)])
    assert all(S == 1 for S, _ in rep)
    for p, o in zip(probs, outs):
        p[2](o)
        alone = p[0]()
        assert launch(dev, [p[1](alone)])[0][0] == 1
        for x, y in zip(o, alone):
            assert np.array_equal(dev.get(x).view(np.uint32), dev.get(y).view(np.uint32))   # the same problem launched alone: bit-identical


# ---- (j) bad arguments ------------------------------------------------------------------------------------------------------------------
def test_bad_arguments(dev):
    g = np.random.RandomState(1000)
    t = Task(dev, g, NT, [70], 40, [36])
    tn = Task(dev, g, TN, [70], 40, [36])
    out = t.out()
    dd, _ = dims_dev(dev, [70])
    tab = dev.put(np.frombuffer(bytes(Group(0, 0, 0, 70, 40, 36, 0, 0, 0)), np.uint8).copy())
    cs, cw = dev.empty(80, fill=SENT), dev.empty((36, 4))

    def rc(descs, family=0, ws=None, ctr=None):
        arr = (Desc * len(descs))(*descs)
        return dev.lib.mtts_gemm_f32_grouped(C.addressof(arr), len(descs), family, ws, ctr, None, None)

    def broken(**kw):
        d = t.desc(out)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    bad = [[broken(A=None)], [broken(B=None)], [broken(C=None)], [broken(form=3)], [broken(form=-1)], [broken(groups=0)],
           [t.desc(out)] * 7,
           [t.desc(out, colsum=cs, colsum_w=cw)],                        # colsum on a non-TN form
           [broken(form=NN, colsum=addr(dev, cs), colsum_w=addr(dev, cw))],
           [t.desc(out, a_tap_k=48, a_tap_rows=1)],                       # a_tap_k % 32 != 0
           [t.desc(out, table=tab, dimptr=dd)]]
    # ... and what the entry refuses beyond that list (include/mtts.h), each a descriptor the launcher could not run as the caller meant it
    hd = np.array([70], np.int32)
    bad += [[broken(A2=addr(dev, t.src[0][2]))], [broken(B2=addr(dev, t.src[0][3]))],      # one of A2 / B2 without the other
            [broken(flags=8)], [broken(max_M=0)], [broken(max_N=0)],
            [tn.desc(out, colsum=cs, colsum_w=cw, table=tab)],             # colsum with a table
            [tn.desc(out, colsum=cs)],                                     # colsum without its weights
            [tn.desc(out, a_tap_k=32, a_tap_rows=1)],                      # the A-tap walk on the TN form
            [t.desc(out, a_tap_k=0, a_tap_rows=1)],
            [t.desc(out, host_dims=hd)],                                   # host_dims without dimptr
            [t.desc(out, dimptr=dd, dim_stride=0)], [t.desc(out, dimptr=dd, dim_mult=0)], [t.desc(out, dimptr=dd, dim_sel=1)],
            [t.desc(out, relu_ref=cw, ld_relu=0)],
            [t.desc(out, taps=3, tap_k=12, tap_bstride=40)],               # the B-tap walk on a form other than NN
            [broken(form=NN, taps=3, tap_k=0, tap_bstride=40)]]
    for i, descs in enumerate(bad):
        assert rc(descs) != 0, i
    assert rc([t.desc(out)], family=16) != 0 and rc([t.desc(out)], family=-1) != 0
    assert rc([t.desc(out)], ws=dev.ptr(cs)) != 0 and rc([t.desc(out)], ctr=dev.ptr(cs)) != 0   # half a split-K workspace
    if dev.gpu:   # a forced LDS-DMA family refuses what those kernels cannot take ...
        assert rc([broken(form=NN, taps=3, tap_k=12, tap_bstride=40)], family=4064) != 0
    else:         # ... and does not exist in the emulator build
        assert rc([t.desc(out)], family=4064) != 0
    assert dev.lib.mtts_gemm_f32_grouped(None, 1, 0, None, None, None, None) != 0
    assert dev.lib.mtts_gemm_f32_grouped(C.addressof((Desc * 1)(t.desc(out))), 0, 0, None, None, None, None) != 0
    if dev.gpu:
        torch.cuda.synchronize()
    assert untouched(dev.get(out)) and untouched(dev.get(cs))
    # ... and the same descriptors, unbroken, are accepted
    assert rc([t.desc(out)]) == 0
    out_tn = tn.out()
    assert rc([tn.desc(out_tn, colsum=cs, colsum_w=cw)]) == 0
    t.check("j accepted", dev.get(out))


# ---- the forced LDS-DMA family (device build only) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,groups", [(NT, 8), (NN, 3)])
def test_lds_dma_task_groups_ragged_m(gdev, form, groups):
    check_ragged_m(gdev, form, groups, 1, family=4064)


@pytest.mark.parametrize("feature", ["rowmap", "all"])
def test_lds_dma_epilogue(gdev, feature):
    check_epilogue(gdev, feature, family=4064)


@pytest.mark.parametrize("form,dual,K", [(NT, False, 530), (NN, False, 1100), (TN, False, 2100), (NT, True, 1100)])
def test_lds_dma_splitk(gdev, form, dual, K):
    check_splitk(gdev, form, dual, K, family=4064)
