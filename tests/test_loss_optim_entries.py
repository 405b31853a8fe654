"""The loss and optimizer kernels of csrc/rowops.h through their C entries (include/mtts.h: mtts_rows_loss, mtts_rows_loss_grad, mtts_sumsq_norm,
mtts_adam_clip, mtts_sgd_update, mtts_sum_tasks, mtts_broadcast) against float64 restatements of the reference formulas written out here:
model/loss.py:19-92 (masked L1 / MSE means and their sum), optimizer.py:9-15 + main.py:61 (clip_grad_norm_ then torch.optim.Adam),
systems/utils.py:39-47 (theta' = theta - lr g), main.py:62 (gradient accumulation).

Loss: 1 task and 3 ragged tasks whose Mr, Mp, nF and nP all differ, invalid rows inside Mr and Mp, every (pitch, energy) level combination;
inputs behind a task's rows and the inputs of a switched-off level are NaN, outputs behind the rows hold a sentinel.  The six loss scalars
and Adam's w, m, v are held to the project's arbiter rule (rowtask_util.arbiter_ok); every gradient element to a bound from the fp32 operation
count of its formula; sums to n * 2^-24 * sum|terms| + one ulp.  The same checks run on the SIMT emulator and, marked gpu, on the device."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
from oracle_util import Dev
from rowtask_util import EPS, SENT, arbiter_ok, assert_within, i32, i64, pack, stride_of, sum_bound, ulp32, unpack

F32 = np.float32
F = lambda x: float(F32(x))   # a hyper-parameter as the fp32 value the C entry receives


@pytest.fixture(params=[pytest.param(False, id="emu"), pytest.param(True, id="gpu", marks=pytest.mark.gpu)])
def dev(request):
    if request.param:
        ge.build_device()
    return Dev(request.param)


# ------------------------------------------------------------------------------------------------------------------------------- loss
# Mr 901 with n_mel 80: 18020 float4 > 64 workgroups x 256 threads, a second grid-stride trip with a ragged tail; no Mr is a multiple of 256
LOSS_ROWS = {1: dict(Mr=(901,), Mp=(37,)), 3: dict(Mr=(901, 13, 410), Mp=(37, 3, 21))}
SCALE = F(1.0 / 3.0)


def loss_formula(d, n_mel, pf, ef, dtype, scale=None):
    """loss.py:19-92 for one task in `dtype`: (six scalars, gradients of scale * total w.r.t. the predictions or None)"""
    T = lambda k: torch.from_numpy(d[k].astype(np.float64)).to(dtype)
    rm, pm = torch.from_numpy(d["rvalid"] != 0), torch.from_numpy(d["pvalid"] != 0)
    names = ["mel", "post", "pp", "ep", "logd"] + (["pp_r"] if pf else []) + (["ep_r"] if ef else [])
    x = {k: T(k).requires_grad_(scale is not None) for k in names}
    tgt = T("tgt")
    l1 = lambda a: (a - tgt).abs().masked_select(rm[:, None]).mean()
    mse = lambda a, b, m: ((a.masked_select(m) - b.masked_select(m)) ** 2).mean()
    pitch = mse(x["pp_r"], T("p_tgt_r"), rm) if pf else mse(x["pp"], T("p_tgt"), pm)
    energy = mse(x["ep_r"], T("e_tgt_r"), rm) if ef else mse(x["ep"], T("e_tgt"), pm)
    dur = mse(x["logd"], torch.log(torch.from_numpy(d["dur"]).to(dtype) + 1), pm)
    mel, post = l1(x["mel"]), l1(x["post"])
    total = mel + post + dur + pitch + energy
    out = np.array([float(v.detach()) for v in (total, mel, post, pitch, energy, dur)], np.float64)
    grads = None
    if scale is not None:
        gs = torch.autograd.grad(total * scale, [x[k] for k in names], allow_unused=True)
        grads = {k: (np.zeros(d[k].shape) if gv is None else gv.numpy()) for k, gv in zip(names, gs)}
    return out, grads


@functools.lru_cache(maxsize=None)
def loss_case(tasks, n_mel, pf, ef):
    """inputs of every task and their float64 / fp32 references, computed once per case and shared by the emulator and the device run"""
    g = np.random.RandomState(100 * tasks + n_mel + 2 * pf + ef)
    R = LOSS_ROWS[tasks]
    data = []
    for Mr, Mp in zip(R["Mr"], R["Mp"]):
        d = {}
        d["rvalid"] = (g.rand(Mr) > 0.25).astype(np.uint8)
        d["pvalid"] = (g.rand(Mp) > 0.25).astype(np.uint8)
        d["rvalid"][0] = d["pvalid"][0] = 1
        if Mr > 3:
            d["rvalid"][1], d["rvalid"][Mr - 1] = 0, 1
        if Mp > 2:
            d["pvalid"][1], d["pvalid"][Mp - 1] = 0, 1
        for k in ("mel", "post", "tgt"):
            d[k] = g.standard_normal((Mr, n_mel)).astype(F32)
        d["mel"][0, :5] = d["tgt"][0, :5]              # mel == target exactly: the gradient is exactly 0 there (torch.sign)
        d["post"][0, 3:9] = d["tgt"][0, 3:9]
        d["mel"][Mr - 1, n_mel - 1] = d["tgt"][Mr - 1, n_mel - 1]
        for k in ("pp", "ep", "logd", "p_tgt", "e_tgt"):
            d[k] = g.standard_normal(Mp).astype(F32)
        d["logd"] = np.abs(d["logd"]) + F32(0.5)
        d["dur"] = g.randint(0, 10, Mp).astype(np.int32)
        d["dur"][0] = 0
        for k in ("pp_r", "ep_r", "p_tgt_r", "e_tgt_r"):
            d[k] = g.standard_normal(Mr).astype(F32)
        d["nF"], d["nP"] = int(d["rvalid"].sum()), int(d["pvalid"].sum())
        assert d["nF"] < Mr or Mr < 4
        d["ref64"], d["grad64"] = loss_formula(d, n_mel, pf, ef, torch.float64, SCALE)
        d["ref32"], _ = loss_formula(d, n_mel, pf, ef, torch.float32)
        data.append(d)
    if tasks == 3:
        assert len({d["nF"] for d in data}) == 3 and len({d["nP"] for d in data}) == 3
    return data


class LossBufs:
    def __init__(self, dev, data, n_mel, pf, ef):
        R_ = [len(d["rvalid"]) for d in data]
        P_ = [len(d["pvalid"]) for d in data]
        self.Mr, self.Mp, self.T = R_, P_, len(data)
        capR, capP = max(R_) + 2, max(P_) + 2
        self.ts = dict(mel=stride_of(capR * n_mel), rrow=stride_of(capR, 4), prow=stride_of(capP, 4), pred=stride_of(capP, 12), pred_r=stride_of(capR, 12))
        put = lambda k, st, fill, dt=F32: dev.put(pack([d[k] for d in data], self.ts[st], fill, dt))
        nan_if = lambda off, k, st: dev.put(np.full(self.T * self.ts[st], np.nan, F32)) if off else put(k, st, np.nan)
        self.inputs = [put("mel", "mel", np.nan), put("post", "mel", np.nan), put("tgt", "mel", np.nan), put("rvalid", "rrow", 1, np.uint8),
                       nan_if(pf, "pp", "pred"), nan_if(ef, "ep", "pred"), put("logd", "pred", np.nan), nan_if(pf, "p_tgt", "prow"), nan_if(ef, "e_tgt", "prow"),
                       put("dur", "prow", 0, np.int32), put("pvalid", "prow", 1, np.uint8),
                       nan_if(not pf, "pp_r", "pred_r"), nan_if(not ef, "ep_r", "pred_r"), nan_if(not pf, "p_tgt_r", "rrow"), nan_if(not ef, "e_tgt_r", "rrow")]
        self.ptr = (C.c_void_p * 15)(*[dev.ptr(x).value for x in self.inputs])
        self.ts_arr = i64([self.ts[k] for k in ("mel", "rrow", "prow", "pred", "pred_r")])
        self.counts = (i32(R_), i32(P_), i32([d["nF"] for d in data]), i32([d["nP"] for d in data]))
        self.ws = dev.ws(max(max(R_), max(P_)))


@pytest.mark.parametrize("pf,ef", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("n_mel", [32, 80])
@pytest.mark.parametrize("tasks", [1, 3])
def test_loss_and_gradient(dev, tasks, n_mel, pf, ef):
    data = loss_case(tasks, n_mel, pf, ef)
    b, P = LossBufs(dev, data, n_mel, pf, ef), dev.ptr
    losses = dev.empty((tasks + 1, 6), fill=SENT)
    assert dev.lib.mtts_rows_loss(tasks, *b.counts, n_mel, pf, ef, b.ptr, b.ts_arr, P(losses), P(b.ws), None) == 0
    got = dev.get(losses)
    assert np.all(got[tasks] == SENT)
    for t, d in enumerate(data):
        # the arbiter rule on the six scalars total, mel, postnet mel, pitch, energy, duration of a task.  Observed ratio
        # max(err_kernel - ulp, 0) / err_torch32 over all 16 cases: at most 0.85 on the emulator, at most 1.20 on the MI355X (limit 3).
        arbiter_ok(got[t], d["ref32"], d["ref64"], f"loss task {t}")
    # gradients of SCALE * total
    outs = dict(mel=("mel", n_mel), post=("mel", n_mel), pp=("pred", 0), ep=("pred", 0), logd=("pred", 0), pp_r=("pred_r", 0), ep_r=("pred_r", 0))
    bufs = {k: dev.put(np.full(tasks * b.ts[st], SENT, F32)) for k, (st, _) in outs.items()}
    assert dev.lib.mtts_rows_loss_grad(tasks, *b.counts, n_mel, pf, ef, b.ptr, b.ts_arr, C.c_float(SCALE), P(bufs["mel"]), P(bufs["post"]), P(bufs["pp"]),
                                       P(bufs["ep"]), P(bufs["logd"]), P(bufs["pp_r"]), P(bufs["ep_r"]), P(b.ws), None) == 0
    res = {}
    for k, (st, w) in outs.items():
        n = b.Mr if st in ("mel", "pred_r") else b.Mp
        res[k], rest = unpack(dev.get(bufs[k]), b.ts[st], [(r, w) if w else (r,) for r in n])
        assert np.all(rest == SENT), k
    for t, d in enumerate(data):
        rv, pv, G = d["rvalid"] != 0, d["pvalid"] != 0, d["grad64"]
        for k in ("mel", "post"):
            # w = scale / (nF * n_mel): the product is exact, one rounding in the division, times a sign: within one ulp
            assert_within(res[k][t], G[k], ulp32(G[k]), f"d{k}")
            assert np.all(res[k][t][~rv] == 0)
            assert np.all(res[k][t][d[k] == d["tgt"]] == 0) and (d[k] == d["tgt"])[rv].sum() >= 5
        # w (pred - target): a division, a difference and a product, three roundings of relative size 2^-24 each.  The duration target
        # logf(dur + 1) adds the error of an fp32 log, bounded by 2 ulp of the target (HIP documents 1 ulp for logf), times w = 2 scale / nP.
        wP = 2.0 * SCALE / d["nP"]
        logt = np.log(d["dur"].astype(np.float64) + 1.0)
        for k, extra in (("pp", 0.0), ("ep", 0.0), ("logd", wP * 2.0 * ulp32(logt) * (logt > 0))):
            if (k == "pp" and pf) or (k == "ep" and ef):
                assert np.all(res[k][t] == 0) and np.all(G[k] == 0)      # the level is switched off here: exactly 0, NaN inputs never read
                continue
            assert_within(res[k][t], G[k], 3.01 * EPS * np.abs(G[k]) + extra, f"d{k}")
            assert np.all(res[k][t][~pv] == 0) and np.any(res[k][t][pv] != 0)
        for k, on in (("pp_r", pf), ("ep_r", ef)):
            if not on:
                assert np.all(res[k][t] == SENT)    # a phoneme-level feature has no frame-level gradient: the kernel leaves that buffer alone
                continue
            assert_within(res[k][t], G[k], 3.01 * EPS * np.abs(G[k]), f"d{k}")
            assert np.all(res[k][t][~rv] == 0) and np.any(res[k][t][rv] != 0)


# -------------------------------------------------------------------------------------------------------------------------- optimizer
def flat_case(seed, n4, tasks=1):
    g = np.random.RandomState(seed)
    return [g.standard_normal(4 * n4).astype(F32) for _ in range(tasks)]


@pytest.mark.parametrize("with_extra", [False, True])
@pytest.mark.parametrize("n4,n_partials", [(3 * 256 * 40 + 301, 3), (77, 2), (512, 512)])
def test_sumsq_norm(dev, n4, n_partials, with_extra):
    """3 workgroups over 31021 float4: 40 full grid-stride trips and a ragged 41st; 77 float4 on 2 workgroups: the second one idle; the engine's
    512 partials with one float4 each"""
    P = dev.ptr
    gr = flat_case(n4, n4)[0] * F32(0.05)
    extra = np.array([3.7], F32)
    partial, out = dev.empty(n_partials + 2, fill=SENT), dev.empty(2, fill=SENT)
    assert dev.lib.mtts_sumsq_norm(P(dev.put(gr)), n4, n_partials, P(dev.put(extra)) if with_extra else None, P(partial), P(out), None) == 0
    got = dev.get(out)
    assert got[1] == SENT and np.all(dev.get(partial)[n_partials:] == SENT)
    S = float((gr.astype(np.float64) ** 2).sum())
    tot = S + (float(extra[0]) if with_extra else 0.0)
    ref = np.sqrt(tot)
    # fp32 chain of one term: its square, the float4's pair tree (2), the thread's running sum (one add per trip), the wavefront tree (6), the
    # workgroup's (2); the partials are then added in double.  |dS| <= n 2^-24 S, d(sqrt) = dS / (2 sqrt)
    trips = -(-n4 // (n_partials * 256))
    n = 1 + 2 + trips + 6 + 2
    assert_within(got[0], ref, n * EPS * S / (2 * ref) + ulp32(ref), "sumsq_norm")


def adam_f64(w, g, m, v, max_norm, lr, b1, b2, eps, wd, step):
    """clip_grad_norm_(max_norm) then one torch.optim.Adam step, written out in float64"""
    w, g, m, v = (a.astype(np.float64) for a in (w, g, m, v))
    if max_norm > 0:
        g = g * min(max_norm / (np.sqrt((g * g).sum()) + 1e-6), 1.0)
    if wd != 0:
        g = g + wd * w
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    return w - (lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + eps), m, v


def adam_torch(w, g, m, v, max_norm, lr, b1, b2, eps, wd, step, dtype):
    p = torch.nn.Parameter(torch.from_numpy(w.astype(np.float64)).to(dtype))
    p.grad = torch.from_numpy(g.astype(np.float64)).to(dtype)
    if max_norm > 0:
        torch.nn.utils.clip_grad_norm_([p], max_norm)
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    opt.state[p] = dict(step=torch.tensor(float(step - 1)), exp_avg=torch.from_numpy(m.astype(np.float64)).to(dtype),
                        exp_avg_sq=torch.from_numpy(v.astype(np.float64)).to(dtype))
    opt.step()
    return p.detach().numpy(), opt.state[p]["exp_avg"].numpy(), opt.state[p]["exp_avg_sq"].numpy()


@pytest.mark.parametrize("step", [1, 7])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("clip", ["below", "above", "off"])
def test_adam_clip(dev, clip, wd, step):
    """norm below max_norm (coef 1), above it, and max_norm 0 (no clip); 3 workgroups over 1837 float4: two full trips and a ragged third"""
    P = dev.ptr
    n4, max_blocks = 3 * 256 * 2 + 301, 3
    rs = np.random.RandomState(7 * step + len(clip))
    w, gr = (rs.standard_normal(4 * n4).astype(F32) for _ in range(2))
    gr *= F32((0.5 if clip == "below" else 5.0) / np.sqrt((gr.astype(np.float64) ** 2).sum()))
    m = (0.1 * rs.standard_normal(4 * n4)).astype(F32) if step > 1 else np.zeros(4 * n4, F32)
    v = (0.01 * rs.standard_normal(4 * n4) ** 2).astype(F32) if step > 1 else np.zeros(4 * n4, F32)
    max_norm = 0.0 if clip == "off" else 1.0
    hp = dict(max_norm=max_norm, lr=F(1e-3), b1=F(0.9), b2=F(0.98), eps=F(1e-9), wd=F(wd), step=step)
    dw, dm, dv, dg = (dev.put(np.concatenate([a, np.full(8, SENT, F32)])) for a in (w, m, v, gr))
    partial, norm = dev.empty(8), dev.empty(1)
    assert dev.lib.mtts_sumsq_norm(P(dg), n4, 8, None, P(partial), P(norm), None) == 0
    assert dev.lib.mtts_adam_clip(P(dw), P(dg), P(dm), P(dv), n4, P(norm), hp["max_norm"], hp["lr"], hp["b1"], hp["b2"], hp["eps"], step, hp["wd"], max_blocks,
                                  None) == 0
    ref = adam_f64(w, gr, m, v, **hp)
    t64 = adam_torch(w, gr, m, v, dtype=torch.float64, **hp)
    t32 = adam_torch(w, gr, m, v, dtype=torch.float32, **hp)
    for name, buf, r, a64, a32 in zip("wmv", (dw, dm, dv), ref, t64, t32):
        got = dev.get(buf)
        assert np.all(got[4 * n4:] == SENT), name
        np.testing.assert_allclose(r, a64, rtol=1e-9, atol=1e-13 * np.abs(r).max())     # the written-out formula IS torch's Adam (both float64)
        # Observed ratio max(err_kernel - ulp, 0) / err_torch32 over the 12 cases, emulator and MI355X alike: w at most 0.16, m at most 0.26,
        # v at most 0.56 (limit 3).
        arbiter_ok(got[:4 * n4], a32, r, f"adam {name} clip={clip} wd={wd} step={step}")
    assert (float(dev.get(norm)[0]) > 1.0) == (clip != "below")


def test_sgd_update_sum_tasks_broadcast(dev):
    """3 tasks at distinct strides, 2 workgroups over 1101 float4: two full grid-stride trips and a ragged third; the gaps between the tasks stay"""
    P = dev.ptr
    tasks, n4, mb = 3, 2 * 256 * 2 + 77, 2
    n = 4 * n4
    w, gr = flat_case(1, n4, tasks), flat_case(2, n4, tasks)
    w_ts, g_ts, d_ts = stride_of(n, 8), stride_of(n, 24), stride_of(n, 40)
    lr = F(0.37)
    dw = dev.put(pack(w, w_ts, SENT, F32))
    dg = dev.put(pack(gr, g_ts, np.nan, F32))
    assert dev.lib.mtts_sgd_update(tasks, P(dw), w_ts, P(dg), g_ts, n4, lr, mb, None) == 0
    got, rest = unpack(dev.get(dw), w_ts, [(n,)] * tasks)
    assert np.all(rest == SENT)
    for t in range(tasks):
        step = lr * gr[t].astype(np.float64)
        ref = w[t] - step
        # w - lr g: a product and a difference, fused or not: at most one rounding of each
        assert_within(got[t], ref, EPS * (np.abs(step) + np.abs(ref)) * 1.01, "sgd_update")
    for accumulate, scale in ((0, F(0.125)), (1, F(1.7)), (0, 1.0)):
        prev = flat_case(3, n4)[0]
        out = dev.put(np.concatenate([prev, np.full(8, SENT, F32)]))
        assert dev.lib.mtts_sum_tasks(tasks, P(dg), g_ts, scale, P(out), n4, accumulate, mb, None) == 0
        got = dev.get(out)
        assert np.all(got[n:] == SENT)
        terms = np.stack([scale * x.astype(np.float64) for x in gr] + ([prev.astype(np.float64)] if accumulate else []))
        ref = terms.sum(0)
        assert_within(got[:n], ref, sum_bound(tasks + 2, np.abs(terms).sum(0), ref), "sum_tasks")    # tasks terms, the scale, the accumulate
    dst = dev.put(np.full(tasks * d_ts, SENT, F32))
    assert dev.lib.mtts_broadcast(tasks, P(dev.put(w[0])), P(dst), d_ts, n4, mb, None) == 0
    got, rest = unpack(dev.get(dst), d_ts, [(n,)] * tasks)
    assert np.all(rest == SENT)
    for t in range(tasks):
        np.testing.assert_array_equal(got[t], w[0])


def test_bad_arguments_are_rejected(dev):
    lib, P = dev.lib, dev.ptr
    data = loss_case(1, 32, 0, 0)
    b = LossBufs(dev, data, 32, 0, 0)
    out = dev.empty(4096, fill=SENT)
    o = P(out)
    loss = lambda tasks=1, c=b.counts, n_mel=32, ptr=b.ptr, ts=b.ts_arr, L=o, ws=P(b.ws): lib.mtts_rows_loss(tasks, *c, n_mel, 0, 0, ptr, ts, L, ws, None)
    grad = lambda tasks=1, c=b.counts, n_mel=32, ptr=b.ptr, ts=b.ts_arr, L=o, ws=P(b.ws): lib.mtts_rows_loss_grad(tasks, *c, n_mel, 0, 0, ptr, ts, 1.0, L, o, o, o, o,
                                                                                                                  None, None, ws, None)
    nullp = (C.c_void_p * 15)(*[None if i == 6 else dev.ptr(x).value for i, x in enumerate(b.inputs)])
    for f in (loss, grad):
        assert f(tasks=0) != 0 and f(tasks=9) != 0                    # tasks outside 1 .. 8
        assert f(n_mel=30) != 0 and f(n_mel=1028) != 0                # n_mel % 4, n_mel > 1024
        assert f(ptr=None) != 0 and f(ptr=nullp) != 0 and f(L=None) != 0 and f(ws=None) != 0 and f(ts=None) != 0   # null pointers
        assert f(c=(b.counts[0], b.counts[1], i32([0]), b.counts[3])) != 0 and f(c=(b.counts[0], b.counts[1], i32([902]), b.counts[3])) != 0   # nF outside 1 .. Mr
        assert f(c=(None,) + b.counts[1:]) != 0
    # a frame-level feature needs its frame-level arrays and gradient buffers
    nofr = (C.c_void_p * 15)(*[None if i >= 11 else dev.ptr(x).value for i, x in enumerate(b.inputs)])
    assert lib.mtts_rows_loss(1, *b.counts, 32, 1, 0, nofr, b.ts_arr, o, P(b.ws), None) != 0
    assert lib.mtts_rows_loss_grad(1, *b.counts, 32, 0, 1, b.ptr, b.ts_arr, 1.0, o, o, o, o, o, None, None, P(b.ws), None) != 0
    g = P(dev.put(np.ones(64, F32)))
    assert lib.mtts_sumsq_norm(None, 4, 2, None, o, o, None) != 0 and lib.mtts_sumsq_norm(g, 0, 2, None, o, o, None) != 0
    assert lib.mtts_sumsq_norm(g, 4, 0, None, o, o, None) != 0 and lib.mtts_sumsq_norm(g, 4, 4097, None, o, o, None) != 0
    assert lib.mtts_sumsq_norm(g, 4, 2, None, None, o, None) != 0 and lib.mtts_sumsq_norm(g, 4, 2, None, o, None, None) != 0
    adam = lambda w=o, gg=g, n4=4, norm=g, step=1, mb=2: lib.mtts_adam_clip(w, gg, o, o, n4, norm, 1.0, 1e-3, 0.9, 0.98, 1e-9, step, 0.0, mb, None)
    assert adam(w=None) != 0 and adam(gg=None) != 0 and adam(norm=None) != 0 and adam(n4=0) != 0 and adam(step=0) != 0 and adam(mb=0) != 0
    for tasks in (0, 9):
        assert lib.mtts_sgd_update(tasks, o, 64, g, 0, 4, 0.1, 2, None) != 0
        assert lib.mtts_sum_tasks(tasks, g, 0, 1.0, o, 4, 0, 2, None) != 0
        assert lib.mtts_broadcast(tasks, g, o, 64, 4, 2, None) != 0
    assert lib.mtts_sgd_update(1, None, 64, g, 0, 4, 0.1, 2, None) != 0 and lib.mtts_sgd_update(1, o, -4, g, 0, 4, 0.1, 2, None) != 0
    assert lib.mtts_sgd_update(1, o, 64, g, 0, 4, 0.1, 0, None) != 0
    assert lib.mtts_sum_tasks(1, None, 0, 1.0, o, 4, 0, 2, None) != 0 and lib.mtts_sum_tasks(1, g, 0, 1.0, None, 4, 0, 2, None) != 0
    assert lib.mtts_sum_tasks(1, g, 0, 1.0, o, 0, 0, 2, None) != 0
    assert lib.mtts_broadcast(1, None, o, 64, 4, 2, None) != 0 and lib.mtts_broadcast(1, g, None, 64, 4, 2, None) != 0 and lib.mtts_broadcast(1, g, o, -1, 4, 2, None) != 0
    assert np.all(dev.get(out) == SENT)                                # a refusal launches nothing
