"""TEST INFRASTRUCTURE ONLY — the GE2E loss as include/mtts.h defines it (softmax variant of Wan et al. 2018; parity with any published
GE2E code is UNPINNED), restated in torch with a `dtype` argument: float64 is the reference, float32 the same formulas at the kernels'
precision, whose distance to the float64 result is what test_ge2e.py derives its bounds from.  Every gradient is autograd's, never a
restated formula.  Also the chain (LSTM -> linear -> ReLU -> normalise -> utterance normalise -> loss) on the modules of
oracle/dvector_oracle.py, the trainer rule (scale, joint clip, Adam) and a host trainer that applies it step after step."""
import numpy as np
import torch

from oracle import dvector_oracle as orc


def similarities(e, w, b, detach=()):
    """e [N][M][E] -> s [N M][N].  detach: names of the paths a gradient may NOT take — "c": through the inclusive centroids (path b),
    "x": through the exclusive centroids (path c), "a": the row's own embedding (path a)."""
    N, M, _ = e.shape
    S = e.sum(dim=1)
    c = S / S.norm(dim=1, keepdim=True)
    u = (S[:, None, :] - e) / (M - 1)
    x = u / u.norm(dim=2, keepdim=True)
    if "c" in detach:
        c = c.detach()
    if "x" in detach:
        x = x.detach()
    own = e.detach() if "a" in detach else e
    d = torch.einsum("jie,ke->jik", own, c)
    d_own = (own * x).sum(dim=2)
    eye = torch.eye(N, dtype=torch.bool)[:, None, :].expand(N, M, N)
    d = torch.where(eye, d_own[:, :, None].expand(N, M, N), d)
    return (w * d + b).reshape(N * M, N), d.reshape(N * M, N)


def row_losses(s, N, M):
    target = torch.arange(N).repeat_interleave(M)
    return torch.logsumexp(s, dim=1) - s[torch.arange(N * M), target]


def loss(emb, N, M, w, b, dtype=torch.float64, row_weight=None, detach=()):
    """emb [N M][E] float32 -> dict(L, dw, db, sim, demb) as numpy float64.  row_weight [N M]: the loss is sum(row_weight * row loss) / (N M)
    (None: all ones — the definition)."""
    e = torch.tensor(np.asarray(emb, np.float32), dtype=dtype, requires_grad=True)
    wt = torch.tensor(float(np.float32(w)), dtype=dtype, requires_grad=True)
    bt = torch.tensor(float(np.float32(b)), dtype=dtype, requires_grad=True)
    s, _ = similarities(e.reshape(N, M, -1), wt, bt, detach)
    rows = row_losses(s, N, M)
    if row_weight is not None:
        rows = rows * torch.tensor(np.asarray(row_weight), dtype=dtype)
    L = rows.sum() / (N * M)
    L.backward()
    f = lambda t: t.detach().to(torch.float64).numpy()
    return dict(L=f(L), dw=f(wt.grad), db=f(bt.grad), sim=f(s), demb=f(e.grad))


def embed(lstm, linear, mels):
    """The encoder's training forward with one partial per utterance: F.normalize(relu(linear(h_T)) / |.|)."""
    _, (hidden, _) = lstm(mels)
    raw = torch.relu(linear(hidden[-1]))
    pe = raw / torch.norm(raw, dim=1, keepdim=True)
    return torch.nn.functional.normalize(pe, dim=1)


def named(lstm, linear):
    return [(f"lstm.{n}", p) for n, p in lstm.named_parameters()] + [(f"linear.{n}", p) for n, p in linear.named_parameters()]


def chain(sd, cfg, mels, N, M, w, b, dtype=torch.float64):
    """-> dict(L, sim, emb, dw, db, grads {tensor name: gradient}) of the whole chain, numpy float64."""
    lstm, linear = orc.build(sd, dtype=dtype, **cfg)
    wt = torch.tensor(float(np.float32(w)), dtype=dtype, requires_grad=True)
    bt = torch.tensor(float(np.float32(b)), dtype=dtype, requires_grad=True)
    e = embed(lstm, linear, torch.tensor(np.asarray(mels, np.float32), dtype=dtype))
    s, _ = similarities(e.reshape(N, M, -1), wt, bt)
    L = row_losses(s, N, M).sum() / (N * M)
    L.backward()
    f = lambda t: t.detach().to(torch.float64).numpy()
    return dict(L=f(L), sim=f(s), emb=f(e), dw=f(wt.grad), db=f(bt.grad), grads={n: f(p.grad) for n, p in named(lstm, linear)})


def trainer_step(params, grads, m, v, step, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, max_norm=3.0, scalar_grad_scale=0.01, dtype=np.float64):
    """One step of rule 6 of include/mtts.h on dicts of arrays that include "w" and "b" (arrays of one element): the gradients of w and b
    x scalar_grad_scale, the joint L2 norm of all gradients clipped to max_norm (coefficient min(1, max_norm / (norm + 1e-6))), Adam with
    bias correction (denominator sqrt(v / (1 - b2^step)) + eps), no weight decay.  -> (params, m, v, norm before clipping), new dicts."""
    g = {k: np.asarray(a, dtype) * (dtype(scalar_grad_scale) if k in ("w", "b") else dtype(1)) for k, a in grads.items()}
    norm = dtype(np.sqrt(sum(float((a.astype(np.float64) ** 2).sum()) for a in g.values())))
    coef = min(dtype(1), dtype(max_norm) / (norm + dtype(1e-6)))
    b1, b2 = dtype(betas[0]), dtype(betas[1])
    bc1, bc2 = dtype(1) - b1 ** step, dtype(1) - b2 ** step
    P, Mo, Vo = {}, {}, {}
    for k in params:
        gg = g[k] * coef
        Mo[k] = b1 * np.asarray(m[k], dtype) + (dtype(1) - b1) * gg
        Vo[k] = b2 * np.asarray(v[k], dtype) + (dtype(1) - b2) * gg * gg
        P[k] = np.asarray(params[k], dtype) - (dtype(lr) / bc1) * Mo[k] / (np.sqrt(Vo[k]) / np.sqrt(bc2) + dtype(eps))
    return P, Mo, Vo, float(norm)


class Trainer:
    """The same training, step after step, in torch on the host (`dtype`): test_ge2e.py's precondition and tools/ge2e_bench.py's host leg."""

    def __init__(self, sd, cfg, N, M, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, max_norm=3.0, scalar_grad_scale=0.01, init_w=10.0, init_b=-5.0,
                 dtype=torch.float64):
        self.lstm, self.linear = orc.build(sd, dtype=dtype, **cfg)
        self.w = torch.tensor(float(init_w), dtype=dtype, requires_grad=True)
        self.b = torch.tensor(float(init_b), dtype=dtype, requires_grad=True)
        self.N, self.M, self.dtype, self.max_norm, self.scale = N, M, dtype, max_norm, scalar_grad_scale
        self.params = [p for _, p in named(self.lstm, self.linear)] + [self.w, self.b]
        self.opt = torch.optim.Adam(self.params, lr=lr, betas=betas, eps=eps)

    def train_step(self, mels):
        """-> (loss, similarity matrix [N M][N]) before the update."""
        self.opt.zero_grad()
        e = embed(self.lstm, self.linear, torch.as_tensor(np.asarray(mels, np.float32)).to(self.dtype))
        s, _ = similarities(e.reshape(self.N, self.M, -1), self.w, self.b)
        L = row_losses(s, self.N, self.M).sum() / (self.N * self.M)
        L.backward()
        self.w.grad *= self.scale
        self.b.grad *= self.scale
        torch.nn.utils.clip_grad_norm_(self.params, self.max_norm)
        self.opt.step()
        return float(L.detach()), s.detach().to(torch.float64).numpy()
