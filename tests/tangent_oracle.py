"""Reference for the second-order (tangent) row kernels of csrc/tangent.h and ColArgs modes 5 / 6 of csrc/rowops.h: every operation
written in elementary torch ops on the CPU, and the tangent of its backward taken by autograd (forward over reverse),

    grad = lambda *primals, dy: torch.func.vjp(f, *primals)[1](dy)
    (out, tout) = torch.func.jvp(grad, (primals..., dy), (tangents..., tgy))

never from the closed forms the kernels implement.  Every function takes numpy float32 arrays and a torch dtype: float64 is the reference,
float32 the same restatement at the kernels' precision — the distance between the two is the restatement's own rounding on these inputs,
which is what the tests (test_tangent_entries.py) derive their bounds from.  Returns dicts of numpy float64 arrays."""
import numpy as np
import torch

EPS = 1e-5


def _t(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def _np(d):
    return {k: v.detach().to(torch.float64).numpy() for k, v in d.items()}


def _zeros_like_or(t, like):
    return torch.zeros_like(like) if t is None else t


def jvp_over_vjp(f, primals, tangents, dy, tgy):
    """(cotangents of f at dy, their tangents in direction (tangents, tgy))"""
    def grad(*args):
        return torch.func.vjp(f, *args[:-1])[1](args[-1])
    return torch.func.jvp(grad, (*primals, dy), (*tangents, tgy))


def _xhat_rows(x):
    mean = x.mean(dim=1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=1, keepdim=True)
    return (x - mean) / torch.sqrt(var + EPS)


def layernorm(z, tz, gamma, beta, tgamma, tbeta, mask, dy, tgy, relu_on_z, dtype=torch.float64):
    """f(x, gamma, beta) = mask * (gamma * xhat + beta) over the channels of every row, eps 1e-5.  tgamma / tbeta / mask None: 0 / 0 / all
    rows.  relu_on_z: dz and tgz times [z > 0] (the LayerNorm input is a ReLU output whose backward rides in the kernel)."""
    z, tz, gamma, beta, dy, tgy = (_t(a, dtype) for a in (z, tz, gamma, beta, dy, tgy))
    tgamma, tbeta = _zeros_like_or(_t(tgamma, dtype), gamma), _zeros_like_or(_t(tbeta, dtype), beta)
    m = torch.ones(z.shape[0], 1, dtype=dtype) if mask is None else _t(mask.astype(np.float32), dtype)[:, None]
    f = lambda x, g, b: m * (g * _xhat_rows(x) + b)
    y, ty = torch.func.jvp(f, (z, gamma, beta), (tz, tgamma, tbeta))
    (dz, dgamma, dbeta), (tgz, hgamma, hbeta) = jvp_over_vjp(f, (z, gamma, beta), (tz, tgamma, tbeta), dy, tgy)
    if relu_on_z:
        pos = (z > 0).to(dtype)
        dz, tgz = dz * pos, tgz * pos
    tstats = torch.stack([tz.mean(dim=1), (_xhat_rows(z) * tz).mean(dim=1)], dim=1)   # what the kernels hand from forward to backward
    return _np(dict(y=y, ty=ty, tstats=tstats, dz=dz, tgz=tgz, dgamma=dgamma, dbeta=dbeta, hgamma=hgamma, hbeta=hbeta))


def softmax(S, tS, dP, tgP, alpha, dtype=torch.float64):
    """f(S) = softmax(alpha * S) over the last axis; direction (tS, tgP).  P / tP are f and its jvp (what the kernel is handed)."""
    S, tS, dP, tgP = (_t(a, dtype) for a in (S, tS, dP, tgP))
    f = lambda s: torch.softmax(alpha * s, dim=-1)
    P, tP = torch.func.jvp(f, (S,), (tS,))
    (dS,), (tgS,) = jvp_over_vjp(f, (S,), (tS,), dP, tgP)
    return _np(dict(P=P, tP=tP, dS=dS, tgS=tgS))


def batchnorm(x, tx, gamma, beta, tgamma, tbeta, dy, tgy, do_tanh, dtype=torch.float64):
    """f(x, gamma, beta) = [tanh](gamma * xhat + beta), statistics over the rows of x (the caller passes the in-rectangle rows only),
    biased variance, eps 1e-5.  tsum = [sum tx * xhat | sum tx] per channel."""
    x, tx, gamma, beta, dy, tgy = (_t(a, dtype) for a in (x, tx, gamma, beta, dy, tgy))
    tgamma, tbeta = _zeros_like_or(_t(tgamma, dtype), gamma), _zeros_like_or(_t(tbeta, dtype), beta)

    def xhat_cols(v):
        mean = v.mean(dim=0, keepdim=True)
        var = ((v - mean) ** 2).mean(dim=0, keepdim=True)
        return (v - mean) / torch.sqrt(var + EPS)

    def f(v, g, b):
        o = g * xhat_cols(v) + b
        return torch.tanh(o) if do_tanh else o
    y, ta = torch.func.jvp(f, (x, gamma, beta), (tx, tgamma, tbeta))
    (dx, dgamma, dbeta), (tdx, hgamma, hbeta) = jvp_over_vjp(f, (x, gamma, beta), (tx, tgamma, tbeta), dy, tgy)
    tsum = torch.cat([(tx * xhat_cols(x)).sum(dim=0), tx.sum(dim=0)])
    return _np(dict(y=y, ta=ta, tsum=tsum, dx=dx, tdx=tdx, dgamma=dgamma, dbeta=dbeta, hgamma=hgamma, hbeta=hbeta))


def rowdot(x, tx, w, tw, tb, valid, dout, tgout, dtype=torch.float64):
    """f(x, w, b) = valid * (x @ w + b), b a scalar.  tw / tb None: 0."""
    x, tx, w, dout, tgout = (_t(a, dtype) for a in (x, tx, w, dout, tgout))
    tw = _zeros_like_or(_t(tw, dtype), w)
    b = torch.zeros((), dtype=dtype)   # (the bias enters neither the tangent of the output nor any gradient but its own)
    tb = torch.zeros((), dtype=dtype) if tb is None else torch.tensor(float(np.asarray(tb).reshape(-1)[0]), dtype=dtype)
    v = _t(valid.astype(np.float32), dtype)
    f = lambda a, ww, bb: v * (a @ ww + bb)
    _, tout = torch.func.jvp(f, (x, w, b), (tx, tw, tb))
    (dx, _, _), (tdx, _, _) = jvp_over_vjp(f, (x, w, b), (tx, tw, tb), dout, tgout)
    return _np(dict(tout=tout, dx=dx, tdx=tdx))
