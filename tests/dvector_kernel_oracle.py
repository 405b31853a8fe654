"""TEST INFRASTRUCTURE ONLY — torch restatements of the six numerical kernels of meta_tts_amd/csrc/dvector.h, one function per
forward / backward pair, with a `dtype` argument (float64: the reference; float32: the same formulas at the kernels' precision, whose
distance to the float64 result is what test_dvector_kernels.py derives its bounds from).

Written from the formulas in the comments of dvector.h and torch's documented LSTM equations (nn.LSTM, gate order i, f, g, o):
    i = sigmoid(xp_i + W_hi h)   f = sigmoid(xp_f + W_hf h)   g = tanh(xp_g + W_hg h)   o = sigmoid(xp_o + W_ho h)
    c' = f c + i g               h' = o tanh(c')
with xp the input projection (both biases included).  Every backward is autograd's, never a restated formula."""
import numpy as np
import torch


def _t(a, dtype, grad=False):
    return torch.tensor(np.asarray(a), dtype=dtype, requires_grad=grad)


def _np(t):
    return None if t is None else t.detach().numpy()


def lstm_layer(xp, whh, dh_ext=None, dh_last=None, dtype=torch.float64):
    """One LSTM layer as a cell loop from zero state.  xp [N][T][4H], whh [4H][H] (torch's weight_hh layout).  Returns every array the
    kernel stores: gates [N][T][4H] AFTER the non-linearities, cseq / hprev / hseq [N][T][H], hlast [N][H]; and dgates [N][T][4H] =
    d loss / d xp for loss = sum(hseq * dh_ext) + sum(hlast * dh_last) (xp enters the pre-activations additively, so this IS the gradient
    of the gate pre-activations); None when neither upstream gradient is given."""
    x = _t(xp, dtype, grad=True)
    w = _t(whh, dtype)
    N, T, H4 = x.shape
    H = H4 // 4
    h, c = torch.zeros(N, H, dtype=dtype), torch.zeros(N, H, dtype=dtype)
    gates, cseq, hprev, hseq = [], [], [], []
    for t in range(T):
        pre = x[:, t] + h @ w.T
        i, f, g, o = torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H]), torch.tanh(pre[:, 2 * H:3 * H]), torch.sigmoid(pre[:, 3 * H:])
        hprev.append(h)
        c = f * c + i * g
        h = o * torch.tanh(c)
        gates.append(torch.cat([i, f, g, o], dim=1))
        cseq.append(c)
        hseq.append(h)
    out = dict(gates=torch.stack(gates, 1), cseq=torch.stack(cseq, 1), hprev=torch.stack(hprev, 1), hseq=torch.stack(hseq, 1), hlast=h)
    dgates = None
    if dh_ext is not None or dh_last is not None:
        loss = 0
        if dh_ext is not None:
            loss = loss + (out["hseq"] * _t(dh_ext, dtype)).sum()
        if dh_last is not None:
            loss = loss + (out["hlast"] * _t(dh_last, dtype)).sum()
        dgates, = torch.autograd.grad(loss, x)
    res = {k: _np(v) for k, v in out.items()}
    res["dgates"] = _np(dgates)
    return res


def head(hlast, w, bias, dpart, dtype=torch.float64):
    """raw = relu(hlast W^T + bias), part = raw / ||raw|| (a row of zeros divides 0 by 0: NaN, as the encoder's forward does); dz = gradient
    of the Linear output and dh_last = gradient of hlast for loss = sum(part * dpart).  hlast [N][H], w [E][H], bias [E], dpart [N][E]."""
    h = _t(hlast, dtype, grad=True)
    z = h @ _t(w, dtype).T + _t(bias, dtype)
    z.retain_grad()
    raw = torch.relu(z)
    part = raw / torch.norm(raw, dim=1, keepdim=True)
    (part * _t(dpart, dtype)).sum().backward()
    return dict(z=_np(z), eraw=_np(raw), part=_np(part), dz=_np(z.grad), dh_last=_np(h.grad))


def utterance(part, off, dout, dtype=torch.float64):
    """out[b] = F.normalize(mean(part[off[b]:off[b+1]]), eps=1e-12); dpart = gradient of part for loss = sum(out * dout)."""
    p = _t(part, dtype, grad=True)
    out = torch.stack([torch.nn.functional.normalize(p[int(off[b]):int(off[b + 1])].mean(dim=0), dim=0, eps=1e-12) for b in range(len(off) - 1)])
    (out * _t(dout, dtype)).sum().backward()
    return dict(out=_np(out), dpart=_np(p.grad))
