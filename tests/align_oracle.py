"""The definition of the flat-start monophone aligner that tests/test_align.py pins csrc/align.h to (include/mtts.h states it), in float64
numpy and in the same order of operations: emission in ascending f with the reciprocal variance rounded once, logsumexp as
m + log(sum exp(. - m)) over stay, advance, skip, per-state statistics in ascending t, one utterance's per-class sum after another's."""
import numpy as np

NINF = -np.inf
TWO_PI = 6.283185307179586


class Model:
    def __init__(self, mean, var, gvar):
        self.mean, self.var, self.gvar = (np.array(a, np.float64) for a in (mean, var, gvar))

    def copy(self):
        return Model(self.mean, self.var, self.gvar)


def class_scores(x, model):
    """[T][V]: -1/2 sum_f [(x - mu)^2 (1 / var) + log(2 pi var)], the bracket added in ascending f."""
    x = np.asarray(x, np.float32).astype(np.float64)
    iv, lc = 1.0 / model.var, np.log(TWO_PI * model.var)
    acc = np.zeros((x.shape[0], model.mean.shape[0]))
    for f in range(x.shape[1]):
        d = x[:, f, None] - model.mean[None, :, f]
        acc += d * d * iv[None, :, f] + lc[None, :, f]
    return -0.5 * acc


def emission(x, model, cls):
    return class_scores(x, model)[:, np.asarray(cls)]


def emission_scale(x, model, cls):
    """max over cells of sum_f (|(x - mu)^2 / var| + |log(2 pi var)|): what the rounding error of an emission is relative to."""
    x = np.asarray(x, np.float32).astype(np.float64)
    d = x[:, None, :] - model.mean[None]
    return float(((d * d / model.var[None]).sum(-1) + np.abs(np.log(TWO_PI * model.var)).sum(-1)[None])[:, np.asarray(cls)].max())


def lse3(a, b, c):
    m = np.maximum(np.maximum(a, b), c)
    safe = np.where(m == NINF, 0.0, m)
    with np.errstate(divide="ignore"):
        return np.where(m == NINF, NINF, m + np.log(np.exp(a - safe) + np.exp(b - safe) + np.exp(c - safe)))


def _shift(row, k, allowed=None):
    """row[s - k] at s (k > 0) or row[s + |k|] (k < 0), -inf where there is none or where `allowed` is false."""
    out = np.full_like(row, NINF)
    if k > 0:
        out[k:] = row[:-k] if k < len(row) else []
    else:
        out[:k] = row[-k:] if -k < len(row) else []
    return out if allowed is None else np.where(allowed, out, NINF)


def _skip_into(opt):
    """skip_into[s]: state s - 1 exists, has a predecessor s - 2 and is optional."""
    opt = np.asarray(opt, bool)
    a = np.zeros(len(opt), bool)
    a[2:] = opt[1:-1]
    return a


def _skip_from(opt):
    opt = np.asarray(opt, bool)
    a = np.zeros(len(opt), bool)
    a[:-2] = opt[1:-1]
    return a


def forward(b, opt):
    """-> (alpha [T][S], LL)."""
    T, S = b.shape
    opt = np.asarray(opt, bool)
    alpha = np.full((T, S), NINF)
    alpha[0, 0] = b[0, 0]
    if S > 1 and opt[0]:
        alpha[0, 1] = b[0, 1]
    skip = _skip_into(opt)
    for t in range(1, T):
        p = alpha[t - 1]
        alpha[t] = b[t] + lse3(p, _shift(p, 1), _shift(p, 2, skip))
    before = alpha[T - 1, S - 2] if S > 1 and opt[S - 1] else NINF
    return alpha, float(lse3(alpha[T - 1, S - 1], before, NINF))


def backward(b, opt):
    T, S = b.shape
    opt = np.asarray(opt, bool)
    beta = np.full((T, S), NINF)
    beta[T - 1, S - 1] = 0.0
    if S > 1 and opt[S - 1]:
        beta[T - 1, S - 2] = 0.0
    skip = _skip_from(opt)
    for t in range(T - 2, -1, -1):
        e = b[t + 1] + beta[t + 1]
        beta[t] = lse3(e, _shift(e, -1), _shift(e, -2, skip))
    return beta


def posteriors(x, model, cls, opt):
    """-> (LL, gamma [T][S])."""
    b = emission(x, model, cls)
    alpha, LL = forward(b, opt)
    return LL, np.exp((alpha + backward(b, opt)) - LL)


def viterbi(b, opt, ignore_exact_ties=False):
    """-> (durations [S] int32, score, margin): margin = the smallest gap between the best and the second-best finite candidate of any
    decision on the chosen path (the end state included), relative to |score|; inf when no decision had two candidates.
    ignore_exact_ties: gaps of exactly 0 are left out — two adjacent states of one class make paths whose scores are the same additions
    of the same numbers, a tie in every arithmetic, which the tie rule decides and rounding cannot."""
    T, S = b.shape
    opt = np.asarray(opt, bool)
    delta = np.full((T, S), NINF)
    frm = np.zeros((T, S), np.uint8)
    delta[0, 0] = b[0, 0]
    if S > 1 and opt[0]:
        delta[0, 1] = b[0, 1]
    skip = _skip_into(opt)
    cands = np.full((T, 3, S), NINF)
    for t in range(1, T):
        p = delta[t - 1]
        c = np.stack([p, _shift(p, 1), _shift(p, 2, skip)])
        cands[t] = c
        best, f = c[0].copy(), np.zeros(S, np.uint8)
        for k in (1, 2):                      # ties to the first: strictly greater only
            better = c[k] > best
            best, f = np.where(better, c[k], best), np.where(better, k, f).astype(np.uint8)
        delta[t], frm[t] = b[t] + best, f
    last, before = delta[T - 1, S - 1], (delta[T - 1, S - 2] if S > 1 and opt[S - 1] else NINF)
    s, score = (S - 2, before) if before > last else (S - 1, last)
    gaps = [abs(last - before)] if np.isfinite(before) and np.isfinite(last) else []
    dur = np.zeros(S, np.int32)
    for t in range(T - 1, 0, -1):
        dur[s] += 1
        c = np.sort(cands[t, :, s][np.isfinite(cands[t, :, s])])
        if len(c) > 1:
            gaps.append(c[-1] - c[-2])
        s -= int(frm[t, s])
    dur[s] += 1
    if ignore_exact_ties:
        gaps = [g for g in gaps if g != 0.0]
    return dur, float(score), (min(gaps) / abs(score) if gaps else np.inf)


def align(x, model, cls, opt, ignore_exact_ties=False):
    return viterbi(emission(x, model, cls), opt, ignore_exact_ties)


def flat_start(xs, n_classes):
    """Every class = mean and variance of all frames: two passes, rows in order (cumsum adds one row after another)."""
    x = np.concatenate([np.asarray(a, np.float32) for a in xs]).astype(np.float64)
    mean = np.cumsum(x, axis=0)[-1] / len(x)
    d = x - mean
    g = np.cumsum(d * d, axis=0)[-1] / len(x)
    return Model(np.tile(mean, (n_classes, 1)), np.tile(g, (n_classes, 1)), g)


def state_stats(x, gamma):
    """[S][1 + 2 F]: occ, sum gamma x, sum gamma x^2 per state, ascending t."""
    x = np.asarray(x, np.float32).astype(np.float64)
    S, F = gamma.shape[1], x.shape[1]
    out = np.zeros((S, 1 + 2 * F))
    for t in range(len(x)):
        g = gamma[t][:, None]
        out[:, 0] += gamma[t]
        out[:, 1:1 + F] += g * x[t][None]
        out[:, 1 + F:] += g * (x[t] * x[t])[None]
    return out


def em_iteration(model, utts, var_floor=0.01, min_occ=1e-3):
    """utts: [(x, cls, opt)] -> (new model, total LL, [LL]).  Statistics: one utterance's per-class sum (its states of the class in
    ascending s, from zero) after another's."""
    V, F = model.mean.shape
    acc = np.zeros((V, 1 + 2 * F))
    lls = []
    for x, cls, opt in utts:
        LL, gamma = posteriors(x, model, cls, opt)
        lls.append(LL)
        part = state_stats(x, gamma)
        for v in sorted(set(int(c) for c in cls)):
            p = np.zeros(1 + 2 * F)
            for s in range(len(cls)):
                if cls[s] == v:
                    p = p + part[s]
            acc[v] += p
    new = model.copy()
    for v in range(V):
        occ = acc[v, 0]
        if not occ >= min_occ:
            continue
        m = acc[v, 1:1 + F] / occ
        s2 = acc[v, 1 + F:] / occ - m * m
        floor = var_floor * model.gvar
        new.mean[v], new.var[v] = m, np.where(s2 > floor, s2, floor)
    total = 0.0
    for v in lls:
        total += v
    return new, total, lls


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------
def random_model(V, F, seed):
    r = np.random.default_rng(seed)
    return Model(r.normal(0.0, 2.0, (V, F)), r.uniform(0.5, 2.0, (V, F)), r.uniform(0.5, 2.0, F))


def random_features(T, F, seed):
    return np.random.default_rng(seed).normal(0.0, 2.0, (T, F)).astype(np.float32)


def synthetic_corpus(seed, separation, n_utts=12, n_classes=6, n_feat=8, silence=0):
    """Frames drawn from known unit-variance Gaussians (class means `separation` sigma apart per coordinate draw) on known durations;
    class `silence` is optional wherever it stands (never twice in a row, never adjacent to itself).  -> (utts [(x, cls, opt)], true state
    of every frame per utterance, the generating means)."""
    r = np.random.default_rng(seed)
    means = r.normal(0.0, separation, (n_classes, n_feat))
    utts, truth = [], []
    for _ in range(n_utts):
        S = int(r.integers(3, 8))
        for _ in range(1000):
            T = int(r.integers(10, 41))
            cls = [int(r.integers(0, n_classes))]
            while len(cls) < S:
                c = int(r.integers(0, n_classes))
                if c != cls[-1]:
                    cls.append(c)
            opt = [c == silence for c in cls]
            cut = np.sort(r.choice(np.arange(1, T), S - 1, replace=False))
            dur = np.diff(np.concatenate([[0], cut, [T]]))
            if all(d >= 2 for d in dur):
                break
        state = np.repeat(np.arange(S), dur)
        x = (means[np.asarray(cls)[state]] + r.standard_normal((T, n_feat))).astype(np.float32)
        utts.append((x, np.asarray(cls, np.int32), np.asarray(opt, np.uint8)))
        truth.append(state)
    return utts, truth, means
