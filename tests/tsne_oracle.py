"""The definition of exact t-SNE that tests/test_tsne.py pins csrc/tsne.h to, in float64 numpy: sklearn 1.7's method="exact"
(_utils._binary_search_perplexity, _t_sne._joint_probabilities, _kl_divergence, _gradient_descent, TSNE._tsne) restated, plus a float32
twin of the gradient and the step in the kernel's summation order, and `trustworthiness` restated.  Dense [n][n] matrices throughout
(sklearn's are condensed); the diagonal is excluded everywhere."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)      # sklearn's MACHINE_EPSILON
TOL = float(np.float32(1e-5))              # `cdef float PERPLEXITY_TOLERANCE`
TINY = float(np.float32(1e-8))             # `cdef float EPSILON_DBL`
N_ITER_CHECK, EXPLORATION = 50, 250


def make_dvectors(n_spk, n_per, dim=256, seed=0, spread=0.5, adversarial=False):
    """L2-normalised non-negative clustered vectors, as d-vectors are (a ReLU and a normalisation end the encoder): non-negative unit
    centres plus noise of norm about `spread`.  adversarial: the last three rows become a copy of row 0 (distance 0), a far outlier
    (norm 28: every distance is above 745, so its row sum underflows to the 1e-8 rule at beta = 1) and zeros."""
    r = np.random.default_rng(seed)
    c = np.abs(r.standard_normal((n_spk, dim)))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    x = np.repeat(c, n_per, 0) + spread / np.sqrt(dim) * r.standard_normal((n_spk * n_per, dim))
    x = np.maximum(x, 0)
    x /= np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-12)
    x = x.astype(np.float32)
    if adversarial:
        x[-3] = x[0]
        x[-2] = 28.0 * np.abs(r.standard_normal(dim)) / np.sqrt(dim)
        x[-1] = 0
    return x, np.repeat(np.arange(n_spk), n_per)


def sqdist(X, dtype=np.float64):
    """Squared Euclidean distances in the direct form, computed in `dtype`, rounded to float32 as sklearn rounds them; returned as float64."""
    X = np.asarray(X).astype(dtype)
    D = np.zeros((len(X), len(X)), dtype)
    for k in range(X.shape[1]):
        d = X[:, None, k] - X[None, :, k]
        D += d * d
    return D.astype(np.float32).astype(np.float64)


def entropy_at(D, beta):
    """H_i of row i at beta_i (float64; j = i excluded; a row sum of 0 replaced by TINY): what the search drives to log(perplexity)."""
    n = len(D)
    off = ~np.eye(n, dtype=bool)
    Pm = np.exp(-D * beta[:, None]) * off
    S = Pm.sum(1)
    S[S == 0] = TINY
    return np.log(S) + beta * (D * (Pm / S[:, None])).sum(1), Pm / S[:, None]


def search(D, perplexity):
    """_binary_search_perplexity on a square matrix -> (conditional rows, the beta each row was evaluated at)."""
    n = len(D)
    lp = np.log(perplexity)
    beta, lo, hi = np.ones(n), np.full(n, -np.inf), np.full(n, np.inf)
    active = np.ones(n, bool)
    C, beta_at = np.zeros((n, n)), np.ones(n)
    for _ in range(100):
        if not active.any():
            break
        H, Pn = entropy_at(D, beta)
        C[active], beta_at[active] = Pn[active], beta[active]
        diff = H - lp
        active &= ~(np.abs(diff) <= TOL)
        up, dn = active & (diff > 0), active & ~(diff > 0)
        lo[up] = beta[up]
        beta[up] = np.where(np.isinf(hi[up]), beta[up] * 2, (beta[up] + hi[up]) / 2)
        hi[dn] = beta[dn]
        beta[dn] = np.where(np.isinf(lo[dn]), beta[dn] / 2, (beta[dn] + lo[dn]) / 2)
    return C, beta_at, ~active


def joint(C, store=np.float64):
    """_joint_probabilities' last three lines; store=np.float32: the conditional rows and P held as float32, as the device holds them."""
    C = C.astype(store).astype(np.float64)
    P = C + C.T
    P = np.maximum(P / max(P.sum(), EPS), EPS)
    np.fill_diagonal(P, 0)
    return P.astype(store).astype(np.float64)


def affinities(X, perplexity):
    D = sqdist(X)
    C, beta, _ = search(D, perplexity)
    return joint(C), beta, D


def kl_grad(Y, P, exaggeration=1.0):
    """_kl_divergence at degrees_of_freedom 1 on exaggeration x P -> (KL, gradient [n][2]) in float64."""
    Y = np.asarray(Y, np.float64)
    P = np.asarray(P, np.float64) * exaggeration
    d = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1)
    num = 1.0 / (1.0 + d)
    np.fill_diagonal(num, 0)
    Q = np.maximum(num / num.sum(), EPS)
    PQ = (P - Q) * num
    np.fill_diagonal(PQ, 0)
    grad = 4.0 * (PQ.sum(1, keepdims=True) * Y - PQ @ Y)
    m = ~np.eye(len(Y), dtype=bool)
    return float((P[m] * np.log(np.maximum(P[m], EPS) / Q[m])).sum()), grad


def step(Y, update, gains, grad, momentum, learning_rate, min_gain=0.01):
    """_gradient_descent lines 402-409 in the arrays' dtype -> (Y, update, gains, grad x gains)."""
    dt = Y.dtype.type
    inc = update * grad < 0
    gains = np.where(inc, gains + dt(0.2), gains * dt(0.8))
    gains = np.maximum(gains, dt(min_gain))
    gg = grad * gains
    update = dt(momentum) * update - dt(learning_rate) * gg
    return Y + update, update, gains, gg


def run(Y, update, gains, P, n_iter, exaggeration, momentum, learning_rate, min_gain=0.01, grad_fn=None):
    grad_fn = grad_fn or (lambda y: kl_grad(y, P, exaggeration)[1])
    for _ in range(n_iter):
        Y, update, gains, _ = step(Y, update, gains, grad_fn(Y).astype(Y.dtype), momentum, learning_rate, min_gain)
    return Y, update, gains


def descend(Y0, P, max_iter, learning_rate, early_exaggeration=12.0, stop_at=None):
    """TSNE._tsne without the early stops (no test input triggers one): EXPLORATION iterations at momentum 0.5 on early_exaggeration x P,
    the rest at momentum 0.8, update and gains starting afresh in each phase as _gradient_descent does.  stop_at: states to keep."""
    Y = np.asarray(Y0, np.float64).copy()
    kept = {}
    it = 0
    for upto, ex, mom in ((min(EXPLORATION, max_iter), early_exaggeration, 0.5), (max_iter, 1.0, 0.8)):
        u, g = np.zeros_like(Y), np.ones_like(Y)
        while it < upto:
            Y, u, g, _ = step(Y, u, g, kl_grad(Y, P, ex)[1], mom, learning_rate)
            it += 1
            if stop_at and it in stop_at:
                kept[it] = Y.copy()
    return (Y, kept) if stop_at else Y


# ---- the float32 twin: the kernel's arithmetic and summation order -------------------------------------------------------------------
def _seq(t):
    """Sum over axis 0 in order, in t's dtype."""
    acc = t[0].copy()
    for k in range(1, len(t)):
        acc = acc + t[k]
    return acc


def _fold(v):
    """tsne_block_fold: 256 threads add ceil(n / 256) consecutive values each, then the 256 partial sums in order (float64)."""
    v = np.asarray(v, np.float64)
    per = -(-len(v) // 256)
    part = _seq(np.pad(v, (0, 256 * per - len(v))).reshape(256, per).T)
    return float(np.cumsum(part)[-1])


def pair_sums32(Y, P, fma=False):
    """tsne_pair_kernel: per row (attractive [n][2], repulsive [n][2], share of Z [n], smallest num [n]) in float32; lane = j mod 64 adds in
    ascending j, then 4 groups of 16 lanes, then the 4 group sums.  fma: with the contractions a compiler may apply (a*b+c rounded once)."""
    f32, f64 = np.float32, np.float64
    Y, P = np.asarray(Y, f32), np.asarray(P, f32)
    n = len(Y)
    L = -(-n // 64)
    dx, dy = Y[:, None, 0] - Y[None, :, 0], Y[:, None, 1] - Y[None, :, 1]
    d2 = (dx.astype(f64) * dx + (dy * dy)).astype(f32) if fma else dx * dx + dy * dy
    num = f32(1) / (f32(1) + d2)
    w, q = P * num, num * num
    other = ~np.eye(n, dtype=bool)

    def lanes(a):   # [n][n] -> [L][n][64]
        return np.pad(a, ((0, 0), (0, 64 * L - n))).reshape(n, L, 64).transpose(1, 0, 2)

    def tree(acc):  # [n][64] -> [n]
        g = _seq(acc.reshape(n, 4, 16).transpose(2, 0, 1))
        return _seq(g.T)

    def dot(a, b):
        a, b = lanes(a), lanes(b)
        acc = np.zeros((n, 64), f32)
        for k in range(L):
            acc = (acc.astype(f64) + a[k].astype(f64) * b[k]).astype(f32) if fma else acc + a[k] * b[k]
        return tree(acc)

    attr = np.stack([dot(w, dx), dot(w, dy)], 1)
    rep = np.stack([dot(q, dx), dot(q, dy)], 1)
    z = tree(_seq(lanes(np.where(other, num, f32(0)))))
    return attr, rep, z, np.where(other, num, f32(1)).min(1)


def kl_grad32(Y, P, exaggeration=1.0, fma=False):
    """The device's gradient (float32) and KL (float64 on the twin's Z) at Y; Q's floor in the gradient as tsne_grad_kernel applies it."""
    Y32, P32 = np.asarray(Y, np.float32), np.asarray(P, np.float32)
    attr, rep, z, nmin = pair_sums32(Y32, P32, fma)
    Z = _fold(z)
    qsum = rep.astype(np.float64) / Z
    for i in np.flatnonzero(nmin.astype(np.float64) < EPS * Z):
        d = Y32[i] - Y32
        num = np.float32(1) / (np.float32(1) + (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]))
        q = np.maximum(num.astype(np.float64) / Z, EPS) * num
        q[i] = 0
        qsum[i] = np.cumsum(q[:, None] * d, 0)[-1]
    grad = (4.0 * (exaggeration * attr.astype(np.float64) - qsum)).astype(np.float32)
    Y64 = Y32.astype(np.float64)
    Pe = P32.astype(np.float64) * exaggeration
    d = ((Y64[:, None, :] - Y64[None, :, :]) ** 2).sum(-1)
    Q = np.maximum(1.0 / (1.0 + d) / Z, EPS)
    m = ~np.eye(len(Y32), dtype=bool)
    return float((Pe[m] * np.log(np.maximum(Pe[m], EPS) / Q[m])).sum()), grad


# ---- quality measures -------------------------------------------------------------------------------------------------------------------
def trustworthiness(X, Y, n_neighbors=5):
    """sklearn.manifold.trustworthiness (Euclidean) restated."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    n = len(X)
    dX = np.sqrt(np.maximum(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1), 0))
    dY = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(dX, np.inf)
    np.fill_diagonal(dY, np.inf)
    ind_X = np.argsort(dX, axis=1)
    ind_Y = np.argsort(dY, axis=1, kind="stable")[:, :n_neighbors]
    rank = np.zeros((n, n), int)
    rank[np.arange(n)[:, None], ind_X] = np.arange(1, n + 1)
    r = rank[np.arange(n)[:, None], ind_Y] - n_neighbors
    t = float(np.sum(r[r > 0]))
    return 1.0 - t * (2.0 / (n * n_neighbors * (2.0 * n - 3.0 * n_neighbors - 1.0)))


def same_speaker_1nn(Y, labels):
    Y = np.asarray(Y, np.float64)
    d = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    return float((labels[d.argmin(1)] == labels).mean())
