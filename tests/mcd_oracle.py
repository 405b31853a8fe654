"""The definition of mel-cepstral distortion along a DTW path that tests/test_mcd_dtw.py pins csrc/dtw.h to (include/mtts.h states it),
in float64 numpy and in the device's summation order: cepstra summed in ascending n, squared differences in ascending k, the F0 sums in
the order of the walk back from (Ta-1, Tb-1).  Written from the definition, not from the device code; the DP is vectorised along
anti-diagonals (the only direction in which the recurrence has no dependency)."""
import numpy as np

MCD_SCALE = 10.0 * np.sqrt(2.0) / np.log(10.0)


def dct_basis(n_mel, n_coef):
    """Rows 1 .. n_coef of the orthonormal DCT-II: B[k-1][n] = sqrt(2 / N) cos(pi (2 n + 1) k / (2 N)), float64 [n_coef][n_mel].  The angle
    is reduced in integers first ((2 n + 1) k mod 4 N, then the cosine's symmetries down to [0, pi / 4]), so that no rounding of a large
    argument enters."""
    N = n_mel
    q = (2 * np.arange(N)[None, :] + 1) * np.arange(1, n_coef + 1)[:, None] % (4 * N)
    q = np.where(q > 2 * N, 4 * N - q, q)                    # cos(2 pi - x) = cos x: q in [0, 2 N]
    sign = np.where(q > N, -1.0, 1.0)
    q = np.where(q > N, 2 * N - q, q)                        # cos(pi - x) = -cos x: q in [0, N]
    val = np.where(2 * q > N, np.sin(np.pi * (N - q) / (2.0 * N)), np.cos(np.pi * q / (2.0 * N)))
    return np.sqrt(2.0 / N) * sign * val


def cepstra(mel, B):
    """mel [T][n_mel] (float32 log-mel) -> [T][K] float64, each sum in ascending n."""
    m = np.asarray(mel).astype(np.float64)
    c = np.zeros((len(m), len(B)))
    for n in range(m.shape[1]):
        c += B[None, :, n] * m[:, n, None]
    return c


def cepstra_scale(mel, B):
    """sum_n |B[k][n] m[n]| per output: what the rounding bound of `cepstra` is relative to."""
    return (np.abs(np.asarray(mel).astype(np.float64))[:, None, :] * np.abs(B)[None]).sum(-1)


def frame_distance(a, b):
    q = np.zeros((len(a), len(b)))
    for k in range(a.shape[1]):
        t = a[:, None, k] - b[None, :, k]
        q += t * t
    return np.sqrt(q)


def dtw_tables(d):
    """d [Ta][Tb] -> (D [Ta][Tb], from [Ta][Tb] uint8: 0 = (i-1, j-1), 1 = (i-1, j), 2 = (i, j-1); ties to the first)."""
    ta, tb = d.shape
    P = np.full((ta + 1, tb + 1), np.inf)       # P[i + 1][j + 1] = D(i, j); the border is +inf, the corner 0 so that D(0, 0) = d(0, 0)
    P[0, 0] = 0.0
    frm = np.zeros((ta, tb), np.uint8)
    for s in range(ta + tb - 1):
        i = np.arange(max(0, s - tb + 1), min(ta - 1, s) + 1)
        j = s - i
        best, up, left = P[i, j].copy(), P[i, j + 1], P[i + 1, j]
        f = np.zeros(len(i), np.uint8)
        m = up < best
        best[m], f[m] = up[m], 1
        m = left < best
        best[m], f[m] = left[m], 2
        P[i + 1, j + 1] = d[i, j] + best
        frm[i, j] = f
    return P[1:, 1:], frm


def backtrack(D, frm, f0_a=None, f0_b=None):
    """-> (path [(i, j)] from (0, 0) forward, smallest decision margin along the path relative to D's end value — inf where no cell of
    the path had two candidates — and the F0 figures (n_voiced_both, cents RMSE, n_vuv_mismatch) or (nan, nan, nan))."""
    ta, tb = D.shape
    i, j, path, margin = ta - 1, tb - 1, [], np.inf
    both = one = 0
    ss = 0.0
    while True:
        path.append((i, j))
        if f0_a is not None:
            fa, fb = float(f0_a[i]), float(f0_b[j])
            if fa > 0.0 and fb > 0.0:
                c = 1200.0 * np.log2(fa / fb)
                ss += c * c
                both += 1
            elif fa > 0.0 or fb > 0.0:
                one += 1
        if i == 0 and j == 0:
            break
        cand = sorted(v for v in (D[i - 1, j - 1] if i and j else np.inf, D[i - 1, j] if i else np.inf, D[i, j - 1] if j else np.inf) if np.isfinite(v))
        if len(cand) > 1:
            margin = min(margin, cand[1] - cand[0])
        f = frm[i, j]
        if f != 2:
            i -= 1
        if f != 1:
            j -= 1
    end = D[-1, -1]
    figures = (float(both), float(np.sqrt(ss / both)) if both else np.nan, float(one)) if f0_a is not None else (np.nan, np.nan, np.nan)
    return path[::-1], (margin / end if end > 0 else 0.0), figures


def mcd(mel_a, mel_b, B, f0_a=None, f0_b=None):
    """-> (out [6] float64 as mtts_dtw_mcd_batch lays it out, path int32 [L][2], margin)."""
    D, frm = dtw_tables(frame_distance(cepstra(mel_a, B), cepstra(mel_b, B)))
    path, margin, fig = backtrack(D, frm, f0_a, f0_b)
    end, L = float(D[-1, -1]), len(path)
    return np.array([end, float(L), MCD_SCALE * end / float(L), *fig]), np.asarray(path, np.int32), margin


def brute_force(d):
    """The cheapest monotone path from (0, 0) to the far corner by enumeration of every path: (cost, number of paths)."""
    ta, tb = d.shape
    best, count = [np.inf], [0]

    def walk(i, j, cost):
        cost = cost + d[i, j]
        if i == ta - 1 and j == tb - 1:
            count[0] += 1
            best[0] = min(best[0], cost)
            return
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            if i + di < ta and j + dj < tb:
                walk(i + di, j + dj, cost)

    walk(0, 0, 0.0)
    return best[0], count[0]


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
def random_mel(T, n_mel=80, seed=0):
    """Log-mel-like frames: a smooth random walk over time around -5 with a spectral tilt, float32 [T][n_mel]; the cepstra are of the
    size real ones have (|c_1| about 10, the higher ones about 1)."""
    r = np.random.default_rng(seed)
    base = -5.0 - 3.0 * np.arange(n_mel) / n_mel
    walk = np.cumsum(0.35 * r.standard_normal((T, n_mel)), axis=0)
    walk -= walk.mean(0)
    smooth = np.cumsum(r.standard_normal((T, n_mel)), axis=1) * 0.15
    return (base[None] + 0.5 * walk / max(1.0, np.sqrt(T) / 4) + smooth).astype(np.float32)


def stretched_copy(mel, T_new, seed=0, noise=0.15):
    """The realistic pair: `mel` resampled to T_new frames along a monotone, locally uneven time map, plus noise."""
    r = np.random.default_rng(seed)
    T = len(mel)
    steps = r.uniform(0.5, 1.5, T_new)
    pos = np.concatenate([[0.0], np.cumsum(steps)[:-1]])
    pos *= (T - 1) / max(pos[-1], 1e-12) if T_new > 1 else 0.0
    lo = np.minimum(np.floor(pos).astype(int), T - 1)
    hi = np.minimum(lo + 1, T - 1)
    w = (pos - lo)[:, None]
    out = (1 - w) * mel[lo].astype(np.float64) + w * mel[hi].astype(np.float64)
    return (out + noise * r.standard_normal(out.shape)).astype(np.float32)
