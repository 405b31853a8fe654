"""Time the device t-SNE (meta_tts_amd.evaluation.TSNE on csrc/tsne.h) at the reference's two job sizes against sklearn on the host.

Method: synthetic clustered d-vectors (non-negative, L2-normalised, dim 256, 16 per speaker), max_iter=300, perplexity 40,
init="random"; per leg the median wall time of 7 fit_transform calls after 2 warm-up calls.  A device fit_transform creates and destroys
its handle, so the allocation of P (N^2 x 4 bytes), the upload of X, the affinities and the final device synchronisation all fall INSIDE
the timed region.  Legs:
  a  device, N = 3 040 (LibriTTS: 5 modes x 38 speakers x 16)        b  device, N = 8 640 (VCTK: 5 x 108 x 16)
  c  sklearn method="barnes_hut" (the reference's actual call), N = 3 040      d  sklearn method="exact", N = 3 040
plus the one-time affinity cost of the device legs (one mtts_tsne_affinities call, timed alone).  sklearn is imported lazily: a leg
whose import fails is reported as "not available".  The pair pass's own time comes from a kernel trace of leg b
(rocprofv3 --kernel-trace --stats -- python tools/tsne_bench.py --leg b) and is entered by hand.  Writes profiles/tsne_bench.json
(legs that were not run keep the value the file already holds, or "not measured")."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "tsne_bench.json")
SIZES = {"a": 38, "b": 108, "c": 38, "d": 38}


def dvectors(n_spk, n_per=5 * 16, dim=256, seed=0, spread=0.5):
    r = np.random.default_rng(seed)
    c = np.abs(r.standard_normal((n_spk, dim)))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    x = np.maximum(np.repeat(c, n_per, 0) + spread / np.sqrt(dim) * r.standard_normal((n_spk * n_per, dim)), 0)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def median_of(fn, calls=7, warmup=2):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), [round(v, 4) for v in t]


def device_leg(X):
    from meta_tts_amd import _lib
    from meta_tts_amd.evaluation import TSNE
    t = TSNE(perplexity=40, max_iter=300, init="random", random_state=0)
    med, all_t = median_of(lambda: t.fit_transform(X))
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.mtts_tsne_create(len(X), X.shape[1], 0, C.byref(h)) == 0
    aff = lambda: lib.mtts_tsne_affinities(h, X.ctypes.data_as(C.c_void_p), len(X), X.shape[1], 40.0, None, None)   # noqa: E731
    a_med, _ = median_of(aff)
    lib.mtts_tsne_destroy(h)
    return {"n": len(X), "seconds_median": round(med, 4), "seconds_all": all_t, "affinities_seconds_median": round(a_med, 4),
            "n_iter": t.n_iter_ + 1, "kl_divergence": t.kl_divergence_, "p_bytes_per_iteration": len(X) ** 2 * 4}


def sklearn_leg(X, method):
    try:
        from sklearn.manifold import TSNE
    except ImportError:
        return "not available"
    t = TSNE(n_components=2, perplexity=40, max_iter=300, init="random", random_state=0, method=method)
    med, all_t = median_of(lambda: t.fit_transform(X))
    return {"n": len(X), "seconds_median": round(med, 4), "seconds_all": all_t, "threads": int(os.environ.get("OMP_NUM_THREADS", os.cpu_count() or 1)),
            "kl_divergence": float(t.kl_divergence_)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", action="append", choices=list(SIZES), help="legs to run (default: all)")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    res.setdefault("method", "median of 7 fit_transform calls after 2 warm-up calls (handle create / destroy inside the timed region); synthetic clustered d-vectors, dim 256; max_iter=300, perplexity 40, init=random")
    for leg in a.leg or list(SIZES):
        X = dvectors(SIZES[leg])
        res[leg] = device_leg(X) if leg in "ab" else sklearn_leg(X, "barnes_hut" if leg == "c" else "exact")
        print(leg, json.dumps(res[leg]), flush=True)
    for leg in SIZES:
        res.setdefault(leg, "not measured")
    res.setdefault("pair_pass", "not measured")
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
