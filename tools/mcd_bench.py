"""Time the device MCD / DTW (meta_tts_amd.evaluation.MelCepstralDistortion on csrc/dtw.h) at an evaluation step's size against the
float64 numpy oracle on the host.

Method: 608 pairs (a fifth of LibriTTS's 3 040 per adaptation step) of synthetic log-mels, 260 .. 860 frames per side, side B a
time-stretched noisy copy of side A, F0 tracks with voiced stretches; per leg the median wall time of 7 calls after 2 warm-up calls.
A device call is one `mcd_batch`: packing, upload, cepstra, sweep, backtrack and download all fall inside the timed region; the handle
(and its workspace, once grown) is reused from call to call, as an evaluation reuses it from mode to mode.  Legs:
  a_f0, a_nof0   device, 608 pairs, with and without F0 tracks
  b              tests/mcd_oracle.py (float64 numpy, the DP vectorised along anti-diagonals) on the first 32 of those pairs, over a pool
                 of 16 host processes
  c              dtw_sweep_kernel's own time per call and cells per second, from the statistics of a kernel trace of leg a_nof0
                 (rocprofv3 --kernel-trace --stats -- python tools/mcd_bench.py --leg a_nof0; then --kernel-stats <the kernel_stats csv>; the csv's rows for
                 this handle's kernels are kept by hand in profiles/mcd_kernel_trace.md)
Writes profiles/mcd_bench.json; legs that were not run keep the value the file already holds, or "not measured"."""
import argparse
import csv
import json
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "mcd_bench.json")
N_PAIRS, N_ORACLE, HOST_PROCESSES = 608, 32, 16
LEGS = ("b", "a_f0", "a_nof0")    # (the host leg first: its pool is up and gone before this process opens the device)


def make_pairs(n_pairs=N_PAIRS, seed=0):
    import mcd_oracle as O
    r = np.random.default_rng(seed)
    base = O.random_mel(860, 80, seed=1)
    A, Bs, fa, fb = [], [], [], []
    for p in range(n_pairs):
        ta, tb = (int(v) for v in r.integers(260, 861, 2))
        a = np.roll(base, int(r.integers(0, 860)), axis=0)[:ta] + (0.05 * r.standard_normal((ta, 80))).astype(np.float32)
        A.append(np.ascontiguousarray(a, np.float32))
        Bs.append(O.stretched_copy(a, tb, seed=p))
        for T, out in ((ta, fa), (tb, fb)):
            f = np.where(np.sin(np.arange(T) / 9.0 + p) > -0.3, 120.0 + 40.0 * np.sin(np.arange(T) / 23.0 + p), 0.0)
            out.append(f.astype(np.float64))
    return A, Bs, fa, fb


def median_of(fn, calls=7, warmup=2):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), [round(v, 4) for v in t]


def device_leg(pairs, with_f0, calls, warmup):
    from meta_tts_amd.evaluation import MelCepstralDistortion
    A, Bs, fa, fb = pairs
    cells = int(sum(len(a) * len(b) for a, b in zip(A, Bs)))
    m = MelCepstralDistortion(max_frames=1024, max_cells=1 << 28)
    try:
        out = []
        med, all_t = median_of(lambda: out.append(m.mcd_batch(A, Bs, fa if with_f0 else None, fb if with_f0 else None)), calls, warmup)
    finally:
        m.close()
    return {"pairs": len(A), "cells": cells, "seconds_median": round(med, 4), "seconds_all": all_t, "cells_per_second": round(cells / med),
            "mean_mcd_db": float(out[-1][:, 2].mean())}


def _oracle_one(job):
    import mcd_oracle as O
    a, b, fa, fb = job
    return O.mcd(a, b, O.dct_basis(80, 13), fa, fb)[0]


def oracle_leg(pairs):
    A, Bs, fa, fb = (v[:N_ORACLE] for v in pairs)
    cells = int(sum(len(a) * len(b) for a, b in zip(A, Bs)))
    jobs = list(zip(A, Bs, fa, fb))
    with multiprocessing.get_context("spawn").Pool(HOST_PROCESSES) as pool:
        out = []
        med, all_t = median_of(lambda: out.append(pool.map(_oracle_one, jobs, chunksize=1)))
    return {"pairs": len(A), "cells": cells, "processes": HOST_PROCESSES, "seconds_median": round(med, 4), "seconds_all": all_t, "cells_per_second": round(cells / med),
            "mean_mcd_db": float(np.mean([o[2] for o in out[-1]]))}


def sweep_from_stats(path, cells_per_call):
    """The dtw_sweep_kernel row of a rocprofv3 kernel_stats csv -> its time per call and cells per second."""
    for row in csv.DictReader(open(path, newline="")):
        if "dtw_sweep_kernel" in row.get("Name", ""):
            calls, total_ns = int(row["Calls"]), float(row["TotalDurationNs"])
            per_call = total_ns / calls * 1e-9
            return {"launches": calls, "seconds_per_launch": round(per_call, 6), "cells_per_second": round(cells_per_call / per_call), "source": "profiles/mcd_kernel_trace.md"}
    return "not measured"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", action="append", choices=LEGS, help="legs to run (default: all)")
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-stats", help="a rocprofv3 kernel_stats csv of a run of leg a_nof0: fills leg c")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    res.setdefault("method", "median of 7 calls after 2 warm-up calls; 608 synthetic pairs of 260..860 frames per side, 80 mels, 13 coefficients; "
                             "device: one mcd_batch per call on a reused handle; oracle: 32 of the pairs over 16 host processes")
    pairs = make_pairs()
    for leg in a.leg or ([] if a.kernel_stats else list(LEGS)):
        res[leg] = oracle_leg(pairs) if leg == "b" else device_leg(pairs, leg == "a_f0", a.calls, a.warmup)
        print(leg, json.dumps(res[leg]), flush=True)
    if a.kernel_stats:
        res["c"] = sweep_from_stats(a.kernel_stats, int(sum(len(x) * len(y) for x, y in zip(pairs[0], pairs[1]))))
        print("c", json.dumps(res["c"]), flush=True)
    for leg in LEGS + ("c",):
        res.setdefault(leg, "not measured")
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
