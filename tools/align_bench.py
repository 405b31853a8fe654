"""Time the device forced aligner (meta_tts_amd.align.MonophoneAligner on csrc/align.h) at a small corpus's size against the float64
numpy oracle on the host.

Method: 64 synthetic utterances of 3 .. 10 s at 22 050 / 256 (258 .. 861 frames), 40 .. 120 states each (about one per seven frames), 80
features, 70 classes, class 0 an optional silence at every sixth state; frames drawn around class means on random durations.  Per leg
the median wall time of 7 calls after 2 warm-up calls on one reused handle (its workspace, once grown, stays); packing, upload and
download fall inside the timed region.  Legs:
  a   one EM iteration: em_begin, one em_accumulate of all 64 utterances, em_finish (emission, forward, backward, statistics, fold, M step)
  b   align: emission, Viterbi sweep, backtrack
  c   tests/align_oracle.py: the E step (posteriors and per-state statistics) of the first 16 of those utterances over a pool of 16 host
      processes, one utterance per task
  d   the sweep kernels' own time per launch (align_sweep_kernel<false>, align_backward_kernel, and every other align_* kernel), from
      the statistics of a kernel trace of leg a (rocprofv3 --kernel-trace --stats -- python tools/align_bench.py --leg a; then
      --kernel-stats <the kernel_stats csv>)
Writes profiles/align_bench.json; legs that were not run keep the value the file already holds, or "not measured"."""
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
OUT = os.path.join(ROOT, "profiles", "align_bench.json")
N_UTTS, N_ORACLE, HOST_PROCESSES, N_FEAT, N_CLASSES = 64, 16, 16, 80, 70
LEGS = ("c", "a", "b")    # (the host leg first: its pool is up and gone before this process opens the device)


def make_corpus(seed=0):
    r = np.random.default_rng(seed)
    means = r.normal(-5.0, 2.0, (N_CLASSES, N_FEAT))
    feats, seqs = [], []
    for _ in range(N_UTTS):
        T = int(r.integers(258, 862))
        S = int(np.clip(T // 7, 40, 120))
        cls = []
        for s in range(S):
            c = 0 if s % 6 == 5 else int(r.integers(1, N_CLASSES))
            while cls and c == cls[-1]:
                c = int(r.integers(1, N_CLASSES))
            cls.append(c)
        cut = np.sort(r.choice(np.arange(1, T), S - 1, replace=False))
        state = np.repeat(np.arange(S), np.diff(np.concatenate([[0], cut, [T]])))
        feats.append((means[np.asarray(cls)[state]] + r.standard_normal((T, N_FEAT))).astype(np.float32))
        seqs.append([f"p{c}" for c in cls])
    return feats, seqs


def median_of(fn, calls=7, warmup=2):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), [round(v, 4) for v in t]


def shape(feats, seqs):
    return {"utterances": len(feats), "frames": int(sum(len(x) for x in feats)), "states": int(sum(len(s) for s in seqs)),
            "cells": int(sum(len(x) * len(s) for x, s in zip(feats, seqs)))}


def device_leg(corpus, leg, calls, warmup):
    from meta_tts_amd.align import MonophoneAligner
    feats, seqs = corpus
    a = MonophoneAligner([f"p{c}" for c in range(N_CLASSES)], n_feat=N_FEAT, optional=("p0",), max_frames=1024, max_states=128, max_cells=1 << 24, max_utts=64)
    try:
        a.flat_start(feats)
        a.em_iteration(feats, seqs, batch_utterances=N_UTTS)
        out = []
        if leg == "a":
            med, all_t = median_of(lambda: out.append(a.em_iteration(feats, seqs, batch_utterances=N_UTTS)[0]), calls, warmup)
            extra = {"total_ll_last": out[-1]}
        else:
            med, all_t = median_of(lambda: out.append(a.align(feats, seqs)), calls, warmup)
            extra = {"frames_aligned": int(sum(int(d.sum()) for d in out[-1]))}
    finally:
        a.close()
    s = shape(feats, seqs)
    return {**s, "seconds_median": round(med, 4), "seconds_all": all_t, "cells_per_second": round(s["cells"] / med), **extra}


def _oracle_one(job):
    import align_oracle as O
    x, cls, opt = job
    model = O.Model(np.zeros((N_CLASSES, N_FEAT)) - 5.0, np.full((N_CLASSES, N_FEAT), 5.0), np.full(N_FEAT, 5.0))
    LL, gamma = O.posteriors(x, model, cls, opt)
    return LL, float(O.state_stats(x, gamma)[:, 0].sum())


def oracle_leg(corpus):
    feats, seqs = (v[:N_ORACLE] for v in corpus)
    jobs = [(x, np.asarray([int(p[1:]) for p in s], np.int32), np.asarray([p == "p0" for p in s], np.uint8)) for x, s in zip(feats, seqs)]
    with multiprocessing.get_context("spawn").Pool(HOST_PROCESSES) as pool:
        out = []
        med, all_t = median_of(lambda: out.append(pool.map(_oracle_one, jobs, chunksize=1)))
    s = shape(feats, seqs)
    return {**s, "processes": HOST_PROCESSES, "seconds_median": round(med, 4), "seconds_all": all_t, "cells_per_second": round(s["cells"] / med),
            "occupancy_sum": float(sum(o[1] for o in out[-1]))}


def kernels_from_stats(path):
    """The align_* rows of a rocprofv3 kernel_stats csv -> launches and time per launch of each."""
    res = {}
    for row in csv.DictReader(open(path, newline="")):
        name = row.get("Name", "")
        if "align_" in name:
            short = name.split("(")[0].replace("void ", "").replace("mtts::", "")
            calls, total_ns = int(row["Calls"]), float(row["TotalDurationNs"])
            res[short] = {"launches": calls, "seconds_per_launch": round(total_ns / calls * 1e-9, 6), "percent_of_gpu_time": float(row.get("Percentage", "nan"))}
    return res or "not measured"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", action="append", choices=LEGS, help="legs to run (default: all)")
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-stats", help="a rocprofv3 kernel_stats csv of a run of leg a: fills leg d")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    res.setdefault("method", "median of 7 calls after 2 warm-up calls on one reused handle, upload and download inside; 64 synthetic utterances of 258..861 frames, "
                             "40..120 states, 80 features, 70 classes; oracle: the E step of 16 of the utterances over 16 host processes")
    corpus = make_corpus()
    for leg in a.leg or ([] if a.kernel_stats else list(LEGS)):
        res[leg] = oracle_leg(corpus) if leg == "c" else device_leg(corpus, leg, a.calls, a.warmup)
        print(leg, json.dumps(res[leg]), flush=True)
    if a.kernel_stats:
        res["d"] = kernels_from_stats(a.kernel_stats)
        print("d", json.dumps(res["d"]), flush=True)
    for leg in LEGS + ("d",):
        res.setdefault(leg, "not measured")
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
