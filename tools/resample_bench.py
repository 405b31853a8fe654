#!/usr/bin/env python3
"""Device resampling in front of the packed waveform buffer (csrc/resample.h), kaiser_best, measured as four legs:
  a        Resampler(24000, 22050).resample_batch of 64 x 5 s, host to host;
  b        the evaluation set of tools/speaker_eval_bench.py (624 utterances of 3-10 s) synthesised at 22 050 Hz -> d-vectors through the
           chained entry (SpeakerEmbedder.embed_utterances(source_rate=22050, normalize_dbfs=-30): the 16 kHz signal stays on the device);
  c        the route possible without it: scipy.signal.resample_poly with the same filter on 16 host threads, then embed_utterances;
  d        embed_utterances of the same set at 16 kHz — the path that existed before — on this build and, with --parent-lib, on a
           libmtts.so built from the parent commit (alternating, two child processes each; the condition is |ratio - 1| <= 2 %).
Each leg runs in a child process of its own under a time limit, as the median wall time of 7 calls after 2 warm-up calls; every call
ends in a device synchronise (the entry points are synchronous); a leg that fails ends the run.  Writes profiles/resample_bench.json
and prints it.  The resample kernel's own time comes from a separate `rocprofv3 --kernel-trace --stats -- python
tools/resample_bench.py --leg a` run and is quoted against 8 bytes per output sample (profiles/resample_kernel_trace.md)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NEW_SYMBOLS = ("mtts_stft_load_resampler", "mtts_stft_resample_batch", "mtts_dvector_embed_wavs_resampled")   # absent from a parent-commit library


def corpus(utts, sr):
    """tools/speaker_eval_bench.py's set: the same durations and tones, sampled at `sr`."""
    g = np.random.RandomState(0)
    out = []
    for _ in range(utts):
        n = int(sr * (int(16000 * g.uniform(3.0, 10.0)) / 16000))
        t = np.arange(n) / sr
        out.append((0.5 * np.sin(2 * np.pi * g.uniform(100, 300) * t + 3 * np.sin(2 * np.pi * 0.7 * t)) + 0.02 * g.standard_normal(n)).astype(np.float32))
    return out


def leg(name, a):
    import torch
    assert torch.cuda.is_available(), "every leg needs an MI355X"
    from meta_tts_amd import _lib
    from meta_tts_amd import evaluation as E
    from meta_tts_amd.audio import resample as A
    from meta_tts_amd.speaker_encoder import synthetic_state_dict
    lib_path = None
    if name == "d_parent":
        lib_path = os.path.abspath(a.parent_lib)
        for s in NEW_SYMBOLS:
            _lib.EXPORTS.pop(s)
    extra = {}
    if name == "a":
        g = np.random.RandomState(1)
        wavs = [(0.3 * g.standard_normal(5 * 24000)).astype(np.float32) for _ in range(64)]
        rs = A.Resampler(24000, 22050)
        call = lambda: rs.resample_batch(wavs)   # noqa: E731
        audio = 64 * 5.0
        n_out = sum(rs.output_length(len(w)) for w in wavs)
        extra = {"n_out": n_out, "bytes_8_per_output": 8 * n_out, "taps": rs.taps, "up": rs.up, "down": rs.down}
    else:
        emb = E.SpeakerEmbedder(synthetic_state_dict(0), max_partials=a.max_partials, max_utts=a.max_partials, lib_path=lib_path)
        if name == "b":
            wavs = corpus(a.utts, 22050)
            call = lambda: emb.embed_utterances(wavs, source_rate=22050, normalize_dbfs=-30.0)   # noqa: E731
            audio = sum(len(w) for w in wavs) / 22050
        elif name == "c":
            from concurrent.futures import ThreadPoolExecutor
            from scipy import signal
            wavs = corpus(a.utts, 22050)
            up, down, H, h = A.resample_filter(22050, 16000, "kaiser_best")
            pool = ThreadPoolExecutor(16)

            def one(w):
                y = signal.resample_poly(w.astype(np.float64), up, down, window=h / up).astype(np.float32)
                return A.normalize_volume(y, -30.0, increase_only=True)[0].astype(np.float32)

            call = lambda: emb.embed_utterances(list(pool.map(one, wavs)))   # noqa: E731
            audio = sum(len(w) for w in wavs) / 22050
        else:
            wavs = corpus(a.utts, 16000)
            call = lambda: emb.embed_utterances(wavs)   # noqa: E731
            audio = sum(len(w) for w in wavs) / 16000
    for _ in range(a.warmup):
        res = call()
    times = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        res = call()
        times.append(time.perf_counter() - t0)
    s = float(np.median(times))
    check = float(np.abs(res[0][:1000]).sum()) if name == "a" else float(np.abs(res[:32]).sum())
    return dict({"utts": len(wavs), "audio_s": round(audio, 1), "ms_per_call": round(s * 1e3, 2), "ms_min": round(min(times) * 1e3, 2),
                 "ms_max": round(max(times) * 1e3, 2), "audio_s_per_s": round(audio / s, 1), "checksum": check}, **extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=624)
    ap.add_argument("--max-partials", type=int, default=2048)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--leg", default="all", choices=["all", "a", "b", "c", "d", "d_parent"])
    ap.add_argument("--parent-lib", default=None, help="a libmtts.so built from the parent commit (leg d's other arm)")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_bench.json"))
    a = ap.parse_args()
    if a.leg != "all":
        print(json.dumps(leg(a.leg, a)))
        return
    res = {"utts": a.utts, "max_partials": a.max_partials, "warmup": a.warmup, "reps": a.reps, "preset": "kaiser_best",
           "config": "a: 64 x 5 s 24000 -> 22050 Hz host to host; b / c / d: 624 utterances of 3-10 s, LSTM(40, 256, 3), synthetic weights"}
    order = ["a", "b", "c"] + (["d", "d_parent", "d", "d_parent"] if a.parent_lib else ["d", "d"])
    for name in order:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--utts", str(a.utts), "--max-partials", str(a.max_partials), "--warmup", str(a.warmup),
               "--reps", str(a.reps)] + (["--parent-lib", a.parent_lib] if a.parent_lib else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"leg {name} failed with status {r.returncode}: nothing further is started")
        res.setdefault(name, []).append(json.loads(r.stdout.strip().splitlines()[-1]))
    for name in ("a", "b", "c"):
        res[name] = res[name][0]
    res["b_speedup_vs_c"] = round(res["c"]["ms_per_call"] / res["b"]["ms_per_call"], 2)
    if a.parent_lib:
        this, parent = [np.mean([r["ms_per_call"] for r in res[k]]) for k in ("d", "d_parent")]
        res["d_this_over_parent"] = round(float(this / parent), 4)
        res["d_checksums_equal"] = len({r["checksum"] for k in ("d", "d_parent") for r in res[k]}) == 1
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
