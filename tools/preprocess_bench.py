#!/usr/bin/env python3
"""The preprocessing stage for U utterances x S seconds at the LibriTTS configuration (1024 / 256 / 1024, 80 mels, 22050 Hz,
phoneme-level pitch and energy, no file I/O): utterances/s and audio-seconds/s of
  new          the batched device path (meta_tts_amd/preprocessor.py: mel_batch, phoneme_average x 2, outlier_stats x 2, merge_stats,
               normalize_values x 2 — all utterances share every launch);
  device_loop  the route before it: one get_mel_from_wav call per utterance on the device, the remaining steps in numpy;
  cpu          the torch / numpy restatement (oracle/stft_oracle.py + the same numpy steps) on 16 threads;
  new_f0       `new` with the pitch computed too: one f0_batch call (csrc/pitch.h, YIN) in front, its output fed to the pitch steps;
  f0           that f0_batch call alone;
  f0_host      the same F0 definition in float64 numpy (tests/f0_oracle.py), utterances spread over 16 threads.
The first three legs take an injected f0 (pitch extraction is not part of their numbers).
Each leg runs in a child process of its own under a time limit, after warm-up, as the median wall time of repeated calls that end in
a device synchronise (every entry point is synchronous); a leg that fails ends the run.  Writes profiles/preprocess_bench.json and
prints it.  Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/preprocess_bench.py --leg new` run."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SR, N_FFT, HOP, N_MEL = 22050, 1024, 256, 80
CFG = {"path": {"raw_path": "", "preprocessed_path": ""},
       "preprocessing": {"val_size": 0, "audio": {"sampling_rate": SR, "max_wav_value": 32768.0},
                         "stft": {"filter_length": N_FFT, "hop_length": HOP, "win_length": N_FFT},
                         "mel": {"n_mel_channels": N_MEL, "mel_fmin": 0, "mel_fmax": None},
                         "pitch": {"feature": "phoneme_level", "normalization": True},
                         "energy": {"feature": "phoneme_level", "normalization": True}}}


def corpus(utts, secs):
    g = np.random.RandomState(0)
    out = []
    for u in range(utts):
        n = int(SR * secs) + 37 * u
        T = n // HOP + 1
        durs = []
        while sum(durs) < T - 12:
            durs.append(int(g.randint(0, 12)))
        t = np.arange(n) / SR
        w = (0.5 * np.sin(2 * np.pi * g.uniform(100, 300) * t + 3 * np.sin(2 * np.pi * 0.7 * t)) + 0.02 * g.standard_normal(n)).astype(np.float32)
        f0 = 120 + 40 * g.standard_normal(T)
        f0[g.rand(T) < 0.3] = 0
        out.append((w, durs, f0))
    return out


def host_steps(energies, f0s, durs):
    """preprocessor.py:231-261, 348-369 and partial_fit in numpy, utterance by utterance."""
    state = {"pitch": np.zeros(3), "energy": np.zeros(3)}
    saved = {"pitch": [], "energy": []}

    def seg(x, d):
        pos = 0
        for i, k in enumerate(d):
            x[i] = np.mean(x[pos: pos + k]) if k > 0 else 0
            pos += k
        return x[: len(d)]

    def fit(st, v):
        p25, p75 = np.percentile(v, 25), np.percentile(v, 75)
        lo, hi = p25 - 1.5 * (p75 - p25), p75 + 1.5 * (p75 - p25)
        v = v[(v > lo) & (v < hi)].astype(np.float64)
        if len(v) == 0:
            return
        n, m = float(len(v)), float(v.mean())
        M2 = float(((v - m) ** 2).sum())
        tot = st[0] + n
        delta = m - st[1]
        st[2] += M2 + delta * delta * st[0] * n / tot
        st[1] += delta * n / tot
        st[0] = tot

    for e, f0, d in zip(energies, f0s, durs):
        total = sum(d)
        p = np.array(f0[:total], np.float64)
        nz = np.where(p != 0)[0]
        p = np.interp(np.arange(len(p)), nz, p[nz])
        p = seg(p, d)
        e = seg(np.array(e[:total]), d)
        saved["pitch"].append(p)
        saved["energy"].append(e)
        fit(state["pitch"], p)
        fit(state["energy"], e)
    stats = {}
    for k in ("pitch", "energy"):
        mean, std = state[k][1], float(np.sqrt(state[k][2] / state[k][0]))
        lo, hi = np.inf, -np.inf
        for v in saved[k]:
            v = (v - mean) / std
            lo, hi = min(lo, v.min()), max(hi, v.max())
        stats[k] = [lo, hi, mean, std]
    return stats


def leg(name, a):
    data = corpus(a.utts, a.secs)
    wavs, durs, f0s = [d[0] for d in data], [d[1] for d in data], [d[2] for d in data]
    keep = [sum(d) for d in durs]
    if name == "f0_host":
        from concurrent.futures import ThreadPoolExecutor
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import f0_oracle
        pool = ThreadPoolExecutor(16)

        def call():
            f0 = list(pool.map(lambda w: f0_oracle.yin(w, SR, HOP)[0], wavs))
            return {"pitch": [min(f.min() for f in f0), max(f.max() for f in f0), float(np.mean([f.mean() for f in f0])), float(np.mean([(f > 0).mean() for f in f0]))]}
    elif name == "cpu":
        import torch
        from meta_tts_amd.audio.stft import mel_filterbank
        from oracle import stft_oracle as orc
        torch.set_num_threads(16)
        basis = mel_filterbank(SR, N_FFT, N_MEL, 0, None)

        def call():
            en = [orc.mel_spectrogram(w, N_FFT, HOP, N_FFT, basis)[1] for w in wavs]
            return host_steps(en, f0s, durs)
    else:
        import torch
        assert torch.cuda.is_available(), "the device legs need an MI355X"
        from meta_tts_amd.audio import tools
        from meta_tts_amd.preprocessor import Preprocessor
        pp = Preprocessor(CFG, max_samples=int(SR * a.secs) + 37 * a.utts + 64)
        if name == "f0":
            def call():
                f0 = pp.f0_batch(wavs)[0]
                return {"pitch": [min(f.min() for f in f0), max(f.max() for f in f0), float(np.mean([f.mean() for f in f0])), float(np.mean([(f > 0).mean() for f in f0]))]}
        elif name == "device_loop":
            def call():
                en = [tools.get_mel_from_wav(w, pp.STFT)[1] for w in wavs]
                return host_steps(en, f0s, durs)
        else:
            def call():
                f0 = pp.f0_batch(wavs)[0] if name == "new_f0" else f0s
                _, en = pp.mel_batch(wavs, keep)
                p = pp.phoneme_average([f[:k] for f, k in zip(f0, keep)], durs, interpolate=True)
                e = pp.phoneme_average(en, durs)
                stats = {}
                for k, v in (("pitch", p), ("energy", e)):
                    _, parts = pp.outlier_stats(v)
                    mean, std = pp.mean_std(pp.merge_stats(np.zeros(3), parts))
                    _, lo, hi = pp.normalize_values(v, mean, std)
                    stats[k] = [lo, hi, mean, std]
                return stats
    for _ in range(a.warmup):
        stats = call()
    times = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        stats = call()
        times.append(time.perf_counter() - t0)
    s = float(np.median(times))
    audio = sum(len(w) for w in wavs) / SR
    return {"ms_per_call": round(s * 1e3, 2), "ms_min": round(min(times) * 1e3, 2), "ms_max": round(max(times) * 1e3, 2),
            "utterances_per_s": round(a.utts / s, 1), "audio_s_per_s": round(audio / s, 1), "stats": {k: [float(x) for x in v] for k, v in stats.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--secs", type=float, default=5.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--leg", default="all", choices=["all", "new", "device_loop", "cpu", "new_f0", "f0", "f0_host"])
    ap.add_argument("--timeout", type=int, default=240, help="seconds per leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preprocess_bench.json"))
    a = ap.parse_args()
    if a.leg != "all":
        print(json.dumps(leg(a.leg, a)))
        return
    res = {"utts": a.utts, "secs": a.secs, "warmup": a.warmup, "reps": a.reps, "config": "LibriTTS 1024/256/1024, 80 mels, 22050 Hz, phoneme level"}
    for name in ("new", "device_loop", "cpu", "new_f0", "f0", "f0_host"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--utts", str(a.utts), "--secs", str(a.secs), "--warmup", str(a.warmup),
                            "--reps", str(a.reps)], capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"leg {name} failed with status {r.returncode}: nothing further is started")
        res[name] = json.loads(r.stdout.strip().splitlines()[-1])
    res["speedup_vs_device_loop"] = round(res["device_loop"]["ms_per_call"] / res["new"]["ms_per_call"], 2)
    res["speedup_vs_cpu"] = round(res["cpu"]["ms_per_call"] / res["new"]["ms_per_call"], 2)
    res["f0_speedup_vs_host"] = round(res["f0_host"]["ms_per_call"] / res["f0"]["ms_per_call"], 2)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
