"""Time the device HiFi-GAN generator (meta_tts_amd.hifigan.HiFiGAN on csrc/hifigan.h) at the shape of the adaptation / synthesis path:
the published V1 configuration with synthetic weights, 5 utterances x 400 frames (512 000 samples per call).

Method: per leg the median wall time of 7 calls after 2 warm-up calls; a device call is one `mel2wav` (upload of the mel, the generator,
download of the waveform); "spread" is max - min of the 7 calls.  Legs:
  a   GEMM route (direct_max_channels = 0)
  b   direct route for the stages with C <= 64 (direct_max_channels = 64)
  c   tests/hifigan_oracle.py in float32 on 16 host threads
  d   vocoder.MelGAN (synthetic weights) on the same mels, for context
  k   hg_conv_direct_kernel's own time per call and its TFLOP/s against the fp32 matrix peak, from the statistics of a kernel trace of
      leg b (rocprofv3 --kernel-trace --stats -- python tools/hifigan_bench.py --leg b; then --kernel-stats <the kernel_stats csv>)
  e   bf16 operands (numerics="bf16"), GEMM route (direct_max_channels = 0); reports the waveform's SNR in dB against leg a's
  f   bf16 operands, direct route for the stages with C <= 128 (direct_max_channels = 128); SNR as for e
  kb  hg_conv_direct_bf16_kernel's own time per call and its GB/s against its algorithmic bytes, from a kernel trace of leg f
      (rocprofv3 --kernel-trace --stats -- python tools/hifigan_bench.py --leg f; then --kernel-stats-bf16 <the kernel_stats csv>)
The SNR of e / f needs leg a in the same run (its waveform is the reference); it is reported, not gated.
`HiFiGAN`'s default direct_max_channels becomes 64 only if b beats a in one session by more than the larger of the two spreads
("direct_route_wins").  Writes profiles/hifigan_bench.json; legs that were not run keep the value the file already holds, or
"not measured"."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "hifigan_bench.json")
B, T, N_MEL = 5, 400, 80
LEGS = ("c", "a", "b", "d", "e", "f")
FP32_MATRIX_PEAK_TFLOPS = 157.3   # v_mfma_f32_32x32x2_f32 dense peak of the MI355X


def mels():
    g = np.random.RandomState(0)
    return (g.standard_normal((B, N_MEL, T)) * 1.5 - 4.0).astype(np.float32)


def median_of(fn, calls=7, warmup=2):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return {"ms_median": round(1e3 * float(np.median(t)), 3), "ms_spread": round(1e3 * (max(t) - min(t)), 3), "ms_all": [round(1e3 * v, 3) for v in t]}


def direct_flops(config):
    """multiply-add flops per call of the convolutions the direct route takes (C in {32, 64})"""
    c, rows, total = config["upsample_initial_channel"], T, 0.0
    for i, r in enumerate(config["upsample_rates"]):
        c //= 2
        rows *= r
        if c in (32, 64):
            for j, k in enumerate(config["resblock_kernel_sizes"]):
                total += 2.0 * len(config["resblock_dilation_sizes"][j]) * 2.0 * B * rows * k * c * c
    return total


def direct_bf16_bytes(config):
    """algorithmic bytes per call of hg_conv_direct_bf16_kernel (C in {32, 64, 128}): fp32 activations in and out, the residual and the MRF
    sum where the epilogue touches them, the bf16 weight image once per convolution"""
    c, rows, total = config["upsample_initial_channel"], T, 0.0
    for i, r in enumerate(config["upsample_rates"]):
        c //= 2
        rows *= r
        if c in (32, 64, 128):
            act = 4.0 * B * rows * c
            for j, k in enumerate(config["resblock_kernel_sizes"]):
                n_dil = len(config["resblock_dilation_sizes"][j])
                for m in range(n_dil):
                    total += 2 * act + 2.0 * k * c * c                       # first convolution of the pair: x in, t out
                    last = m == n_dil - 1
                    total += (3 + (1 if last and j > 0 else 0)) * act + 2.0 * k * c * c   # second: t and res in, x or the MRF sum out (read too for j > 0)
    return total


_WAV_A = {}


def snr_db(wav, ref):
    err = float(np.sum((wav.astype(np.float64) - ref) ** 2))
    return round(10.0 * np.log10(float(np.sum(ref.astype(np.float64) ** 2)) / err), 2) if err > 0 else float("inf")


def hifigan_leg(direct_max, calls, warmup, numerics="fp32", leg=None):
    from meta_tts_amd import hifigan as H
    voc = H.HiFiGAN(H.synthetic_state_dict(0), max_B=B, max_T=T, direct_max_channels=direct_max, numerics=numerics)
    try:
        m = mels()
        res = median_of(lambda: voc.mel2wav(m), calls, warmup)
        wav = voc.mel2wav(m)
    finally:
        voc.close()
    res["direct_max_channels"] = direct_max
    if leg == "a":
        _WAV_A["wav"] = wav
    if numerics != "fp32":
        res["numerics"] = numerics
        res["snr_db_vs_leg_a"] = snr_db(wav, _WAV_A["wav"]) if "wav" in _WAV_A else "not measured"
    return res


def oracle_leg(calls, warmup):
    import torch
    import hifigan_oracle as HO
    from meta_tts_amd import hifigan as H
    torch.set_num_threads(16)
    sd, m = H.synthetic_state_dict(0), mels()
    res = median_of(lambda: HO.generator(sd, m, H.V1, torch.float32), calls, warmup)
    res["threads"] = 16
    return res


def melgan_leg(calls, warmup):
    from meta_tts_amd import vocoder as V
    voc = V.MelGAN(V.synthetic_state_dict(0), max_B=B, max_T=T)
    try:
        m = mels()
        return median_of(lambda: voc.mel2wav(m, mel_scale=1.0 / np.log(10.0)), calls, warmup)
    finally:
        voc.close()


def kernel_from_stats(path, calls_per_run):
    from meta_tts_amd import hifigan as H
    total_ns = 0.0
    for row in csv.DictReader(open(path, newline="")):
        if "hg_conv_direct_kernel" in row.get("Name", ""):
            total_ns += float(row["TotalDurationNs"])
    if total_ns == 0.0:
        return "not measured"
    per_call = total_ns / calls_per_run * 1e-9
    tf = direct_flops(H.V1) / per_call * 1e-12
    return {"ms_per_call": round(1e3 * per_call, 3), "tflops": round(tf, 2), "fraction_of_fp32_matrix_peak": round(tf / FP32_MATRIX_PEAK_TFLOPS, 3),
            "generator_calls_in_trace": calls_per_run}


def kernel_bf16_from_stats(path, calls_per_run):
    from meta_tts_amd import hifigan as H
    total_ns = 0.0
    for row in csv.DictReader(open(path, newline="")):
        if "hg_conv_direct_bf16_kernel" in row.get("Name", ""):
            total_ns += float(row["TotalDurationNs"])
    if total_ns == 0.0:
        return "not measured"
    per_call = total_ns / calls_per_run * 1e-9
    return {"ms_per_call": round(1e3 * per_call, 3), "algorithmic_gb": round(direct_bf16_bytes(H.V1) * 1e-9, 3),
            "gb_per_s": round(direct_bf16_bytes(H.V1) / per_call * 1e-9, 1), "generator_calls_in_trace": calls_per_run}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", action="append", choices=LEGS, help="legs to run (default: all)")
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-stats", help="a rocprofv3 kernel_stats csv of a run of leg b: fills leg k")
    ap.add_argument("--kernel-stats-bf16", help="a rocprofv3 kernel_stats csv of a run of leg f: fills leg kb")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    res.setdefault("method", "median of 7 calls after 2 warm-up calls; HiFi-GAN V1, synthetic weights, 5 utterances x 400 frames; a device call is one "
                             "mel2wav (mel upload, generator, waveform download); spread = max - min of the 7 calls")
    ran = a.leg or ([] if (a.kernel_stats or a.kernel_stats_bf16) else list(LEGS))
    ran = sorted(ran, key=lambda leg: leg != "a")   # leg a first: its waveform is the reference of the SNR of e / f
    for leg in ran:
        res[leg] = (oracle_leg(a.calls, a.warmup) if leg == "c" else melgan_leg(a.calls, a.warmup) if leg == "d"
                    else hifigan_leg(0, a.calls, a.warmup, "bf16") if leg == "e" else hifigan_leg(128, a.calls, a.warmup, "bf16") if leg == "f"
                    else hifigan_leg(0 if leg == "a" else 64, a.calls, a.warmup, leg=leg))
        print(leg, json.dumps(res[leg]), flush=True)
    if a.kernel_stats:
        res["k"] = kernel_from_stats(a.kernel_stats, a.calls + a.warmup)
        print("k", json.dumps(res["k"]), flush=True)
    if a.kernel_stats_bf16:
        res["kb"] = kernel_bf16_from_stats(a.kernel_stats_bf16, a.calls + a.warmup + 1)   # (+1: the call that keeps the waveform)
        print("kb", json.dumps(res["kb"]), flush=True)
    for leg in LEGS + ("k", "kb"):
        res.setdefault(leg, "not measured")
    if "a" in ran and "b" in ran:   # one session: the comparison that decides the default
        margin = max(res["a"]["ms_spread"], res["b"]["ms_spread"])
        res["direct_route_wins"] = bool(res["a"]["ms_median"] - res["b"]["ms_median"] > margin)
    res.setdefault("direct_route_wins", "not measured")
    for leg in ("e", "f"):   # one session: bf16 against fp32's GEMM route
        if "a" in ran and leg in ran:
            margin = max(res["a"]["ms_spread"], res[leg]["ms_spread"])
            res[f"bf16_leg_{leg}_beats_a"] = bool(res["a"]["ms_median"] - res[leg]["ms_median"] > margin)
        res.setdefault(f"bf16_leg_{leg}_beats_a", "not measured")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
