"""Time the device MOSNet (meta_tts_amd.mosnet.MOSNet on csrc/mosnet.h) at the shape of an evaluation set: synthetic weights, 608
synthetic utterances of 3 - 10 s (the reference scores 8 640 wavs one file at a time on the CPU; 608 is one mode of it).

Method: per leg the median wall time of 7 calls after 2 warm-up calls; a device call is one `score_wavs` of the whole list (uploads, the
resampler where there is one, STFT, the network, downloads, cut into device calls of `max_frames` frames); "spread" is max - min.  Legs:
  a   score_wavs of the 608 utterances at 16 kHz
  b   the same signals at 22 050 Hz, resampled on the device
  c   tests/mosnet_oracle.py in float32 torch on 16 host threads on the first 32 utterances (float64 numpy magnitudes), per utterance
  d   per-kernel rows from the statistics of a kernel trace of leg a (rocprofv3 --kernel-trace --stats -- python tools/mosnet_bench.py
      --leg a; then --kernel-stats <the kernel_stats csv>): every convolution instance's time per call of leg a and its TFLOP/s against the
      fp32 matrix peak, the recurrence, the projection / dense GEMMs
  r   what the compiler reports per kernel (--resources <the remarks of hipcc -Rpass-analysis=kernel-resource-usage>)
Writes profiles/mosnet_bench.json; legs that were not run keep the value the file already holds, or "not measured".  No target ratio is
set: the CPU leg is the only comparison, and it is an order of magnitude."""
import argparse
import csv
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "mosnet_bench.json")
N_UTTS, N_ORACLE = 608, 32
LEGS = ("a", "b", "c")
FP32_MATRIX_PEAK_TFLOPS = 157.3   # v_mfma_f32_32x32x2_f32 dense peak of the MI355X


def utterances(rate, n=N_UTTS):
    """n signals of 3 - 10 s at `rate`: noise under a slow envelope plus a tone, amplitudes that give magnitudes of order 1."""
    g = np.random.RandomState(0)
    out = []
    for i in range(n):
        m = int(rate * g.uniform(3.0, 10.0))
        t = np.arange(m) / rate
        out.append(((0.03 + 0.05 * g.rand()) * (0.5 + 0.5 * np.sin(2 * np.pi * 1.3 * t + i)) * g.standard_normal(m)
                    + 0.02 * np.sin(2 * np.pi * (120.0 + 3 * i) * t)).astype(np.float32))
    return out


def median_of(fn, calls=7, warmup=2):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return {"ms_median": round(1e3 * float(np.median(t)), 3), "ms_spread": round(1e3 * (max(t) - min(t)), 3), "ms_all": [round(1e3 * v, 3) for v in t]}


def frames_of(wavs16):
    return int(sum(len(w) // 256 + 1 for w in wavs16))


def device_leg(rate, calls, warmup):
    from meta_tts_amd import mosnet as M
    net = M.MOSNet(M.synthetic_state_dict(0))
    try:
        wavs = utterances(rate)
        res = median_of(lambda: net.score_wavs(wavs, source_rate=rate), calls, warmup)
        utt, frames = net.score_wavs(wavs, source_rate=rate)
    finally:
        net.close()
    n_frames = int(sum(len(f) for f in frames))
    res.update(utterances=len(wavs), seconds_of_audio=round(sum(len(w) for w in wavs) / rate, 1), frames=n_frames, source_rate=rate,
               ms_per_utterance=round(res["ms_median"] / len(wavs), 4), score_mean=round(float(np.mean(utt)), 4), score_std=round(float(np.std(utt)), 4))
    return res


def oracle_leg(calls, warmup):
    import torch
    import mosnet_oracle as MO
    from meta_tts_amd import mosnet as M
    torch.set_num_threads(16)
    sd = M.synthetic_state_dict(0)
    mags = [MO.stft_magnitude(w, dtype=np.float64).astype(np.float32) for w in utterances(16000, N_ORACLE)]
    res = median_of(lambda: MO.network(sd, mags, 257, torch.float32), calls, warmup)
    res.update(threads=16, utterances=N_ORACLE, frames=int(sum(len(m) for m in mags)), ms_per_utterance=round(res["ms_median"] / N_ORACLE, 3), calls=calls, warmup=warmup)
    return res


def conv_layers():
    """[(cin, cout, stride, F_out)] of layers 1 .. 11 at n_freq = 257 (layer 0 is the VALU kernel)."""
    from meta_tts_amd import mosnet as M
    w, out = M.widths(257), []
    for l in range(1, 12):
        b, j = divmod(l, 3)
        c = M.CHANNELS[b]
        out.append((c if j else M.CHANNELS[b - 1], c, 3 if j == 2 else 1, w[b + 1] if j == 2 else w[b]))
    return out


def kernels_from_stats(path, calls_in_trace, frames):
    rows = {}
    for row in csv.DictReader(open(path, newline="")):
        name = row.get("Name", "")
        if "mos_" in name or "gemm_f32" in name or "stft_" in name or "resample_" in name:
            rows[name] = rows.get(name, 0.0) + float(row["TotalDurationNs"])
    if not any("mos_conv3x3" in n for n in rows):
        return "not measured"
    out, conv_ms, conv_flops = {}, 0.0, 0.0
    for cin, cout, sf, f_out in conv_layers():
        ns = sum(v for n, v in rows.items() if re.search(rf"mos_conv3x3_kernelILi{cin}ELi{cout}ELi{sf}EE|mos_conv3x3_kernel<{cin}, {cout}, {sf}>", n))
        if ns == 0.0:
            continue
        per_call = ns / calls_in_trace * 1e-9
        flops = 2.0 * frames * f_out * 9.0 * cin * cout
        tf = flops / per_call * 1e-12
        out[f"mos_conv3x3_kernel<{cin},{cout},{sf}>"] = {"ms_per_call": round(1e3 * per_call, 3), "tflops": round(tf, 2),
                                                        "fraction_of_fp32_matrix_peak": round(tf / FP32_MATRIX_PEAK_TFLOPS, 3)}
        conv_ms += 1e3 * per_call
        conv_flops += flops
    out["all_mfma_convolutions"] = {"ms_per_call": round(conv_ms, 3), "tflops": round(conv_flops / (conv_ms * 1e-3) * 1e-12, 2)}
    for key in ("mos_conv_first_kernel", "mos_blstm_kernel", "mos_head_kernel", "gemm_f32", "stft_", "resample_"):
        ns = sum(v for n, v in rows.items() if key in n)
        if ns:
            out[key + ("*" if key.endswith("_") or key == "gemm_f32" else "")] = {"ms_per_call": round(ns / calls_in_trace * 1e-6, 3)}
    out["score_wavs_calls_in_trace"] = calls_in_trace
    return out


def resources_from_remarks(path):
    """{kernel: VGPRs / AGPRs / scratch bytes per lane / LDS bytes / waves per SIMD} of the mos_* kernels from hipcc's remarks."""
    out, cur = {}, None
    keys = {"VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane", "Occupancy [waves/SIMD]": "waves_per_simd",
            "LDS Size [bytes/block]": "lds_bytes"}
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            cur = None
            if "mos_" in name:
                t = re.search(r"mos_conv3x3_kernelILi(\d+)ELi(\d+)ELi(\d+)EE", name)
                cur = f"mos_conv3x3_kernel<{t.group(1)},{t.group(2)},{t.group(3)}>" if t else re.search(r"(mos_[a-z_0-9]+_kernel)", name).group(1)
                out[cur] = {}
            continue
        if cur:
            for k, v in keys.items():
                m = re.search(re.escape(k) + r": (\d+)", line)
                if m:
                    out[cur][v] = int(m.group(1))
    return out or "not measured"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", action="append", choices=LEGS, help="legs to run (default: all)")
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-stats", help="a rocprofv3 kernel_stats csv of a run of leg a: fills leg d")
    ap.add_argument("--resources", help="hipcc's -Rpass-analysis=kernel-resource-usage remarks of the library build: fills r")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    res.setdefault("method", "median of 7 calls after 2 warm-up calls; MOSNet with synthetic weights, 608 synthetic utterances of 3 - 10 s; a device call is one "
                             "score_wavs of the whole list (uploads, resampler, STFT, network, downloads; device calls of 8 192 frames); spread = max - min")
    ran = a.leg or ([] if (a.kernel_stats is not None or a.resources is not None) else list(LEGS))
    for leg in ran:
        res[leg] = oracle_leg(a.calls, a.warmup) if leg == "c" else device_leg(16000 if leg == "a" else 22050, a.calls, a.warmup)
        print(leg, json.dumps(res[leg]), flush=True)
    if a.kernel_stats:
        frames = res["a"]["frames"] if isinstance(res.get("a"), dict) else frames_of(utterances(16000))
        res["d"] = kernels_from_stats(a.kernel_stats, a.calls + a.warmup + 1, frames)
        print("d", json.dumps(res["d"]), flush=True)
    if a.resources:
        res["r"] = resources_from_remarks(a.resources)
    for leg in LEGS + ("d", "r"):
        res.setdefault(leg, "not measured")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
