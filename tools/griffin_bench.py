#!/usr/bin/env python3
"""Griffin-Lim on the device (csrc/griffin.h through TacotronSTFT.inv_mel_with_angles) for B utterances x S seconds, LibriTTS
configuration: milliseconds per call and per iteration and the real-time factor from device events after warm-up, the CPU time of the
torch restatement (tests/gl_oracle.py) on the same batch, and the algorithmic FLOPs and bytes.  Per-kernel shares of peak come from a
separate `rocprofv3 --kernel-trace --stats` run of this script.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=8)
    ap.add_argument("--secs", type=float, default=5.0)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-reps", type=int, default=1, help="torch restatement repetitions (0: skip)")
    a = ap.parse_args()
    import torch
    from meta_tts_amd.audio import audio_processing as AP
    from meta_tts_amd.audio import stft as S
    from meta_tts_amd.audio import tools

    sr, n_fft, hop = 22050, 1024, 256
    st = S.TacotronSTFT(n_fft, hop, n_fft, 80, sr, 0, 8000, max_samples=int(sr * a.secs) + 64)
    stream = torch.cuda.current_stream()
    st.set_stream(stream.cuda_stream)
    rs = np.random.RandomState(0)
    n = int(sr * a.secs)
    t = np.arange(n) / sr
    mels = []
    for _ in range(a.utts):
        w = 0.5 * np.sin(2 * np.pi * rs.uniform(100, 300) * t + 3 * np.sin(2 * np.pi * 0.7 * t)) + 0.02 * rs.standard_normal(n)
        mels.append(tools.get_mel_from_wav(w.astype(np.float32), st)[0])
    F = n_fft // 2 + 1
    angles = [AP.random_angles((1, F, m.shape[1] - 1))[0] for m in mels]
    T = sum(m.shape[1] - 1 for m in mels)
    audio_s = sum(hop * (m.shape[1] - 2) for m in mels) / sr

    for _ in range(a.warmup):
        st.inv_mel_with_angles(mels, angles, a.iters)
    ev_ms, wall_ms = [], []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        w0 = time.perf_counter()
        e0.record(stream)
        st.inv_mel_with_angles(mels, angles, a.iters)
        e1.record(stream)
        e1.synchronize()
        wall_ms.append((time.perf_counter() - w0) * 1e3)
        ev_ms.append(e0.elapsed_time(e1))
    ms = float(np.median(ev_ms))
    flops_iter = 2.0 * (2.0 * T * 2 * F * n_fft)
    samples = sum(hop * (m.shape[1] - 1) + n_fft for m in mels)
    kp = (2 * F + 3) & ~3
    bytes_iter = 4.0 * (samples + 2 * F * n_fft + T * kp        # forward GEMM: padded signals + basis in, spectrum out
                        + 2 * T * kp + T * F                     # phasor: spectrum in / out, magnitude
                        + T * kp + n_fft * kp + T * n_fft        # inverse GEMM
                        + T * n_fft + samples)                   # overlap-add: frames in, next padded signals out
    res = {"utts": a.utts, "secs": a.secs, "iters": a.iters, "frames": T, "audio_s": round(audio_s, 3),
           "ms_per_call": round(ms, 3), "ms_per_call_wall": round(float(np.median(wall_ms)), 3),
           "ms_per_iter": round(ms / max(1, a.iters), 4), "rtf": round(ms / 1e3 / audio_s, 5),
           "gflop_per_iter": round(flops_iter / 1e9, 3), "tflop_per_call": round(flops_iter * a.iters / 1e12, 4),
           "tflops_achieved": round(flops_iter * a.iters / (ms / 1e3) / 1e12, 2), "mb_per_iter": round(bytes_iter / 1e6, 2)}
    if a.cpu_reps > 0:
        import gl_oracle as GO
        torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
        o = GO.Stft(n_fft, hop, n_fft)
        cpu = []
        for _ in range(a.cpu_reps):
            c0 = time.perf_counter()
            with torch.no_grad():
                for m, an in zip(mels, angles):
                    GO.inv_mel(o, m, st.mel_basis, an, a.iters)
            cpu.append(time.perf_counter() - c0)
        res["cpu_torch_ms"] = round(float(np.median(cpu)) * 1e3, 1)
        res["cpu_threads"] = torch.get_num_threads()
        res["speedup_vs_cpu"] = round(res["cpu_torch_ms"] / ms, 1)
    st.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
