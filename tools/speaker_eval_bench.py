#!/usr/bin/env python3
"""The wav -> d-vector stage of a speaker-similarity evaluation for a LibriTTS-sized slice (default: 624 utterances of 3-10 s at
16 kHz, LSTM(40, 256, 3) with synthetic weights; no file I/O): utterances/s and audio-seconds/s of
  new     the batched device chain (meta_tts_amd/evaluation.py: SpeakerEmbedder.embed_utterances — packed STFT, power, mel, device
          gather, encoder; all utterances of a chunk share every launch);
  pcm16   the same set held as int16 through SpeakerEmbedder.embed_pcm16 (2 bytes per sample uploaded, widened on the device);
  device  the same samples resident in device memory as [utts][longest] float32 rows through SpeakerEmbedder.embed_device;
  today   the route possible before it: a numpy float32 front-end on the host (framing, basis product, power, mel, slicing) and
          one mtts_dvector_embed call per utterance with host mels;
  cpu     the torch restatement on 16 threads, one utterance at a time as the reference's evaluation/wavs_to_dvector.py does
          (--cpu-utts utterances, 32 by default, one warm-up and at most three repeats: the rate is what is compared).
Each leg runs in a child process of its own under a time limit, after warm-up, as the median wall time of repeated calls that end in
a device synchronise (every entry point is synchronous); a leg that fails ends the run.  Writes profiles/speaker_eval_bench.json and
prints it; `--legs a,b` runs only those legs and merges them into the file that is there.  pcm16 and device hold the float leg's samples
cut to 16 bits (trunc(x * 32768)), so their d-vectors differ from the float leg's in the last digits and agree with each other.
Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/speaker_eval_bench.py --leg new` (or pcm16 /
device: wav_ingest_kernel against 6 / 8 bytes per sample) run."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SR, N_FFT, HOP, N_MEL, FRAMES = 16000, 400, 160, 40, 160   # FRAMES: frames of a partial utterance


def corpus(utts):
    g = np.random.RandomState(0)
    out = []
    for u in range(utts):
        n = int(SR * g.uniform(3.0, 10.0))
        t = np.arange(n) / SR
        out.append((0.5 * np.sin(2 * np.pi * g.uniform(100, 300) * t + 3 * np.sin(2 * np.pi * 0.7 * t)) + 0.02 * g.standard_normal(n)).astype(np.float32))
    return out


def host_slices(wav, basis, melb, slices_of, xp=np):
    """The partial stack of one waveform on the host in float32 (numpy, or torch when xp is torch)."""
    wav_sl, mel_sl = slices_of(len(wav))
    if wav_sl[-1].stop >= len(wav):
        wav = np.pad(wav, (0, wav_sl[-1].stop - len(wav)), "constant")
    x = np.pad(wav, N_FFT // 2, mode="reflect")
    T = len(wav) // HOP + 1
    frames = np.lib.stride_tricks.as_strided(x, (T, N_FFT), (x.strides[0] * HOP, x.strides[0]))
    F = N_FFT // 2 + 1
    if xp is np:
        spec = frames @ basis.T
        mel = (spec[:, :F] ** 2 + spec[:, F:] ** 2) @ melb.T
        return np.stack([mel[s] for s in mel_sl])
    spec = xp.from_numpy(np.ascontiguousarray(frames)) @ basis.T
    mel = (spec[:, :F] ** 2 + spec[:, F:] ** 2) @ melb.T
    return xp.stack([mel[s] for s in mel_sl])


def leg(name, a):
    from meta_tts_amd import evaluation as E
    from meta_tts_amd.audio.stft import forward_basis, mel_filterbank
    from meta_tts_amd.speaker_encoder import DVectorEncoder, synthetic_state_dict
    wavs = corpus(a.cpu_utts if name == "cpu" else a.utts)
    sd = synthetic_state_dict(0)
    basis, melb = forward_basis(N_FFT, N_FFT, "hann"), mel_filterbank(SR, N_FFT, N_MEL)
    if name == "cpu":
        import torch
        from oracle import dvector_oracle
        torch.set_num_threads(16)
        lstm, linear = dvector_oracle.build(sd)
        tb, tm = torch.from_numpy(basis), torch.from_numpy(melb)

        def call():
            out = []
            with torch.no_grad():
                for w in wavs:
                    _, (hidden, _) = lstm(host_slices(w, tb, tm, E.compute_partial_slices, torch))
                    raw = torch.relu(linear(hidden[-1]))
                    m = (raw / torch.norm(raw, dim=1, keepdim=True)).mean(dim=0)
                    out.append((m / torch.norm(m, 2)).numpy())
            return np.stack(out)
    else:
        import torch
        assert torch.cuda.is_available(), "the device legs need an MI355X"
        if name == "today":
            enc = DVectorEncoder(sd, max_partials=64, max_utts=1)

            def call():
                out = []
                for w in wavs:
                    st = host_slices(w, basis, melb, E.compute_partial_slices)
                    out.append(enc.embed(st, [slice(0, len(st))])[0])
                return np.stack(out)
        else:
            emb = E.SpeakerEmbedder(sd, max_partials=a.max_partials, max_utts=a.max_partials)
            call = lambda: emb.embed_utterances(wavs)   # noqa: E731
            if name != "new":
                i16 = [np.trunc(w * np.float32(32768)).astype(np.int16) for w in wavs]
                call = lambda: emb.embed_pcm16(i16)   # noqa: E731
            if name == "device":
                lengths = np.asarray([len(w) for w in i16], np.int32)
                rows = np.zeros((len(i16), int(lengths.max())), np.float32)
                for r, w in zip(rows, i16):
                    r[: len(w)] = w.astype(np.float32) / np.float32(32768)
                dev = torch.from_numpy(rows).cuda()
                torch.cuda.synchronize()
                call = lambda: emb.embed_device(dev.data_ptr(), rows.shape[1], lengths)   # noqa: E731
    warmup, reps = (1, min(a.reps, 3)) if name == "cpu" else (a.warmup, a.reps)
    for _ in range(warmup):
        vec = call()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        vec = call()
        times.append(time.perf_counter() - t0)
    s = float(np.median(times))
    audio = sum(len(w) for w in wavs) / SR
    partials = sum(len(E.compute_partial_slices(len(w))[1]) for w in wavs)
    return {"utts": len(wavs), "partials": partials, "audio_s": round(audio, 1), "ms_per_call": round(s * 1e3, 2), "ms_min": round(min(times) * 1e3, 2),
            "ms_max": round(max(times) * 1e3, 2), "utterances_per_s": round(len(wavs) / s, 1), "audio_s_per_s": round(audio / s, 1),
            "dvector_checksum": float(np.abs(vec[: min(len(vec), 32)]).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=624)
    ap.add_argument("--cpu-utts", type=int, default=32)
    ap.add_argument("--max-partials", type=int, default=2048)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--leg", default="all", choices=["all", "new", "pcm16", "device", "today", "cpu"])
    ap.add_argument("--legs", default="new,pcm16,device,today,cpu", help="with --leg all: the legs to run, merged into the file at --out when it holds the same set-up")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "speaker_eval_bench.json"))
    a = ap.parse_args()
    if a.leg != "all":
        print(json.dumps(leg(a.leg, a)))
        return
    res = {"utts": a.utts, "cpu_utts": a.cpu_utts, "max_partials": a.max_partials, "warmup": a.warmup, "reps": a.reps,
           "config": "16 kHz, 3-10 s utterances, n_fft 400 / hop 160 / 40 mels, LSTM(40, 256, 3) + Linear(256, 256), synthetic weights"}
    legs = a.legs.split(",")
    if os.path.exists(a.out):
        with open(a.out) as f:
            old = json.load(f)
        if all(old.get(k) == v for k, v in res.items()):
            res = old
    for name in legs:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--utts", str(a.utts), "--cpu-utts", str(a.cpu_utts), "--max-partials",
                            str(a.max_partials), "--warmup", str(a.warmup), "--reps", str(a.reps)], capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"leg {name} failed with status {r.returncode}: nothing further is started")
        res[name] = json.loads(r.stdout.strip().splitlines()[-1])
    for other in ("today", "cpu"):
        if "new" in res and other in res:
            res[f"speedup_vs_{other}"] = round(res["new"]["utterances_per_s"] / res[other]["utterances_per_s"], 2)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
