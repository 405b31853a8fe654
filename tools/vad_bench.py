#!/usr/bin/env python3
"""Device silence trimming (csrc/vad.h), measured as three legs:
  a        SilenceTrimmer().trim_batch of 64 x 5 s at 16 kHz, host to host;
  b        the evaluation set of tools/speaker_eval_bench.py (624 utterances of 3-10 s, here with pauses) synthesised at 22 050 Hz ->
           d-vectors through the fully chained entry (SpeakerEmbedder.embed_utterances(source_rate=22050, normalize_dbfs=-30, trim=True):
           all of `preprocess_wav` on the device);
  c        the same set through embed_utterances(source_rate=22050, normalize_dbfs=-30) without trimming — the path that existed before —
           on this build and, with --parent-lib, on a libmtts.so built from the parent commit (alternating, two child processes each).
Each leg runs in a child process of its own under a time limit, as the median wall time of 7 calls after 2 warm-up calls; every call
ends in a device synchronise (the entry points are synchronous); a leg that fails ends the run.  Writes profiles/vad_bench.json and
prints it.  The expectation — trimming adds a small fraction to leg c, and c is unchanged against the parent — is reported
(b_over_c, c_this_over_parent), not asserted.  `kernels`: what hipcc reports for the three kernels of the csrc/vad.h in this tree,
gathered at bench time by compiling it at -O3 for gfx950 with -Rpass-analysis=kernel-resource-usage (no GPU involved)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NEW_SYMBOLS = ("mtts_stft_load_vad", "mtts_stft_trim_batch", "mtts_dvector_embed_wavs_preprocessed")   # absent from a parent-commit library


def kernel_resources():
    """{kernel: {vgprs, sgprs, scratch_bytes, lds_bytes}} for the kernels of csrc/vad.h as hipcc compiles them now."""
    import re
    import tempfile
    csrc = os.path.join(ROOT, "meta_tts_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "vad_only.hip")
        with open(src, "w") as f:
            f.write('#include "vad.h"\n')
        r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "-I" + csrc, src, "-o", os.path.join(tmp, "vad_only.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit("hipcc could not compile csrc/vad.h for the resource report:\n" + r.stderr[-2000:])
    fields = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "ScratchSize [bytes/lane]": "scratch_bytes", "LDS Size [bytes/block]": "lds_bytes"}
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            hit = re.search(r"(vad_[a-z]+_kernel)", m.group(1))
            cur = out.setdefault(hit.group(1), {}) if hit else None
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z \[\]/]*): (\d+)", line)
        if m and cur is not None and m.group(1).strip() in fields:
            cur[fields[m.group(1).strip()]] = int(m.group(2))
    if sorted(out) != ["vad_compact_kernel", "vad_energy_kernel", "vad_mask_kernel"] or any(len(v) != 4 for v in out.values()):
        raise SystemExit(f"could not read the resource report of the three kernels: {out}")
    return out


def corpus(utts, sr, seconds=None):
    """tools/speaker_eval_bench.py's durations and tones at `sr`, gated by pauses of faint noise (about 40 % of every utterance)."""
    g = np.random.RandomState(0)
    out = []
    for _ in range(utts):
        n = int(sr * (seconds if seconds else int(16000 * g.uniform(3.0, 10.0)) / 16000))
        t = np.arange(n) / sr
        gate = np.sin(2 * np.pi * g.uniform(0.5, 1.0) * t + g.uniform(0, 6.28)) > -0.3
        out.append((gate * 0.5 * np.sin(2 * np.pi * g.uniform(100, 300) * t + 3 * np.sin(2 * np.pi * 0.7 * t)) + 1e-3 * g.standard_normal(n)).astype(np.float32))
    return out


def leg(name, a):
    import torch
    assert torch.cuda.is_available(), "every leg needs an MI355X"
    from meta_tts_amd import _lib
    from meta_tts_amd import evaluation as E
    from meta_tts_amd.speaker_encoder import synthetic_state_dict
    lib_path = None
    if name == "c_parent":
        lib_path = os.path.abspath(a.parent_lib)
        for s in NEW_SYMBOLS:
            _lib.EXPORTS.pop(s)
    extra = {}
    if name == "a":
        from meta_tts_amd.audio.vad import SilenceTrimmer
        wavs = corpus(64, 16000, seconds=5.0)
        t = SilenceTrimmer()
        call = lambda: t.trim_batch(wavs)   # noqa: E731
        audio = 64 * 5.0
    else:
        emb = E.SpeakerEmbedder(synthetic_state_dict(0), max_partials=a.max_partials, max_utts=a.max_partials, lib_path=lib_path)
        wavs = corpus(a.utts, 22050)
        audio = sum(len(w) for w in wavs) / 22050
        if name == "b":
            call = lambda: emb.embed_utterances(wavs, source_rate=22050, normalize_dbfs=-30.0, trim=True)   # noqa: E731
        else:
            call = lambda: emb.embed_utterances(wavs, source_rate=22050, normalize_dbfs=-30.0)   # noqa: E731
    for _ in range(a.warmup):
        res = call()
    times = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        res = call()
        times.append(time.perf_counter() - t0)
    s = float(np.median(times))
    if name == "a":
        check = float(sum(np.abs(r[:1000]).sum() for r in res[:4]))
        extra = {"samples_in": sum(len(w) for w in wavs), "samples_out": sum(len(r) for r in res)}
    else:
        check = float(np.abs(res[:32]).sum())
        if name == "b":
            extra = {"samples_16k_in": int(sum(-(-len(w) * 320 // 441) for w in wavs)), "samples_16k_kept": int(emb.last_trimmed_lengths.sum())}
    return dict({"utts": len(wavs), "audio_s": round(audio, 1), "ms_per_call": round(s * 1e3, 2), "ms_min": round(min(times) * 1e3, 2),
                 "ms_max": round(max(times) * 1e3, 2), "audio_s_per_s": round(audio / s, 1), "checksum": check}, **extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=624)
    ap.add_argument("--max-partials", type=int, default=2048)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--leg", default="all", choices=["all", "a", "b", "c", "c_parent"])
    ap.add_argument("--parent-lib", default=None, help="a libmtts.so built from the parent commit (leg c's other arm)")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vad_bench.json"))
    a = ap.parse_args()
    if a.leg != "all":
        print(json.dumps(leg(a.leg, a)))
        return
    res = {"utts": a.utts, "max_partials": a.max_partials, "warmup": a.warmup, "reps": a.reps,
           "config": "a: 64 x 5 s at 16 kHz host to host; b / c: 624 utterances of 3-10 s at 22 050 Hz, kaiser_best, LSTM(40, 256, 3), synthetic weights",
           "kernels": kernel_resources()}
    order = ["a", "b"] + (["c", "c_parent", "c", "c_parent"] if a.parent_lib else ["c", "c"])
    for name in order:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--utts", str(a.utts), "--max-partials", str(a.max_partials), "--warmup", str(a.warmup),
               "--reps", str(a.reps)] + (["--parent-lib", a.parent_lib] if a.parent_lib else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"leg {name} failed with status {r.returncode}: nothing further is started")
        res.setdefault(name, []).append(json.loads(r.stdout.strip().splitlines()[-1]))
    for name in ("a", "b"):
        res[name] = res[name][0]
    this = float(np.mean([r["ms_per_call"] for r in res["c"]]))
    res["b_over_c"] = round(res["b"]["ms_per_call"] / this, 4)
    if a.parent_lib:
        parent = float(np.mean([r["ms_per_call"] for r in res["c_parent"]]))
        res["c_this_over_parent"] = round(this / parent, 4)
        res["c_checksums_equal"] = len({r["checksum"] for k in ("c", "c_parent") for r in res[k]}) == 1
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
