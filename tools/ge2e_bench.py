"""Time one GE2E train_step (meta_tts_amd/ge2e.py) at the published batch: 64 speakers x 10 utterances x 160 frames, LSTM(40, 256, 3).

    python tools/ge2e_bench.py                      # legs host, device and oracle -> profiles/ge2e_bench.json
    python tools/ge2e_bench.py --leg device         # one leg only, nothing written (what a kernel trace wraps)

Legs: "host" — mels in host memory (the step uploads them); "device" — mels already in device memory; "oracle" — the same step by
tests/ge2e_oracle.py in float32 torch on 16 host threads, the only comparison.  Median of 7 calls after 2 warm-up calls; every call ends
with the loss on the host, so a call is a whole step.  Synthetic weights and random mels: the time does not depend on the values."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, M, FRAMES, CALLS, WARMUP = 64, 10, 160, 7, 2
CFG = dict(n_mels=40, hidden=256, layers=3, emb=256)


def _time(fn):
    for _ in range(WARMUP):
        fn()
    ms = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return dict(ms_median=round(float(np.median(ms)), 3), ms_spread=round(max(ms) - min(ms), 3), ms_all=[round(x, 3) for x in ms])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["host", "device", "oracle", "all"], default="all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ge2e_bench.json"))
    args = ap.parse_args()
    import torch
    from meta_tts_amd import speaker_encoder as se
    from meta_tts_amd.ge2e import GE2ETrainer
    mels = np.random.RandomState(0).standard_normal((N * M, FRAMES, CFG["n_mels"])).astype(np.float32)
    sd = se.synthetic_state_dict(0, **CFG)
    res = {}
    if args.leg in ("host", "device", "all"):
        enc = se.DVectorEncoder(sd, max_partials=N * M, max_utts=N * M, frames=FRAMES, **CFG)
        tr = GE2ETrainer(enc, N, M)
        if args.leg in ("host", "all"):
            res["host"] = _time(lambda: tr.train_step(mels))
        if args.leg in ("device", "all"):
            t = torch.from_numpy(mels).cuda()
            torch.cuda.synchronize()

            def step():
                tr.forward_backward_device(t.data_ptr(), return_loss=True)
                tr.step()
            res["device"] = _time(step)
        res["loss_after"] = tr.forward_backward(mels)
        enc.close()
    if args.leg in ("oracle", "all"):
        import ge2e_oracle as GO
        torch.set_num_threads(16)
        host = GO.Trainer(sd, CFG, N, M, dtype=torch.float32)
        res["oracle"] = dict(_time(lambda: host.train_step(mels)), threads=16, dtype="float32")
    print(json.dumps(res))
    if args.leg == "all":
        out = dict(method=f"median of {CALLS} calls after {WARMUP} warm-up calls; one call = one train_step of {N} speakers x {M} utterances x {FRAMES} frames, "
                          f"LSTM(40, 256, 3), ending with the loss on the host; spread = max - min", **res)
        out["kernel_trace"] = "not measured"
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
