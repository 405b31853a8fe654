"""A kernel defined in meta_tts_amd/csrc/rowops.h, tangent.h or dvector.h is launched from exactly ONE place in csrc/: its inline host launcher
(launch_*) next to the kernel.  The engine and the raw C entries of kernel_api.inc both go through that launcher, so the float64 pins of
test_kernel_entries.py / test_tangent_entries.py / test_dvector_kernels.py hold for the launch the product uses.  Source-level, CPU only."""
from __future__ import annotations

import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "meta_tts_amd", "csrc")
KERNEL = re.compile(r"__global__\s+(?:__launch_bounds__\(\d+\)\s+)?void\s+(\w+)\s*\(")
LAUNCH = re.compile(r"MTTS_LAUNCH(?:_LN)?\s*\(\s*\(?\s*(\w+)")
NEVER_LAUNCHED = "copy_rows_kernel"   # no launch site in csrc/ at all

def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def test_one_launch_site_per_row_kernel():
    kernels = [k for h in ("rowops.h", "tangent.h", "dvector.h") for k in KERNEL.findall(_read(os.path.join(CSRC, h)))]
    assert len(kernels) > 70 and {"lstm_recurrent_kernel", "lstm_bptt_kernel", "dvec_head_kernel", "dvec_head_bwd_kernel", "dvec_utterance_kernel",
                                  "dvec_utterance_bwd_kernel", "loss_partial_kernel", "loss_final_kernel", "duration_round_kernel",
                                  "sumsq_final_kernel"} <= set(kernels) and len(set(kernels)) == len(kernels), kernels
    sites = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        for name in LAUNCH.findall(_read(path)):
            sites.setdefault(name, []).append(os.path.basename(path))
    wrong = {k: sites.get(k, []) for k in kernels if len(sites.get(k, [])) != 1 and k != NEVER_LAUNCHED}
    assert not wrong, f"kernels without exactly one launch site: {wrong}"
    assert NEVER_LAUNCHED in kernels and NEVER_LAUNCHED not in sites   # (a kernel nobody launches has no launcher either)
    # the four kernels the engine used to launch itself: their one site is the launcher in rowops.h
    for k in ("loss_partial_kernel", "loss_final_kernel", "duration_round_kernel", "sumsq_final_kernel"):
        assert sites[k] == ["rowops.h"], (k, sites[k])
