"""The GEMM launcher's decisions (meta_tts_amd/csrc/gemm_launch.h: the plan step) at the workload's deciding launch shapes, on a CPU: solo or
multi at the 768-workgroup line, the batch regime's split factors and their caps and budgets, task-per-XCD schedule / panel order / grouped
order, BK 16 / 32 and the K-loop variant, the flush at six problems, dual-source problems and forced families, the bf16 mode's 128-tile
threshold and the plane-only / rest cut, the row-complete LayerNorm epilogue, and every refusal with its message.

tests/gemm_plan_cases.cpp is a stand-alone program (host compiler, -DMTTS_EMU, no device, nothing loaded into Python): it calls the planner
on null operand pointers and prints one line per plan — the kernel symbol the plan's identity stands for (read off a stand-in for
MTTS_LAUNCH, so the identity -> kernel table is checked too), the grid, and per problem split factor, placement and start slot.

The expected lines were NOT written by hand and not taken from the planner: tests/golden/gemm_plan*.txt were recorded from the launcher this
one replaced (commit 1ae6838, whose gemm.h had no plan step), by compiling the same program with -DGEMM_PLAN_RECORD_PARENT against that
commit's meta_tts_amd/csrc — the cases then go through its gemm_launch / gemm_batch_begin / gemm_batch_end and the lines are read off the
stand-in's arguments (kernel, grid, GemmArgs::splitk, GemmMulti::start / xcd_group, GemmCtx::last_place / last_kind / error).  One
recording per environment below."""
from __future__ import annotations

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_cases")
    emu = os.path.join(ROOT, "tests", "emu")
    cmd = [HOST_CLANG if os.path.exists(HOST_CLANG) else "clang++", "-O0", "-std=c++17", "-DMTTS_EMU", "-Wno-unused-value", "-Wno-unused-result",
           "-x", "c++", "-I" + emu, "-I" + os.path.join(ROOT, "meta_tts_amd", "csrc"),
           os.path.join(ROOT, "tests", "gemm_plan_cases.cpp"), os.path.join(emu, "hip_emu.cpp"), "-o", exe, "-lpthread"]
    subprocess.run(cmd, check=True, cwd=ROOT)
    return exe


@pytest.mark.parametrize("fixture,env", [
    ("gemm_plan.txt", {}),
    ("gemm_plan_min_groups2.txt", {"MTTS_XCD_SCHED_MIN_GROUPS": "2"}),   # the task-per-XCD schedule for 4 and 2 groups too
    ("gemm_plan_kloop1.txt", {"MTTS_KLOOP": "1"}),                       # the KL = 1 kernels (BK = 32) and KL = 0 (BK = 16)
])
def test_plans_are_the_replaced_launchers(program, fixture, env):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("MTTS_")}
    out = subprocess.run([program], check=True, capture_output=True, text=True, env={**clean, **env}).stdout.splitlines()
    with open(os.path.join(ROOT, "tests", "golden", fixture), encoding="utf-8") as f:
        want = f.read().splitlines()
    assert len(want) > 140
    diff = [(i, w, g) for i, (w, g) in enumerate(zip(want, out)) if w != g]
    assert not diff and len(out) == len(want), (len(want), len(out), diff[:5])
