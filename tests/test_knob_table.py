"""The library's environment switches live in ONE place, meta_tts_amd/csrc/knobs.h, and the three lists of them agree:
what knobs.h reads, what DESIGN.md section 9 documents, and what the tests / tools / bench.py put into an environment.
Source-level, CPU only."""
from __future__ import annotations

import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "meta_tts_amd", "csrc")
NAME = re.compile(r"MTTS_[A-Z0-9_]+")
POINT_OF_USE = "MTTS_GEMM_DUMP"   # GemmProfiler::report reads it at every report: bench.py sets and clears it inside the running process
# MTTS_* names that are not switches of the library: the emulator's, the tests' / bench.py's own, and compile-time macros
NOT_LIBRARY_PREFIX = ("MTTS_EMU", "MTTS_GOLDEN_", "MTTS_BENCH_", "MTTS_SELFTEST_")
NOT_LIBRARY = {"MTTS_PROBE_LIB", "MTTS_ATTN_DIAG", "MTTS_ABLATE", "MTTS_LAUNCH"}


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _knob_names():
    names = set(re.findall(r'"(MTTS_[A-Z0-9_]+)"', _read(os.path.join(CSRC, "knobs.h"))))
    assert names, "knobs.h reads no switch at all?"
    return names


def test_getenv_only_in_knobs_h():
    outside = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if os.path.basename(path) == "knobs.h":
            continue
        outside += [(os.path.basename(path), line.strip()) for line in _read(path).splitlines() if "getenv(" in line]
    assert len(outside) == 1 and outside[0][0] == "gemm.h" and POINT_OF_USE in outside[0][1], outside
    assert POINT_OF_USE not in _knob_names()


def test_every_switch_a_test_or_tool_sets_is_read():
    files = (glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.py")) +
             glob.glob(os.path.join(ROOT, "tools", "*.sh")) + [os.path.join(ROOT, "bench.py")])
    known = _knob_names() | {POINT_OF_USE}
    unknown = {}
    for path in files:
        for n in set(NAME.findall(_read(path))):
            if n.startswith(NOT_LIBRARY_PREFIX) or n in NOT_LIBRARY or n in known:
                continue
            unknown.setdefault(n, []).append(os.path.relpath(path, ROOT))
    assert not unknown, f"switches the library does not read: {unknown}"


def test_design_table_lists_exactly_the_switches():
    text = _read(os.path.join(ROOT, "DESIGN.md"))
    sec = text[text.index("\n## 9."):text.index("\n## 10.")]
    rows = [line for line in sec.splitlines() if line.startswith("|")]   # (the table; the line on retired switches below it is prose)
    documented = set(NAME.findall(re.sub(r"-DMTTS_[A-Z0-9_]+", "", "\n".join(rows))))
    assert documented == _knob_names() | {POINT_OF_USE, "MTTS_BENCH_KEEP_SITES"}, documented ^ (_knob_names() | {POINT_OF_USE, "MTTS_BENCH_KEEP_SITES"})
