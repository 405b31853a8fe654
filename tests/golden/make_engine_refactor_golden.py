#!/usr/bin/env python3
"""Bit-level fixtures of the engine's host orchestration, recorded on the CPU emulator build.

The fixtures in engine_refactor_bits.npz were recorded from commit 17488bb ("fp32 GEMM launcher: a pure launch plan, then one
issue step"), the parent of the commit that gave Plan its RowSpace / AttnSide records and the convolutions their ConvOp.  They pin
what the emulator build computes for four cases — tiny dims, two ragged tasks, max_B=3, max_S=16, max_T=96, dropout on with a fixed
seed — so that a host-side refactor of csrc/engine.h (+ engine_so.inc, engine_imaml.inc) can be checked to the bit:

  train     train-mode forward + loss + backward
  fo        2-step first-order meta_grad
  so        2-step second-order meta_grad
  frame     forward + loss + backward with a frame-level pitch feature

Per case: the losses, mel_post of every task, every exported per-task parameter gradient and (meta_grad) the outer gradient.  The
emulator's GEMMs and reductions are deterministic for identical launch arguments (two recordings of one build are equal; the test
checks that too), so tests/test_engine_refactor_bits.py compares with assert_array_equal.  Large tensors are stored as a strided
sample plus the CRC-32 of all their bytes: the sample says where a difference is, the checksum that there is none anywhere.

Re-record only from a commit whose numbers are meant to become the new reference:
    python tests/golden/make_engine_refactor_golden.py            (writes engine_refactor_bits.npz)
    python tests/golden/make_engine_refactor_golden.py --check    (records twice, compares: the determinism the test rests on)
    python tests/golden/make_engine_refactor_golden.py --lib PATH --out PATH --gemm-dump CSV
--gemm-dump also writes the launcher's per-launch records (MTTS_GEMM_DUMP) of the four cases, for comparing launch sequences.
"""
import argparse
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for q in (ROOT, os.path.join(ROOT, "tests")):
    if q not in sys.path:
        sys.path.insert(0, q)

from meta_tts_amd import synth  # noqa: E402
from meta_tts_amd.engine import Engine  # noqa: E402
from oracle_util import tiny_dims  # noqa: E402

FIXTURE = os.path.join(HERE, "engine_refactor_bits.npz")
MODS = ["speaker_emb", "variance_adaptor", "decoder", "mel_linear", "postnet"]
SEED = 7
SAMPLE = 64       # values kept of a tensor larger than this (evenly strided)


def _put(out, key, a):
    assert np.asarray(a).dtype == np.float32, (key, np.asarray(a).dtype)
    flat = np.ascontiguousarray(a).reshape(-1)
    out[key] = flat if flat.size <= SAMPLE else flat[:: flat.size // SAMPLE][:SAMPLE].copy()
    out[key + "/crc"] = _crc(flat)


def _crc(flat):
    """(CRC-32 of all bytes, element count) as two float32-exact halves each: every entry of a recording is a float32 array."""
    c = zlib.crc32(flat.tobytes())
    return np.array([c >> 16, c & 0xFFFF, flat.size >> 16, flat.size & 0xFFFF], np.float32)


def pack(rec):
    """One file of three arrays instead of two thousand: names, offsets into one float32 vector."""
    names = sorted(rec)
    offs = np.cumsum([0] + [rec[n].size for n in names]).astype(np.int64)
    return {"names": np.array(names), "offsets": offs, "values": np.concatenate([rec[n] for n in names])}


def unpack(z):
    offs = z["offsets"]
    return {str(n): z["values"][offs[i]:offs[i + 1]] for i, n in enumerate(z["names"])}


def _engine(dims, lib):
    eng = Engine(dims, adapt_modules=MODS, max_tasks=2, max_B=3, max_S=16, max_T=96, lib_path=lib)
    eng.load_params(synth.make_params(dims, 0))
    eng.set_dropout(True, SEED)
    return eng


def _batches(dims, seeds, sizes, **kw):
    kw = dict(n_mel=dims.n_mel, vocab=dims.vocab, s_range=(5, 13), d_range=(1, 6), first_len=12, **kw)
    return [synth.make_batch(s, n, speaker=2 + 3 * j, **kw) for j, (s, n) in enumerate(zip(seeds, sizes))]


def _pass_case(out, tag, eng, dims, **kw):
    eng.set_batches(0, _batches(dims, (3, 4), (3, 2), **kw))
    eng.forward(0, use_fast=False, train=True)
    _put(out, tag + "/losses", eng.loss(0))
    eng.backward(0, use_fast=False, scale=1.0, need_encoder=True)
    for t in range(2):
        _put(out, f"{tag}/mel_post/{t}", eng.outputs(0, t)["mel_post"])
        for n in eng.params:
            _put(out, f"{tag}/grad/{t}/{n}", eng.export(n, 2, t))


def _meta_case(out, tag, eng, dims, second_order):
    sup, qry = _batches(dims, (10, 12), (3, 3)), _batches(dims, (11, 13), (2, 2))
    eng.set_batches(0, sup)
    eng.set_batches(1, qry, spk_from=sup, average_spk=True)
    q, s = eng.meta_grad(2, 0.01, 0.5, second_order=second_order)
    _put(out, tag + "/losses", q)
    _put(out, tag + "/sup_losses", s)
    for t in range(2):
        _put(out, f"{tag}/mel_post/{t}", eng.outputs(1, t)["mel_post"])
        for n in eng.params:
            _put(out, f"{tag}/grad/{t}/{n}", eng.export(n, 2, t))
    for n in eng.params:
        _put(out, f"{tag}/outer/{n}", eng.export(n, 1))


def record(lib, gemm_dump=None):
    """{key: array} of the four cases on the library at `lib` (an emulator build)."""
    out = {}
    if gemm_dump:
        os.environ["MTTS_GEMM_DUMP"] = gemm_dump
    for tag in ("train", "fo", "so", "frame"):
        dims = tiny_dims(pitch_level="frame_level") if tag == "frame" else tiny_dims()
        eng = _engine(dims, lib)     # a handle per case: the dropout counter and the BatchNorm buffers start the same way whatever ran before
        if gemm_dump:
            eng.profile_gemm(True)
        if tag == "train":
            _pass_case(out, tag, eng, dims)
        elif tag == "frame":
            _pass_case(out, tag, eng, dims, pitch_level="frame_level")
        else:
            _meta_case(out, tag, eng, dims, second_order=(tag == "so"))
        if gemm_dump:
            eng.profile_report()
            eng.profile_gemm(False)
        eng.close()
    if gemm_dump:
        os.environ.pop("MTTS_GEMM_DUMP", None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="emulator library (default: build this tree's)")
    ap.add_argument("--out", default=FIXTURE)
    ap.add_argument("--check", action="store_true", help="record twice and compare instead of writing")
    ap.add_argument("--gemm-dump", default=None)
    a = ap.parse_args()
    lib = a.lib
    if lib is None:
        import __graft_entry__ as ge
        lib = ge.build_emulator()
    res = record(lib, a.gemm_dump)
    if a.check:
        again = record(lib)
        bad = [k for k in res if not np.array_equal(res[k], again[k])]
        print("deterministic" if not bad else "DIFFERENT: %s" % bad[:10], "-", len(res), "arrays")
        sys.exit(1 if bad else 0)
    np.savez_compressed(a.out, **pack(res))
    print("wrote", a.out, os.path.getsize(a.out), "bytes,", len(res), "arrays")


if __name__ == "__main__":
    main()
