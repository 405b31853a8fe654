"""Helpers of the multi-task kernel-entry tests (test_adaptor_entries.py, test_loss_optim_entries.py): per-task arrays laid out at a task
stride LARGER than a task's extent, sentinels behind every task's rows, and the error bounds the tests assert.

Layout rules (they keep a wrong kernel inside the allocation): every array holds `tasks * stride` elements; a row array's stride covers
`cap = max(rows) + 2` rows plus a gap, so a kernel that ignores a task's row count still writes inside the buffer — onto the sentinel."""
import ctypes as C

import numpy as np

SENT = 777.0          # float sentinel behind a task's rows in outputs
ISENT = -777          # int sentinel (idx_out)
EPS = 2.0 ** -24      # fp32 unit roundoff

ROWSETS = {1: (9,), 3: (9, 1, 6)}   # ragged: a full task, a one-row task, a task that ends inside a 4-row workgroup


def i32(v):
    return (C.c_int * len(v))(*[int(x) for x in v])


def i64(v):
    return (C.c_int64 * len(v))(*[int(x) for x in v])


def ulp32(x):
    """one fp32 ulp at |x| (float64 array in, float64 out)"""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def stride_of(n_elems, gap=8):
    """a task stride > the task's extent, a multiple of 4 elements (float4 loads start aligned)"""
    return ((int(n_elems) + 3) & ~3) + gap


def pack(parts, stride, fill, dtype):
    """parts[t] (any shape) at t * stride of one flat array, `fill` elsewhere"""
    out = np.full(len(parts) * stride, fill, dtype)
    for t, a in enumerate(parts):
        a = np.asarray(a, dtype).ravel()
        assert a.size <= stride
        out[t * stride: t * stride + a.size] = a
    return out


def unpack(flat, stride, shapes):
    """(per-task arrays of the given shapes, everything else as one flat array)"""
    flat = np.asarray(flat)
    rest = np.ones(flat.size, bool)
    parts = []
    for t, sh in enumerate(shapes):
        n = int(np.prod(sh))
        parts.append(flat[t * stride: t * stride + n].reshape(sh).copy())
        rest[t * stride: t * stride + n] = False
    return parts, flat[rest]


def sum_bound(n, abs_terms_sum, result):
    """|got - ref64| of an fp32 reduction of n terms: n * 2^-24 * sum|terms| + one fp32 ulp of the result"""
    return n * EPS * np.asarray(abs_terms_sum, np.float64) + ulp32(result)


def assert_within(got, ref, bound, what=""):
    err = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    bad = ~(err <= bound)      # (a NaN is a failure)
    assert not bad.any(), (what, float(err[bad].max()), float(np.asarray(bound)[bad].min() if np.ndim(bound) else bound), int(bad.sum()))


def arbiter_ok(kernel, torch32, ref64, what=""):
    """The project's arbiter rule: err(kernel, f64) <= 3 * err(torch fp32 of the same formula, f64) + one fp32 ulp of the reference value.
    err of the fp32 party = its largest element error; the ulp is taken element by element.  Returns the ratio
    max(err_kernel - ulp, 0) / err_torch for the record (inf when torch is exact and the kernel is not within an ulp)."""
    ref64 = np.asarray(ref64, np.float64)
    ek = np.abs(np.asarray(kernel, np.float64) - ref64)
    et = float(np.abs(np.asarray(torch32, np.float64) - ref64).max())
    over = float(np.maximum(ek - ulp32(ref64), 0).max())
    ratio = 0.0 if over == 0 else (over / et if et > 0 else float("inf"))
    print(f"arbiter {what}: err_kernel {float(ek.max()):.3e} err_torch32 {et:.3e} ratio {ratio:.3f}")
    assert over <= 3 * et, (what, float(ek.max()), et, ratio)
    return ratio
