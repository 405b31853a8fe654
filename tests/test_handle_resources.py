"""Who owns what on the device (csrc/devres.h): every handle of include/mtts.h gives back exactly what it took.

The emulator build keeps a ledger of live allocations, bytes, streams and events, counts frees of pointers that are not live, and can
make the n-th allocation from now fail (tests/emu/hip_emu.h: emu_*).  Two kinds of test on tiny configurations:

  * round trip — create, exercise, destroy each of the four handle kinds: the ledger returns to where it was, no bad free;
  * failure sweep — for every allocation n of a create (and of every later allocating call) the call is repeated with allocation n
    failing: a create must return non-zero with a message and leave the ledger at baseline; a later call must leave a handle that
    destroys cleanly.  Nothing is skipped: n runs over every allocation the successful call makes.

`exercise_*` return what the calls computed, so the same flows serve as the bit-identity capture of a refactor (run them against two
builds of the emulator library and compare with np.array_equal)."""
import ctypes as C
import math

import numpy as np
import pytest

import __graft_entry__ as ge
from oracle_util import synth, tiny_dims
from meta_tts_amd import _lib
from meta_tts_amd import speaker_encoder as se
from meta_tts_amd import vocoder as V
from meta_tts_amd.audio.stft import TacotronSTFT, inverse_basis
from meta_tts_amd.engine import Engine

MODS = ["speaker_emb", "variance_adaptor", "decoder", "mel_linear", "postnet"]
ENG_CAPS = dict(max_tasks=2, max_B=3, max_S=16, max_T=96)
DV_CFG = dict(n_mels=8, hidden=64, emb=64, layers=2)
VOC_CFG = dict(n_mel=16, ngf=16, n_res=2, ratios=(4, 2))
STFT_CFG = dict(filter_length=64, hop_length=16, n_mel=8)


@pytest.fixture(scope="module")
def emu_lib():
    return ge.build_emulator()


class Ledger:
    def __init__(self, path):
        self.lib = _lib.load(path)
        for n in ("emu_live_allocs", "emu_live_bytes", "emu_live_streams", "emu_live_events", "emu_bad_frees", "emu_alloc_calls"):
            getattr(self.lib, n).restype = C.c_longlong
            getattr(self.lib, n).argtypes = []
        self.lib.emu_fail_alloc_after.restype = None
        self.lib.emu_fail_alloc_after.argtypes = [C.c_longlong]

    def live(self):
        return (self.lib.emu_live_allocs(), self.lib.emu_live_bytes(), self.lib.emu_live_streams(), self.lib.emu_live_events())

    def bad(self):
        return self.lib.emu_bad_frees()

    def calls(self):
        return self.lib.emu_alloc_calls()

    def fail_after(self, n):
        self.lib.emu_fail_alloc_after(n)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- the flows ---------------------------------------------------------------------------------------------------------------------
def _engine(lib_path):
    dims = tiny_dims()
    eng = Engine(dims, adapt_modules=MODS, lib_path=lib_path, **ENG_CAPS)
    eng.load_params(synth.make_params(dims, 0))
    kw = dict(n_mel=dims.n_mel, vocab=dims.vocab, s_range=(5, 13), d_range=(1, 6), first_len=12)
    sup = [synth.make_batch(31 + 2 * j, 3, speaker=2 + j, **kw) for j in range(2)]
    qry = [synth.make_batch(32 + 2 * j, 2, speaker=2 + j, **kw) for j in range(2)]
    eng.set_dropout(True, 77)
    eng.set_batches(0, sup)
    eng.set_batches(1, qry, spk_from=sup, average_spk=True)
    return eng


def exercise_engine(lib_path):
    out = {}
    eng = _engine(lib_path)
    eng.forward(0, use_fast=False, train=True)
    out["mel_post"] = eng.outputs(0, 0)["mel_post"].copy()
    q, s = eng.meta_grad(2, 1e-3, 0.5)
    out["fo.q"], out["fo.s"] = q.copy(), s.copy()
    for n in eng.params:
        out["fo." + n] = eng.export(n, 1).copy()
    eng.reserve_second_order(2)
    q, s = eng.meta_grad(2, 1e-3, 0.5, second_order=True)
    out["so.q"], out["so.s"] = q.copy(), s.copy()
    for n in eng.params:
        out["so." + n] = eng.export(n, 1).copy()
    eng.reserve_second_order(3)          # another step count: the fast-weight history is reserved again
    q, _ = eng.meta_grad(3, 1e-3, 0.5, second_order=True)
    out["so3.q"] = q.copy()
    eng.set_numerics("bf16")             # operand planes + weight shadows
    eng.forward(0, use_fast=False, train=True)
    out["bf16.mel_post"] = eng.outputs(0, 0)["mel_post"].copy()
    eng.set_numerics("fp32")
    eng.set_inner_prox(1.0)
    eng.adapt(1, 0.02, fetch_losses=False)
    out["imaml.q"] = eng.imaml_begin().copy()
    eng.imaml_cg_step(0.02, 1.0)
    out["imaml.norms"] = eng.imaml_finish(0.02, 1.0, grad_scale=0.5, max_norm=0.0).copy()
    out["imaml.mel_linear"] = eng.export("mel_linear.weight", 1).copy()
    eng.set_inner_prox(0.0)
    eng.synchronize()
    eng.close()
    return out


def exercise_overlap_counters(lib_path):
    """the overlapped-exchange flow of tests/test_allreduce_overlap_emu.py: how many collectives / inner-update launches it issued"""
    eng = _engine(lib_path)
    eng.comm_init(eng.comm_unique_id(), 0, 2)
    out = {}
    for kind in ("fo", "so"):
        assert eng.arm_allreduce_overlap()
        eng.meta_grad(2, 1e-3, 0.5, second_order=(kind == "so"), fetch_losses=False)
        eng.allreduce_outer()
        eng.synchronize()
        out[kind] = (eng.allreduce_launches, eng.inner_update_launches)
    eng.close()
    return out


def _dv_case(seed, n_utts, frames, n_mels):
    g = np.random.RandomState(seed)
    counts = g.randint(1, 4, size=n_utts)
    mels = g.standard_normal((int(counts.sum()), frames, n_mels)).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(counts)])
    return mels, [slice(int(off[i]), int(off[i + 1])) for i in range(n_utts)]


def _score(lib, h, n_vec, dim, seed):
    g = np.random.RandomState(seed)
    a = g.standard_normal((n_vec, dim)).astype(np.float32)
    b = g.standard_normal((n_vec, dim)).astype(np.float32)
    ia = np.arange(n_vec, dtype=np.int32)
    ib = ia[::-1].copy()
    sim = np.empty(n_vec, np.float32)
    rc1 = lib.mtts_dvector_cosine_indexed(h, _ptr(a), n_vec, _ptr(b), n_vec, dim, n_vec, _ptr(ia), _ptr(ib), 1e-6, _ptr(sim))
    off = np.array([0, n_vec // 2, n_vec], np.int32)
    cen = np.empty((2, dim), np.float32)
    rc2 = lib.mtts_dvector_centroids(h, _ptr(a), _ptr(off), 2, dim, _ptr(cen))
    return rc1, rc2, sim, cen


def exercise_dvector(lib_path):
    out = {}
    enc = se.DVectorEncoder(se.synthetic_state_dict(3, **DV_CFG), max_partials=64, max_utts=16, frames=7, lib_path=lib_path, **DV_CFG)
    mels, slices = _dv_case(4, 3, 7, DV_CFG["n_mels"])
    out["embed"], out["partials"] = [x.copy() for x in enc.embed(mels, slices, return_partials=True)]
    enc.enable_training()
    e = enc.embed_train(mels, slices)
    out["embed_train"] = e.copy()
    enc.backward(np.ones_like(e))
    out["grad.linear.weight"] = enc.export("linear.weight", 1).copy()
    for n_vec in (6, 4000):              # the scoring workspace, then every buffer of it grown
        rc1, rc2, sim, cen = _score(enc.lib, enc.h, n_vec, 16, 9)
        assert rc1 == 0 and rc2 == 0, enc.lib.mtts_dvector_last_error(enc.h)
        out[f"sim{n_vec}"], out[f"cen{n_vec}"] = sim, cen
    enc.close()
    return out


def _stft_calls(t, n, seed):
    """one call each of mel, Griffin-Lim (loads the inverse basis on first use), mel_batch, power_mel_batch on waveforms of ~n samples"""
    g = np.random.RandomState(seed)
    lib, h, hop, n_mel = t.lib, t.h, t.hop_length, t.n_mel_channels
    out = {}
    y = (0.5 * g.standard_normal((1, n))).clip(-1, 1).astype(np.float32)
    out["mel"], out["energy"] = t.mel_spectrogram(y)
    mag, ph = t.stft_fn.transform(y)
    out["gl"] = t.stft_fn.griffin_lim_with_angles(mag, ph, 2)
    ns = np.array([n, n - 3 * hop], np.int32)
    wavs = (0.5 * g.standard_normal(int(ns.sum()))).clip(-1, 1).astype(np.float32)
    keep = np.full(2, -1, np.int32)
    T = int((ns // hop + 1).sum())
    mel, energy, pmel = np.empty((T, n_mel), np.float32), np.empty(T, np.float32), np.empty((T, n_mel), np.float32)
    t._check(lib.mtts_stft_mel_batch(h, 2, _ptr(ns), _ptr(keep), _ptr(wavs), _ptr(mel), _ptr(energy)))
    t._check(lib.mtts_stft_power_mel_batch(h, 2, _ptr(ns), _ptr(wavs), _ptr(pmel)))
    out["mel_batch"], out["energy_batch"], out["power_mel"] = mel, energy, pmel
    return out


def _tacotron(lib_path):
    return TacotronSTFT(STFT_CFG["filter_length"], STFT_CFG["hop_length"], STFT_CFG["filter_length"], STFT_CFG["n_mel"], 16000, 0.0, 8000.0,
                        max_samples=1 << 20, lib_path=lib_path)


def exercise_stft(lib_path):
    t = _tacotron(lib_path)
    out = {"small." + k: v for k, v in _stft_calls(t, 400, 1).items()}
    out.update({"large." + k: v for k, v in _stft_calls(t, 4000, 2).items()})   # every DevBuf grows
    t.close()
    return out


def exercise_vocoder(lib_path):
    sd = V.synthetic_state_dict(5, **VOC_CFG)
    voc = V.MelGAN(sd, max_B=2, max_T=24, lib_path=lib_path, **VOC_CFG)
    g = np.random.RandomState(1)
    mel = (g.standard_normal((2, 16, 20)) * 1.5 - 4.0).astype(np.float32)
    wav = voc.mel2wav(mel, np.array([20, 13], np.int32), mel_scale=1.0 / math.log(10.0))
    voc.close()
    return {"wav": wav}


EXERCISES = {"engine": exercise_engine, "dvector": exercise_dvector, "stft": exercise_stft, "vocoder": exercise_vocoder}


@pytest.mark.parametrize("kind", sorted(EXERCISES))
def test_round_trip_returns_everything(emu_lib, kind):
    led = Ledger(emu_lib)
    base, bad = led.live(), led.bad()
    out = EXERCISES[kind](emu_lib)
    assert out and all(np.all(np.isfinite(v)) for v in out.values())
    assert led.live() == base, (kind, base, led.live())
    assert led.bad() == bad == 0


# ---- failure sweeps ----------------------------------------------------------------------------------------------------------------
def _creates(lib):
    """name -> (create() -> (rc, handle), destroy(handle), last_error(handle or None))"""
    ratios = (C.c_int * 2)(*VOC_CFG["ratios"])

    def mk(fn, *args):
        def create():
            h = C.c_void_p()
            rc = fn(*args, C.byref(h))
            return rc, h
        return create

    return {
        "mtts_vocoder_create": (mk(lib.mtts_vocoder_create, VOC_CFG["n_mel"], VOC_CFG["ngf"], VOC_CFG["n_res"], ratios, 2, 0, 2, 24),
                                lib.mtts_vocoder_destroy, lib.mtts_vocoder_last_error),
        "mtts_dvector_create": (mk(lib.mtts_dvector_create, DV_CFG["n_mels"], DV_CFG["hidden"], DV_CFG["layers"], DV_CFG["emb"], 64, 7, 16, 0),
                                lib.mtts_dvector_destroy, lib.mtts_dvector_last_error),
        "mtts_stft_create": (mk(lib.mtts_stft_create, STFT_CFG["filter_length"], STFT_CFG["hop_length"], STFT_CFG["n_mel"], 1 << 20, 0),
                             lib.mtts_stft_destroy, lib.mtts_stft_last_error),
    }


def _sweep_create(led, name, create, destroy, last_error):
    base = led.live()
    c0 = led.calls()
    rc, h = create()
    K = led.calls() - c0
    assert rc == 0 and K > 0, (name, rc, K)
    destroy(h)
    assert led.live() == base and led.bad() == 0, (name, "clean create / destroy", base, led.live(), led.bad())
    failures = []
    for n in range(K):
        led.fail_after(n)
        rc, h = create()
        led.fail_after(-1)
        msg = last_error(None)
        if rc == 0:
            destroy(h)
            failures.append((n, "returned 0"))
        elif not msg:
            failures.append((n, "no message"))
        elif led.live() != base:
            failures.append((n, "left %s, baseline %s" % (led.live(), base)))
        elif led.bad():
            failures.append((n, "%d bad frees" % led.bad()))
    assert not failures, (name, K, failures)


@pytest.mark.parametrize("name", ["mtts_vocoder_create", "mtts_dvector_create", "mtts_stft_create"])
def test_failed_create_leaves_nothing(emu_lib, name):
    led = Ledger(emu_lib)
    _sweep_create(led, name, *_creates(led.lib)[name])


def test_failed_engine_create_leaves_nothing(emu_lib):
    """mtts_create through the Python wrapper's own configuration code: the wrapper raises on a non-zero return, with the message"""
    from meta_tts_amd.engine import MttsError
    led = Ledger(emu_lib)

    def create():
        try:
            return 0, Engine(tiny_dims(), adapt_modules=MODS, lib_path=emu_lib, **ENG_CAPS)
        except MttsError:
            return -1, None

    _sweep_create(led, "mtts_create", create, lambda eng: eng.close(), lambda _: led.lib.mtts_last_error(None))


def _sweep_later(led, name, fresh, call, destroy, may_succeed=False):
    """fresh() -> handle object; call(handle) -> rc (negative / non-zero = failure).  With allocation n of the call failing, the handle
    must still destroy cleanly.  may_succeed: the call documents a fallback for some of its allocations and may then return 0."""
    base = led.live()
    h = fresh()
    c0 = led.calls()
    rc = call(h)
    K = led.calls() - c0
    assert rc == 0 and K > 0, (name, rc, K)
    destroy(h)
    assert led.live() == base and led.bad() == 0, (name, "clean run", base, led.live(), led.bad())
    failures, rcs = [], []
    for n in range(K):
        h = fresh()
        led.fail_after(n)
        rc = call(h)
        led.fail_after(-1)
        rcs.append(rc)
        if rc == 0 and not may_succeed:
            failures.append((n, "returned 0"))
        rc2 = call(h)                    # the handle is still usable: the same call, nothing failing, goes through
        if rc2 != 0:
            failures.append((n, "retry returned %d" % rc2))
        destroy(h)
        if led.live() != base:
            failures.append((n, "left %s, baseline %s" % (led.live(), base)))
        if led.bad():
            failures.append((n, "%d bad frees" % led.bad()))
    assert not failures, (name, K, failures)
    return rcs


def _rc(fn):
    """a wrapper call that raises -> -1"""
    def call(h):
        try:
            fn(h)
            return 0
        except Exception:  # noqa: BLE001
            return -1
    return call


def test_failed_engine_reservations_leave_a_clean_handle(emu_lib):
    led = Ledger(emu_lib)
    close = lambda e: e.close()
    fresh = lambda: _engine(emu_lib)
    lib = led.lib
    # mtts_reserve_second_order: the second arena, hv, the fast-weight history are required; the tangent-gradient buffers and the
    # per-step activation / gradient sets are optional (the engine falls back to recomputation) and the call then still returns 0
    rcs = _sweep_later(led, "mtts_reserve_second_order", fresh, lambda e: lib.mtts_reserve_second_order(e.h, 2), close, may_succeed=True)
    assert rcs[0] != 0 and rcs[1] != 0 and any(r != 0 for r in rcs[2:]) and rcs[-1] == 0, rcs   # arena, hv, (optional ...), history; last = an optional set

    def reserved():                      # a second reservation with another step count: the history is given back and taken again
        e = fresh()
        e.reserve_second_order(2)
        return e

    _sweep_later(led, "mtts_reserve_second_order (again)", reserved, lambda e: lib.mtts_reserve_second_order(e.h, 4), close, may_succeed=True)
    _sweep_later(led, "mtts_set_numerics(1)", fresh, lambda e: lib.mtts_set_numerics(e.h, 1), close)

    def imaml(e):
        e.set_inner_prox(1.0)
        e.adapt(1, 0.02, fetch_losses=False)
        e.imaml_begin()

    _sweep_later(led, "mtts_imaml_begin", fresh, _rc(imaml), close, may_succeed=True)


def test_failed_dvector_and_stft_reservations_leave_a_clean_handle(emu_lib):
    led = Ledger(emu_lib)
    lib = led.lib
    close = lambda x: x.close()
    fresh_dv = lambda: se.DVectorEncoder(se.synthetic_state_dict(3, **DV_CFG), max_partials=64, max_utts=16, frames=7, lib_path=emu_lib, **DV_CFG)
    _sweep_later(led, "mtts_dvector_enable_training", fresh_dv, lambda e: lib.mtts_dvector_enable_training(e.h), close)

    def score(e):
        rc1, rc2, _, _ = _score(lib, e.h, 6, 16, 9)
        return rc1 or rc2

    _sweep_later(led, "scoring workspace (grow)", fresh_dv, score, close)

    def load_inverse(t):
        ib = inverse_basis(t.filter_length, t.hop_length, t.win_length, "hann")
        wsq = np.ones(t.filter_length, np.float32)
        return lib.mtts_stft_load_inverse(t.h, _ptr(ib), _ptr(wsq))

    _sweep_later(led, "mtts_stft_load_inverse", lambda: _tacotron(emu_lib), load_inverse, close)
    # every grow of the STFT workspace: first use, and a second, larger call on a handle whose buffers are live
    _sweep_later(led, "STFT workspace (first use)", lambda: _tacotron(emu_lib), _rc(lambda t: _stft_calls(t, 400, 1)), close)

    def warm():
        t = _tacotron(emu_lib)
        _stft_calls(t, 400, 1)
        return t

    _sweep_later(led, "STFT workspace (grow)", warm, _rc(lambda t: _stft_calls(t, 4000, 2)), close)
