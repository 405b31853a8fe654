"""Waveform sources of the d-vector chain (csrc/wavsource.h through include/mtts.h: mtts_dvector_embed_wavs_source;
SpeakerEmbedder.embed_pcm16 / embed_device, WavsToDvector(pcm16=True), MelGAN.infer_device, evaluation.embed_synthesized).
CPU tests run the device code through the SIMT emulator (a "device" pointer is host memory there); the `-m gpu` twins run on the MI355X.

Every tolerance is ZERO, and that is derived, not measured: int16 / 2^15, x * 2^15 and truncation are exact in float32, and behind the
buffer the source fills every launch is the one the host float32 route makes.  So each new route must reproduce an existing route on
the same sample values bit for bit (np.array_equal on vectors, slices, partial counts and trimmed lengths).

Shapes: five utterances of about 0.4 .. 2.5 s, bursts and pauses at about +-20 000 (the trimmer keeps something and removes
something), max_partials = 4 so that they make at least two chunks.  Five ODD lengths cannot be pairwise different modulo 8 (there are
four odd residues): four are odd, 8k + 1 / 3 / 7 / 5, the fifth is 8k + 2, which makes the packed int16 utterances start at the 2-byte
offsets 0, 1, 4, 3, 5 modulo 8.  `_residues` adds nine utterances of 8k + 1 samples, whose packed offsets walk through every residue
0 .. 7; through the resampler the destination (its packed source buffer) takes the same offsets, so head, aligned body, misaligned
body and ragged end of the kernel all run."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
from meta_tts_amd import _lib
from meta_tts_amd import evaluation as E
from meta_tts_amd.engine import MttsError
from meta_tts_amd.speaker_encoder import synthetic_state_dict

TINY = dict(hidden=64, emb=32, layers=2)
CHAINS = [dict(), dict(source_rate=22050, normalize_dbfs=-30.0), dict(source_rate=22050, normalize_dbfs=-30.0, trim=True)]
CHAIN_IDS = ["plain", "resampled", "preprocessed"]


def _emu():
    return ge.build_emulator()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _rate(chain):
    return chain.get("source_rate", 16000)


_CACHE = {}


def _pcm(sr):
    """The five int16 utterances at `sr` (computed once per rate, never written to)."""
    if sr not in _CACHE:
        g, w = np.random.RandomState(5 + sr), sr * 30 // 1000
        out = []
        for secs, r in zip((0.4, 0.9, 1.3, 1.8, 2.5), (1, 3, 7, 2, 5)):
            n = int(secs * sr) // 8 * 8 + r
            env = []
            while len(env) * w < n + w:
                env += [1] * g.randint(8, 26) + [0] * g.randint(12, 21)
            x = np.concatenate([20000.0 * np.sin(2 * np.pi * 200 * np.arange(w) / sr + g.rand()) + 40 * g.standard_normal(w) if lv else 3.0 * g.standard_normal(w)
                                for lv in env])[:n]
            x = np.trunc(x).astype(np.int16)
            x.setflags(write=False)
            out.append(x)
        n = [len(x) for x in out]
        assert all(0.39 * sr <= k <= 2.51 * sr for k in n) and len({k % 8 for k in n}) == 5 and n[0] % 8 == 1 and n[2] % 8 == 7
        assert sorted(int(o) % 8 for o in np.cumsum([0] + n[:-1])) == [0, 1, 3, 4, 5]
        _CACHE[sr] = out
    return _CACHE[sr]


def _residues():
    """Nine utterances of 8k + 1 samples: the packed offsets are 0, 1, .. 7, 0 modulo 8."""
    g = np.random.RandomState(11)
    out = [g.randint(-20000, 20001, size=2400 + 8 * k + 1).astype(np.int16) for k in range(9)]
    assert sorted({int(o) % 8 for o in np.cumsum([0] + [len(x) for x in out[:-1]])}) == list(range(8))
    return out


def _f32(wavs):
    return [w.astype(np.float32) / np.float32(32768) for w in wavs]


def _embedder(lib_path, max_partials=4):
    return E.SpeakerEmbedder(synthetic_state_dict(3, **TINY), lib_path=lib_path, max_partials=max_partials, **TINY)


def _rows(wavs, lib_path, extra=3, fill=np.nan):
    """The float waveforms as rows of one [B][row_stride] array in "device" memory, the padding filled with NaN: (pointer, row_stride,
    lengths, the array that owns the memory).  row_stride is odd, so the rows start at every 4-byte offset modulo 16."""
    n = np.asarray([len(w) for w in wavs], np.int32)
    stride = int(n.max()) + extra
    stride += 1 - stride % 2
    host = np.full((len(wavs), stride), fill, np.float32)
    for i, w in enumerate(wavs):
        host[i, :len(w)] = w
    if lib_path is not None:
        return host.ctypes.data, stride, n, host
    import torch
    dev = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    return dev.data_ptr(), stride, n, dev


def _same(a, b):
    """(vectors, slices) pairs, bit for bit."""
    assert np.array_equal(a[0], b[0]) and len(a[1]) == len(b[1])
    for x, y in zip(a[1], b[1]):
        assert x.shape == y.shape and np.array_equal(x, y)


# ---- 1. embed_pcm16 equals embed_utterances ----------------------------------------------------------------------------------------------
def _check_pcm16(lib_path, chain):
    emb = _embedder(lib_path)
    i16 = _pcm(_rate(chain))
    got = emb.embed_pcm16(i16, return_slices=True, **chain)
    trimmed = emb.last_trimmed_lengths
    emb.last_trimmed_lengths = None
    want = emb.embed_utterances(_f32(i16), return_slices=True, **chain)
    _same(got, want)
    assert sum(len(s) for s in want[1]) > 4                                  # more partials than max_partials: at least two chunks
    assert np.isfinite(got[0]).all() and np.array_equal(emb.embed_pcm16(i16, **chain), got[0])
    if chain.get("trim"):
        n16 = np.asarray([emb.resampler(22050).output_length(len(w)) for w in i16])
        assert np.array_equal(trimmed, emb.last_trimmed_lengths) and np.all(trimmed >= 480) and np.any(trimmed < n16)   # keeps something, removes something
    else:
        assert trimmed is None
    with pytest.raises(TypeError, match="int16"):
        emb.embed_pcm16(_f32(i16))
    emb.close()


@pytest.mark.parametrize("chain", CHAINS, ids=CHAIN_IDS)
def test_pcm16_equals_float_emulator(chain):
    _check_pcm16(_emu(), chain)


@pytest.mark.gpu
@pytest.mark.parametrize("chain", CHAINS, ids=CHAIN_IDS)
def test_pcm16_equals_float_gpu(chain):
    _check_pcm16(None, chain)


def _check_residues(lib_path):
    """Every source residue, as they are (aligned destinations) and through the identity resampler (destinations at the same residues)."""
    emb = _embedder(lib_path, max_partials=5)
    i16 = _residues()
    for chain in (dict(), dict(source_rate=16000), dict(source_rate=16000, trim=True)):
        _same(emb.embed_pcm16(i16, return_slices=True, **chain), emb.embed_utterances(_f32(i16), return_slices=True, **chain))
    ptr, stride, n, keep = _rows(_f32(i16), lib_path)
    for chain in (dict(), dict(source_rate=16000)):
        assert np.array_equal(emb.embed_device(ptr, stride, n, **chain), emb.embed_utterances(_f32(i16), **chain))
    emb.close()


def test_every_residue_emulator():
    _check_residues(_emu())


@pytest.mark.gpu
def test_every_residue_gpu():
    _check_residues(None)


# ---- 2. a device source equals the host source -------------------------------------------------------------------------------------------
def _check_device(lib_path, chain):
    emb = _embedder(lib_path)
    wavs = _f32(_pcm(_rate(chain)))
    ptr, stride, n, keep = _rows(wavs, lib_path)
    got = emb.embed_device(ptr, stride, n, **chain)
    trimmed = emb.last_trimmed_lengths
    assert not np.isnan(got).any()
    assert np.array_equal(got, emb.embed_utterances(wavs, **chain))
    if chain.get("trim"):
        assert np.array_equal(trimmed, emb.last_trimmed_lengths)
    emb.close()


@pytest.mark.parametrize("chain", CHAINS, ids=CHAIN_IDS)
def test_device_equals_host_emulator(chain):
    _check_device(_emu(), chain)


@pytest.mark.gpu
@pytest.mark.parametrize("chain", CHAINS, ids=CHAIN_IDS)
def test_device_equals_host_gpu(chain):
    _check_device(None, chain)


# ---- 3. quantisation -------------------------------------------------------------------------------------------------------------------------
def _check_quantize(lib_path):
    emb = _embedder(lib_path)
    g = np.random.RandomState(9)
    wavs = [np.clip(w * np.float32(1.7) + (g.rand(len(w)).astype(np.float32) - np.float32(0.5)) / np.float32(1000), -0.999, 0.999).astype(np.float32)
            for w in _f32(_pcm(16000))]
    scaled = [w * np.float32(32768) for w in wavs]
    i16 = [np.trunc(s).astype(np.int16) for s in scaled]
    # negative values with a fractional part: truncation towards zero and flooring differ on them
    assert all(np.any((s < 0) & (s != np.trunc(s))) for s in scaled) and all(np.any(np.trunc(s) != np.floor(s)) for s in scaled)
    assert all(np.abs(s).max() < 32768 for s in scaled) and max(np.abs(w).max() for w in wavs) >= np.float32(0.99)
    ptr, stride, n, keep = _rows(wavs, lib_path)
    for chain in (dict(), CHAINS[2]):
        got = emb.embed_device(ptr, stride, n, quantize=32768, **chain)
        assert np.array_equal(got, emb.embed_pcm16(i16, **chain))
    assert not np.array_equal(got, emb.embed_device(ptr, stride, n, **CHAINS[2]))       # (and it is not a no-op)
    emb.close()


def test_quantize_emulator():
    _check_quantize(_emu())


@pytest.mark.gpu
def test_quantize_gpu():
    _check_quantize(None)


# ---- 4. position independence ----------------------------------------------------------------------------------------------------------------
def _check_alone(lib_path):
    emb = _embedder(lib_path)
    for chain in (CHAINS[0], CHAINS[2]):
        i16 = _pcm(_rate(chain))
        batch = emb.embed_pcm16(i16, **chain)
        for i, w in enumerate(i16):
            assert np.array_equal(emb.embed_pcm16([w], **chain)[0], batch[i]), i
        assert np.array_equal(emb.embed_pcm16(i16[::-1], **chain), batch[::-1])
    emb.close()


def test_alone_and_in_the_batch_emulator():
    _check_alone(_emu())


@pytest.mark.gpu
def test_alone_and_in_the_batch_gpu():
    _check_alone(None)


# ---- 5. a producer on another stream ---------------------------------------------------------------------------------------------------------
VOC = dict(n_mel=32, ngf=16, n_res=2, ratios=(8, 4))


@pytest.mark.gpu
def test_vocoder_output_is_embedded_from_its_own_stream():
    import torch
    from meta_tts_amd import vocoder as V
    B, T, lens = 3, 60, np.asarray([60, 41, 53], np.int32)
    voc = V.MelGAN(V.synthetic_state_dict(5, **VOC), max_B=B, max_T=T, **VOC)
    side = torch.cuda.Stream()
    voc.set_stream(side.cuda_stream)
    emb = _embedder(None, max_partials=2)
    g = np.random.RandomState(2)
    mel = (g.standard_normal((B, VOC["n_mel"], T)) * 1.5 - 4.0).astype(np.float32)
    mel_dev = torch.from_numpy(np.ascontiguousarray(mel.transpose(0, 2, 1))).cuda()
    torch.cuda.synchronize()
    chain = dict(source_rate=22050, normalize_dbfs=-30.0)
    wav_ptr, stride, n, stream = voc.infer_device(mel_dev.data_ptr(), 0, B, T, lens)
    got = emb.embed_device(wav_ptr, stride, n, stream=stream, **chain)                  # (nothing waits on the host in between)
    assert stream == side.cuda_stream and stride == T * voc.hop and np.array_equal(n, lens * voc.hop)
    ref = voc.mel2wav(mel, lens, mel_scale=1.0 / np.log(10.0))
    assert np.array_equal(got, emb.embed_utterances([ref[b, :n[b]] for b in range(B)], **chain))
    again = emb.embed_device(*voc.infer_device(mel_dev.data_ptr(), 0, B, T, lens)[:3], stream=stream, quantize=32768, **chain)
    assert np.array_equal(again, emb.embed_pcm16([(ref[b, :n[b]] * 32768).astype("int16") for b in range(B)], **chain))
    voc.close(); emb.close()


@pytest.mark.gpu
def test_embed_synthesized_equals_the_host_route():
    from oracle_util import tiny_dims
    from meta_tts_amd import synth
    from meta_tts_amd import vocoder as V
    from meta_tts_amd.engine import Engine
    dims = tiny_dims()
    b = synth.make_batch(3, 2, speaker=4, n_mel=dims.n_mel, vocab=40, s_range=(10, 20), d_range=(2, 6), first_len=16)
    eng = Engine(dims, adapt_modules=[], max_tasks=1, max_B=2, max_S=20, max_T=int(b[8]))
    eng.load_params(synth.make_params(dims, 0))
    eng.set_batches(0, [b])
    eng.forward(0, train=False)
    lens = np.asarray(b[7], np.int32)
    voc = V.MelGAN(V.synthetic_state_dict(5, **VOC), max_B=2, max_T=int(b[8]), **VOC)
    emb = _embedder(None, max_partials=2)
    chain = dict(source_rate=22050, normalize_dbfs=-30.0, trim=True)
    got = E.embed_synthesized(eng, voc, emb, 0, 0, lens, 32768.0, **chain)
    mel_post = eng.outputs(0, 0)["mel_post"]
    wavs = voc.infer(np.ascontiguousarray(mel_post.transpose(0, 2, 1)), 32768.0, lengths=[int(k) * voc.hop for k in lens])   # int16, as the Saver writes them
    assert all(w.dtype == np.int16 and len(w) == k * voc.hop for w, k in zip(wavs, lens))
    assert np.array_equal(got, emb.embed_pcm16(wavs, **chain)) and np.isfinite(got).all()
    with pytest.raises(ValueError, match="source_rate"):
        E.embed_synthesized(eng, voc, emb, 0, 0, lens, 32768.0)
    voc.close(); emb.close(); eng.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------
def _check_refusals(lib_path):
    emb = _embedder(lib_path)
    lib, name = emb.lib, "mtts_dvector_embed_wavs_source: "
    i16 = _pcm(16000)[:2]
    n, packed = np.asarray([len(w) for w in i16], np.int32), np.ascontiguousarray(np.concatenate(i16))
    ptr, stride, _, keep = _rows(_f32(i16), lib_path)
    vec, cnt, ntr = np.empty((2, emb.emb), np.float32), np.empty(2, np.int32), np.empty(2, np.int32)

    def call(src, stages=0, dbfs=float("nan")):
        return lib.mtts_dvector_embed_wavs_source(emb.encoder.h, emb._dev.h, C.byref(src) if src is not None else None, stages, 2, _ptr(n), 160, emb.frame_step,
                                                  0.75, dbfs, 1, _ptr(vec), _ptr(cnt), None, _ptr(ntr))

    def refused(src, text, **kw):
        assert call(src, **kw) != 0
        both = lib.mtts_stft_last_error(emb._dev.h).decode(), lib.mtts_dvector_last_error(emb.encoder.h).decode()
        assert both[0] == both[1] and both[0].startswith(name) and text in both[0], both

    S = _lib.WavSource
    pcm = lambda **kw: S(**{**dict(kind=S.HOST_PCM16, data=packed.ctypes.data), **kw})          # noqa: E731
    dev = lambda **kw: S(**{**dict(kind=S.DEVICE_F32, data=ptr, row_stride=stride), **kw})      # noqa: E731
    refused(None, "NULL source")
    refused(pcm(data=None), "NULL source data")
    refused(pcm(kind=7), "unknown source kind 7")
    refused(dev(row_stride=int(n.max()) - 1), f"utterance 1: {n[1]} samples exceed row_stride = {n[1] - 1}")
    refused(pcm(quantize_scale=32768.0), "quantize_scale on a host source")
    refused(S(kind=S.HOST_F32, data=ptr, quantize_scale=1.0), "quantize_scale on a host source")
    refused(dev(quantize_scale=-1.0), "negative quantize_scale")
    refused(pcm(), "unknown stages", stages=4)
    emb.trimmer().ensure_loaded()
    refused(pcm(), "volume normalisation needs a resampler", stages=2, dbfs=-30.0)
    # the handle is still usable: the next valid calls succeed and agree with the Python surface
    want = emb.embed_utterances(_f32(i16))
    assert call(pcm()) == 0 and np.array_equal(vec, want)
    assert call(dev()) == 0 and np.array_equal(vec, want)
    f32 = np.ascontiguousarray(np.concatenate(_f32(i16)))
    assert call(S(kind=S.HOST_F32, data=f32.ctypes.data)) == 0 and np.array_equal(vec, want)       # the older entries' form through the new one
    with pytest.raises(MttsError, match="row_stride"):
        emb.embed_device(ptr, 10, n)
    assert np.array_equal(emb.embed_pcm16(i16), want)
    emb.close()


def test_refusals_emulator():
    _check_refusals(_emu())


@pytest.mark.gpu
def test_refusals_gpu():
    _check_refusals(None)


# ---- CPU: the C surface and the files ---------------------------------------------------------------------------------------------------------
def test_symbol_and_ctypes_signature():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "mtts.h")).read()
    decl = re.search(r"int mtts_dvector_embed_wavs_source\(([^;]*)\);", hdr).group(1)
    params = [p.strip() for p in decl.replace("\n", " ").split(",")]
    assert len(params) == 15 and params[2] == "const mtts_wav_source* src" and params[3] == "int stages"
    restype, argtypes = _lib.EXPORTS["mtts_dvector_embed_wavs_source"]
    assert restype is C.c_int and len(argtypes) == 15
    for p, t in zip(params, argtypes):
        assert t is (C.c_void_p if "*" in p else C.c_double if p.startswith("double") else C.c_int), (p, t)
    fields = re.search(r"typedef struct mtts_wav_source \{(.*?)\} mtts_wav_source;", hdr, re.S).group(1)
    names = [f.split()[-1].lstrip("*") for f in fields.split(";") if f.strip()]
    assert names == [f[0] for f in _lib.WavSource._fields_] == ["kind", "data", "row_stride", "producer_stream", "quantize_scale"]
    assert (_lib.WavSource.HOST_F32, _lib.WavSource.HOST_PCM16, _lib.WavSource.DEVICE_F32) == (0, 1, 2)
    for path in (ge.build_emulator(), ge.build_device()):
        assert hasattr(C.CDLL(path), "mtts_dvector_embed_wavs_source"), path


class _Recorder:
    """Stands where a SpeakerEmbedder stands in WavsToDvector.files_to_dvectors: records what each route was given."""
    emb = 4

    def __init__(self):
        self.calls = []

    def embed_pcm16(self, wavs, **kw):
        self.calls.append(("pcm16", [np.array(w) for w in wavs], kw))
        return np.full((len(wavs), self.emb), 16, np.float32)

    def embed_utterances(self, wavs, **kw):
        self.calls.append(("float", [np.array(w) for w in wavs], kw))
        return np.full((len(wavs), self.emb), 32, np.float32)


def test_wav_files_keep_their_16_bits(tmp_path):
    wavfile = pytest.importorskip("scipy.io.wavfile")
    from meta_tts_amd.preprocessor import read_wav
    g = np.random.RandomState(1)
    i16 = g.randint(-20000, 20001, size=801).astype(np.int16)
    f32 = (g.rand(640).astype(np.float32) - np.float32(0.5))
    stereo = g.randint(-20000, 20001, size=(500, 2)).astype(np.int16)
    paths = {k: str(tmp_path / f"{k}.wav") for k in ("i16", "f32", "stereo", "i16_22k")}
    wavfile.write(paths["i16"], 16000, i16)
    wavfile.write(paths["f32"], 16000, f32)
    wavfile.write(paths["stereo"], 16000, stereo)
    wavfile.write(paths["i16_22k"], 22050, i16)
    # what read_wav returns today is unchanged, with and without the new keyword where the file is not mono 16-bit
    w, sr = read_wav(paths["i16"])
    assert sr == 16000 and w.dtype == np.float32 and np.array_equal(w, i16.astype(np.float32) / 32768.0)
    for k, want in (("f32", f32), ("stereo", (stereo.astype(np.float32) / 32768.0).mean(axis=1).astype(np.float32))):
        for keep in (False, True):
            w, sr = read_wav(paths[k], keep_pcm16=keep)
            assert sr == 16000 and w.dtype == np.float32 and np.array_equal(w, want), (k, keep)
    w, sr = read_wav(paths["i16"], keep_pcm16=True)
    assert sr == 16000 and w.dtype == np.int16 and np.array_equal(w, i16)

    def tool(**kw):
        t = E.WavsToDvector.__new__(E.WavsToDvector)                                    # files_to_dvectors alone: no result tree behind it
        t.embedder, t.wav_loader, t.trim = _Recorder(), E.read_wav_16k, False
        t.resample, t.normalize_dbfs, t.pcm16 = kw.get("resample", False), -30.0, kw.get("pcm16", False)
        return t

    t = tool()                                                                                   # default off: everything is float, one call
    out = t.files_to_dvectors([paths["i16"], paths["f32"]])
    assert [c[0] for c in t.embedder.calls] == ["float"] and out.shape == (2, 4)
    assert np.array_equal(t.embedder.calls[0][1][0], i16.astype(np.float32) / 32768.0)
    t = tool(pcm16=True)
    out = t.files_to_dvectors([paths["f32"], paths["i16"], paths["stereo"]])
    calls = {c[0]: c for c in t.embedder.calls}
    assert sorted(calls) == ["float", "pcm16"] and np.array_equal(out[:, 0], [32, 16, 32])
    assert calls["pcm16"][1][0].dtype == np.int16 and np.array_equal(calls["pcm16"][1][0], i16) and calls["pcm16"][2] == dict(trim=False)
    assert [w.dtype for w in calls["float"][1]] == [np.float32] * 2 and np.array_equal(calls["float"][1][0], f32)
    with pytest.raises(MttsError, match="22050"):
        t.files_to_dvectors([paths["i16_22k"]])
    t = tool(pcm16=True, resample=True)
    out = t.files_to_dvectors([paths["i16_22k"], paths["i16"], paths["f32"]])
    got = sorted((c[0], c[2]["source_rate"], len(c[1])) for c in t.embedder.calls)
    assert got == [("float", 16000, 1), ("pcm16", 16000, 1), ("pcm16", 22050, 1)] and np.array_equal(out[:, 0], [16, 16, 32])
    assert all(c[2]["normalize_dbfs"] == -30.0 for c in t.embedder.calls)
    with pytest.raises(ValueError, match="wav_loader"):
        E.WavsToDvector(None, None, wav_loader=E.read_wav_16k, pcm16=True)
