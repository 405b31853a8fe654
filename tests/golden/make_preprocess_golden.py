#!/usr/bin/env python3
"""Generates tests/golden/preprocess.npz by running the REFERENCE's own `Preprocessor.build_from_path`
(/root/reference/preprocessor/preprocessor.py) on a tiny synthetic corpus in the build container, with only its third-party I/O stubbed:
  * tgt.io.read_textgrid -> stub tiers (objects with `_objects[*].start_time / end_time / text`) built from stored arrays;
  * librosa.load -> the stored waveforms; librosa.util / librosa.filters as in make_stft_golden.py (the mel basis is
    meta_tts_amd.audio.stft.mel_filterbank, an INPUT of the fixture);
  * pyworld.dio / stonemask -> the stored f0 of the utterance just loaded;
  * resemblyzer -> dummies (the speaker-encoder reference mels are out of scope);
  * os.listdir -> sorted (the reference takes directory order; meta_tts_amd.preprocessor sorts);
  * torch.Tensor.cuda -> identity.
Everything else is the reference: get_alignment, the wav cut, get_mel_from_wav, interp1d, the in-place segment means, remove_outlier,
StandardScaler.partial_fit, normalize, the files it writes.  Recorded besides the files: the frame-level energy get_mel_from_wav
returned, and remove_outlier's inputs (the un-normalised saved values) and keep masks.
The reference never travels: only this script and the arrays it writes are committed.

Runs: "small" (64 / 16 / 64, 12 mels, 8 kHz; 2 speakers x 3 utterances; phoneme-level pitch and energy), "small_frame" (the same
corpus, frame-level pitch and energy), "libritts" (1024 / 256 / 1024, 80 mels, 22050 Hz; one utterance of about a second).
The corpus holds zero durations, an aliased utterance (some pos < i in the in-place loop), an utterance dropped for <= 1 voiced frame,
leading / trailing / inner silences.  Asserted here: the aliasing, the drop, and that no value lies within a relative 1e-4 of an
outlier fence (so equality of keep masks is a fair demand on float32 energy)."""
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference")

from meta_tts_amd.audio import stft as ours  # noqa: E402  (mel basis shim only)


def pad_center(data, size, axis=-1, **kw):
    n = data.shape[axis]
    lpad = int((size - n) // 2)
    lengths = [(0, 0)] * data.ndim
    lengths[axis] = (lpad, int(size - n - lpad))
    return np.pad(data, lengths, **kw)


STORE = {"wav": {}, "tg": {}, "f0": {}, "cur": None}


class Iv:
    def __init__(self, a, b, t):
        self.start_time, self.end_time, self.text = a, b, t


class Tier:
    def __init__(self, ivs):
        self._objects = ivs


class TG:
    def __init__(self, t):
        self.t = t

    def get_tier_by_name(self, n):
        assert n == "phones"
        return self.t


def _load(path, *a, **k):
    STORE["cur"] = os.path.basename(path).split(".")[0]
    return STORE["wav"][STORE["cur"]], None


librosa = types.ModuleType("librosa")
librosa.util = types.ModuleType("librosa.util")
librosa.filters = types.ModuleType("librosa.filters")
librosa.util.pad_center = pad_center
librosa.util.tiny = lambda x: np.finfo(np.float32).tiny
librosa.util.normalize = lambda S, norm=np.inf, **k: S
librosa.filters.mel = lambda sr, n_fft, n_mels, fmin, fmax: ours.mel_filterbank(sr, n_fft, n_mels, fmin, fmax)
librosa.load = _load
tgt = types.ModuleType("tgt")
tgt.io = types.ModuleType("tgt.io")
tgt.io.read_textgrid = lambda p: TG(STORE["tg"][os.path.basename(p).split(".")[0]])
pw = types.ModuleType("pyworld")
pw.dio = lambda wav, sr, frame_period: (STORE["f0"][STORE["cur"]].copy(), None)
pw.stonemask = lambda wav, p, t, sr: p
res = types.ModuleType("resemblyzer")
res.preprocess_wav = lambda p: np.zeros(16000, np.float32)
res.wav_to_mel_spectrogram = lambda w: np.zeros((100, 40), np.float32)


class VE:
    @staticmethod
    def compute_partial_slices(n, rate, min_coverage):
        return [slice(0, 16000)], [slice(0, 100)]


res.VoiceEncoder = VE
sys.modules.update({"librosa": librosa, "librosa.util": librosa.util, "librosa.filters": librosa.filters, "tgt": tgt, "tgt.io": tgt.io,
                    "pyworld": pw, "resemblyzer": res})
torch.Tensor.cuda = lambda self, *a, **k: self
_listdir = os.listdir
os.listdir = lambda p: sorted(_listdir(p))

import audio as Audio  # noqa: E402  (the reference)
from preprocessor import preprocessor as ref_mod  # noqa: E402
from preprocessor.preprocessor import Preprocessor  # noqa: E402

OUT = {}


def make_corpus(name, sr, hop, speakers, n_utts, seed, s_range, lead=0.05):
    """Waveforms, tiers and f0 of a corpus, stored as arrays under `<name>|...`; fills STORE."""
    g = np.random.RandomState(seed)
    utts = []
    for spk in speakers:
        for u in range(n_utts):
            base = f"{spk}_u{u}"
            durs = g.randint(0, 9, size=g.randint(*s_range))
            durs[0] = max(durs[0], 1)
            if u == 2:                                  # the aliased shape: zero durations early, so that pos < i later on
                durs[:4] = [1, 0, 0, 5]
            durs[-1] = max(durs[-1], 2)
            durs[len(durs) // 2] = 0                    # every utterance has a zero duration
            texts = ["AH0" if i % 5 else "sp" for i in range(len(durs))]        # inner silences
            texts[0], texts[-1] = "T", "IY1"
            edges = np.concatenate([[0], np.cumsum(durs)]) * hop / sr
            start = [0.0] + [lead + e for e in edges[:-1]] + [lead + edges[-1]]  # leading "sil", trailing "sp"
            end = [lead] + [lead + e for e in edges[1:]] + [lead + edges[-1] + 0.04]
            texts = ["sil"] + texts + ["sp"]
            n = int(sr * end[-1]) + 7 + u
            t = np.arange(n) / sr
            w = (0.3 * np.sin(2 * np.pi * 200 * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t)) + 0.05 * g.standard_normal(n)).astype(np.float32)
            w[n // 2] = 1.3                             # one sample outside [-1, 1]: get_mel_from_wav clips
            T = int(durs.sum()) + 4
            f0 = 120 + 40 * g.standard_normal(T)
            f0[g.rand(T) < 0.3] = 0
            f0[0] = 0                                   # unvoiced edges: the fill values of interp1d
            f0[int(durs.sum()) - 1] = 0
            if spk == speakers[-1] and u == 1:          # dropped: a single voiced frame
                f0[:] = 0
                f0[3] = 111.0
            STORE["wav"][base], STORE["f0"][base] = w, f0
            STORE["tg"][base] = Tier([Iv(a, b, c) for a, b, c in zip(start, end, texts)])
            OUT[f"{name}|{base}|wav"], OUT[f"{name}|{base}|f0"] = w, f0
            OUT[f"{name}|{base}|tg_start"], OUT[f"{name}|{base}|tg_end"] = np.asarray(start, np.float64), np.asarray(end, np.float64)
            OUT[f"{name}|{base}|tg_text"] = np.asarray(texts)
            utts.append(f"{spk}/{base}")
    OUT[f"{name}|utts"] = np.asarray(utts)
    return utts


def run(tag, corpus, utts, sr, n_fft, hop, win, n_mel, pitch_feature, energy_feature):
    tmp = tempfile.mkdtemp()
    raw, out = os.path.join(tmp, "raw"), os.path.join(tmp, "out")
    cfg = {"path": {"raw_path": raw, "preprocessed_path": out},
           "preprocessing": {"val_size": 0, "audio": {"sampling_rate": sr, "max_wav_value": 32768.0},
                             "stft": {"filter_length": n_fft, "hop_length": hop, "win_length": win},
                             "mel": {"n_mel_channels": n_mel, "mel_fmin": 0, "mel_fmax": None},
                             "pitch": {"feature": pitch_feature, "normalization": True},
                             "energy": {"feature": energy_feature, "normalization": True}},
           "subsets": {"train": "train"}}
    for su in utts:
        spk, base = su.split("/")
        os.makedirs(os.path.join(raw, "train", spk), exist_ok=True)
        os.makedirs(os.path.join(out, "TextGrid", spk), exist_ok=True)
        open(os.path.join(raw, "train", spk, base + ".wav"), "w").close()
        open(os.path.join(raw, "train", spk, base + ".lab"), "w").write(f"raw text of {base}\n")
        open(os.path.join(out, "TextGrid", spk, base + ".TextGrid"), "w").close()
    p = Preprocessor(cfg)
    rec = {"outlier": []}
    orig_mel, orig_ro = Audio.tools.get_mel_from_wav, p.remove_outlier

    def mel_hook(wav, st):
        m, e = orig_mel(wav, st)
        rec.setdefault("frame_energy", {})[STORE["cur"]] = np.array(e, np.float32)   # before the truncation and the in-place means
        return m, e

    def ro_hook(values):
        values = np.array(values)
        kept = orig_ro(values)
        p25, p75 = np.percentile(values, 25), np.percentile(values, 75)
        lower, upper = p25 - 1.5 * (p75 - p25), p75 + 1.5 * (p75 - p25)
        for fence in (lower, upper):                     # nothing near a fence: masks are precision independent
            assert np.all(np.abs(values - fence) > 1e-4 * max(abs(fence), 1e-30)), (tag, STORE["cur"], fence)
        mask = np.isin(values, kept)
        assert np.array_equal(values[mask], kept)
        rec["outlier"].append((STORE["cur"], values.copy(), mask))
        return kept

    Audio.tools.get_mel_from_wav, p.remove_outlier = mel_hook, ro_hook
    try:
        outs = p.build_from_path()
    finally:
        Audio.tools.get_mel_from_wav = orig_mel
    OUT[f"{tag}|cfg"] = np.asarray(json.dumps(cfg["preprocessing"]))
    OUT[f"{tag}|corpus"] = np.asarray(corpus)
    OUT[f"{tag}|train_txt"] = np.asarray("\n".join(outs["train"]))
    OUT[f"{tag}|speakers"] = np.asarray(open(os.path.join(out, "speakers.json")).read())
    st = json.load(open(os.path.join(out, "stats.json")))
    OUT[f"{tag}|stats"] = np.asarray(st["pitch"] + st["energy"], np.float64)
    OUT[f"{tag}|mel_basis"] = p.STFT.mel_basis.numpy()
    kept_bases = [ln.split("|")[0] for ln in outs["train"]]
    for base in kept_bases:
        spk = base.split("_")[0]
        for kind in ("mel", "pitch", "energy", "duration"):
            OUT[f"{tag}|{base}|{kind}"] = np.load(os.path.join(out, kind, f"{spk}-{kind}-{base}.npy"))
        OUT[f"{tag}|{base}|frame_energy"] = rec["frame_energy"][base]
    assert len(rec["outlier"]) == 2 * len(kept_bases)
    for k, (base, values, mask) in enumerate(rec["outlier"]):      # process_utterance calls remove_outlier(pitch) then (energy)
        feat = "pitch" if k % 2 == 0 else "energy"
        OUT[f"{tag}|{base}|{feat}_raw"], OUT[f"{tag}|{base}|{feat}_keep"] = values, mask
    files = {kind: sorted(os.listdir(os.path.join(out, kind))) for kind in ("mel", "pitch", "energy", "duration")}
    OUT[f"{tag}|files"] = np.asarray(json.dumps(files))
    return p, kept_bases


small = make_corpus("small", 8000, 16, ("s1", "s2"), 3, 0, (8, 20))
p, kept = run("small", "small", small, 8000, 64, 16, 64, 12, "phoneme_level", "phoneme_level")
assert len(kept) == 5 and "s2_u1" not in kept, kept                     # the utterance with one voiced frame is dropped
n_alias = 0
for su in small:
    base = su.split("/")[1]
    ph, du, s, e = p.get_alignment(STORE["tg"][base])
    alias = any(sum(du[:i]) < i and du[i] > 0 for i in range(len(du)))
    n_alias += alias and base in kept
    print(base, "S", len(du), "sum", sum(du), "zeros", du.count(0), "aliased", alias, "kept", base in kept)
    assert 0 in du
assert n_alias >= 1
run("small_frame", "small", small, 8000, 64, 16, 64, 12, "frame_level", "frame_level")
big = make_corpus("libritts", 22050, 256, ("s9",), 1, 1, (14, 18))
run("libritts", "libritts", big, 22050, 1024, 256, 1024, 80, "phoneme_level", "phoneme_level")
np.savez_compressed(os.path.join(HERE, "preprocess.npz"), **OUT)
print(len(OUT), "arrays,", os.path.getsize(os.path.join(HERE, "preprocess.npz")), "bytes")
