"""`Preprocessor` on libmtts.so (reference preprocessor/preprocessor.py): wavs + alignments -> the preprocessed feature tree
(`mel/ pitch/ energy/ duration/*.npy`, `stats.json`, `speakers.json`, `<subset>.txt`) that `meta_tts_amd.data.FeatureDataset` reads.

The device does the batched mel / energy front-end, the pitch interpolation, the phoneme-level segment means, the outlier filter
with the partial statistics, and the normalisation with its min / max (csrc/preprocess.h, the front-end through csrc/melfront.h);
every utterance of a call shares every launch.  The host does what is text or file handling: the TextGrid reader, `get_alignment`,
the walk over the corpus, the `.npy` files.  Two third-party steps are injected, not restated: pitch extraction (`f0_fn`; the default calls pyworld's DIO + StoneMask as
the reference does and raises when pyworld is missing) and the speaker-encoder reference mels (`spk_ref_fn`; skipped when absent).
`f0_fn="device"` needs no injected pitch: the batched YIN estimator of audio/pitch.py (csrc/pitch.h; NOT a DIO / StoneMask clone, parity
with pyworld unpinned) takes all waveforms of a batch in one call.
Wavs are read with scipy.io.wavfile (or an injected loader); a file whose rate differs from the config's raises unless
`build_from_path(resample=True)`, which resamples each batch's wavs on the device (audio/resample.py; librosa.load's role in the reference).

Deliberate differences from the reference's `build_from_path`: directory listings are sorted (the reference takes `os.listdir`
order), and an utterance without a TextGrid is skipped (the reference re-fits the previous utterance's values in that case)."""
from __future__ import annotations

import collections
import ctypes as C
import json
import os
import re

import numpy as np

from .audio.stft import TacotronSTFT, _OnHandle
from .engine import MttsError

Interval = collections.namedtuple("Interval", "start_time end_time text")
Utterance = collections.namedtuple("Utterance", "info pitch energy n_frames pitch_partial energy_partial")


class Tier:
    def __init__(self, name, objects):
        self.name, self._objects = name, list(objects)


class TextGrid:
    def __init__(self, tiers):
        self.tiers = list(tiers)

    def get_tier_by_name(self, name):
        for t in self.tiers:
            if t.name == name:
                return t
        raise ValueError(f"Textgrid has no tier named {name!r}")


_TG_ITEM = re.compile(r"^\s*item\s*\[\d+\]\s*:")
_TG_INTERVAL = re.compile(r"^\s*intervals\s*\[\d+\]\s*:")
_TG_FIELD = re.compile(r"^\s*(class|name|xmin|xmax|text)\s*=\s*(.*?)\s*$")


def read_textgrid(path, include_empty_intervals=False) -> TextGrid:
    """Minimal reader of Praat's long TextGrid format (what the Montreal Forced Aligner writes): interval tiers with
    `xmin / xmax / text` per interval.  Like `tgt.io.read_textgrid`, intervals with empty text are left out by default."""
    unq = lambda v: v[1:-1].replace('""', '"') if len(v) >= 2 and v[0] == '"' and v[-1] == '"' else v
    tiers, cur, iv = [], None, None
    with open(path, encoding="utf-8") as f:
        for line in f:
            if _TG_ITEM.match(line):
                cur, iv = {"class": "", "name": "", "intervals": []}, None
                tiers.append(cur)
                continue
            if cur is None:
                continue
            if _TG_INTERVAL.match(line):
                iv = {}
                cur["intervals"].append(iv)
                continue
            m = _TG_FIELD.match(line)
            if not m:
                continue
            key, val = m.group(1), unq(m.group(2))
            if iv is not None and key in ("xmin", "xmax", "text"):
                iv[key] = val if key == "text" else float(val)
            elif iv is None and key in ("class", "name"):
                cur[key] = val
    out = []
    for t in tiers:
        if t["class"] != "IntervalTier":
            continue
        objs = [Interval(i["xmin"], i["xmax"], i.get("text", "")) for i in t["intervals"]]
        out.append(Tier(t["name"], [o for o in objs if include_empty_intervals or o.text.strip() != ""]))
    return TextGrid(out)


def read_wav(path, keep_pcm16=False):
    """(float32 waveform in [-1, 1], sampling rate): integer PCM is scaled by its full range (int16: / 32768), multi-channel files are averaged.
    keep_pcm16: a mono 16-bit PCM file comes back as the int16 samples it holds (for `SpeakerEmbedder.embed_pcm16`, which widens them
    on the device); every other file as above."""
    from scipy.io import wavfile
    sr, x = wavfile.read(path)
    if keep_pcm16 and x.dtype == np.int16 and x.ndim == 1:
        return x, int(sr)
    if x.dtype.kind == "i":
        x = x.astype(np.float32) / float(2 ** (8 * x.dtype.itemsize - 1))
    elif x.dtype.kind == "u":
        x = (x.astype(np.float32) - 128.0) / 128.0
    x = np.asarray(x, np.float32)
    return (x.mean(axis=1).astype(np.float32) if x.ndim == 2 else x), int(sr)


def pyworld_f0(wav, sampling_rate, hop_length):
    """preprocessor.py:214-220: DIO + StoneMask at a frame period of one hop.  pyworld is third party and not restated."""
    try:
        import pyworld as pw
    except ImportError as e:
        raise MttsError("pitch extraction needs pyworld, which is not installed: pass f0_fn(wav, sampling_rate, hop_length) -> float64[T]") from e
    x = np.asarray(wav, np.float64)
    pitch, t = pw.dio(x, sampling_rate, frame_period=hop_length / sampling_rate * 1000)
    return pw.stonemask(x, pitch, t, sampling_rate)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Preprocessor(_OnHandle):
    """preprocessor/preprocessor.py:18 with the same preprocess-config keys (config/preprocess/LibriTTS.yaml)."""

    def __init__(self, config, *, max_samples=22050 * 40, device=0, lib_path=None):
        self.config = config
        self.in_dir = config["path"]["raw_path"]
        self.out_dir = config["path"]["preprocessed_path"]
        pp = config["preprocessing"]
        self.val_size = pp.get("val_size")
        self.sampling_rate = pp["audio"]["sampling_rate"]
        self.hop_length = pp["stft"]["hop_length"]
        assert pp["pitch"]["feature"] in ["phoneme_level", "frame_level"]
        assert pp["energy"]["feature"] in ["phoneme_level", "frame_level"]
        self.pitch_phoneme_averaging = pp["pitch"]["feature"] == "phoneme_level"
        self.energy_phoneme_averaging = pp["energy"]["feature"] == "phoneme_level"
        self.pitch_normalization = pp["pitch"]["normalization"]
        self.energy_normalization = pp["energy"]["normalization"]
        self.STFT = TacotronSTFT(pp["stft"]["filter_length"], pp["stft"]["hop_length"], pp["stft"]["win_length"], pp["mel"]["n_mel_channels"],
                                 pp["audio"]["sampling_rate"], pp["mel"]["mel_fmin"], pp["mel"]["mel_fmax"], max_samples=max_samples, device=device,
                                 lib_path=lib_path)
        self._dev = self.STFT._dev   # the TacotronSTFT's handle: this class's device steps run on it
        self._resamplers = {}   # file rate -> audio.resample.Resampler on this handle (build_from_path(resample=True))
        self._pitch = None      # audio.pitch.PitchExtractor on this handle, made by the first f0_batch call
        self.train_set = self.val_set = self.test_set = None
        if "subsets" in config:
            self.train_set = config["subsets"].get("train", None)
            self.val_set = config["subsets"].get("val", None)
            self.test_set = config["subsets"].get("test", None)

    def close(self):
        if getattr(self, "STFT", None) is not None:
            self.STFT.close()
            self.STFT = None

    # ---- host: alignment ---------------------------------------------------------------------------------------------------------
    def get_alignment(self, tier):
        """preprocessor.py:308-346 for any object with `_objects[*].start_time / end_time / text`."""
        sil_phones = ["sil", "sp", "spn"]
        phones, durations = [], []
        start_time = end_time = 0
        end_idx = 0
        for t in tier._objects:
            s, e, p = t.start_time, t.end_time, t.text
            if phones == []:            # trim leading silences
                if p in sil_phones:
                    continue
                start_time = s
            phones.append(p)
            if p not in sil_phones:
                end_time = e
                end_idx = len(phones)
            durations.append(int(np.round(e * self.sampling_rate / self.hop_length) - np.round(s * self.sampling_rate / self.hop_length)))
        return phones[:end_idx], durations[:end_idx], start_time, end_time   # trailing silences trimmed

    def remove_outlier(self, values):
        """preprocessor.py:348-356 on the host (the batched device form is `outlier_stats`)."""
        values = np.array(values)
        p25, p75 = np.percentile(values, 25), np.percentile(values, 75)
        lower, upper = p25 - 1.5 * (p75 - p25), p75 + 1.5 * (p75 - p25)
        return values[np.logical_and(values > lower, values < upper)]

    # ---- device steps (csrc/preprocess.h), lists of per-utterance arrays in and out ----------------------------------------------
    def mel_batch(self, wavs, keep_frames=None):
        """get_mel_from_wav of every waveform in one device call, truncated to keep_frames[u] frames (None / < 0: all).
        Returns ([mel (T_u, n_mel) float32], [energy (T_u,) float32])."""
        wavs = [np.ascontiguousarray(np.asarray(w, np.float32).reshape(-1)) for w in wavs]
        n = np.asarray([len(w) for w in wavs], np.int32)
        keep = np.full(len(wavs), -1, np.int32) if keep_frames is None else np.ascontiguousarray(np.asarray(keep_frames, np.int64).astype(np.int32))
        full = n.astype(np.int64) // self.hop_length + 1
        T = np.where(keep < 0, full, np.minimum(full, keep))
        if (T < 1).any():
            raise MttsError(f"mel_batch: utterance {int(np.argmax(T < 1))} keeps no frame (sum(duration) == 0)")
        total, n_mel = int(T.sum()), self.STFT.n_mel_channels
        mel, energy = np.empty((total, n_mel), np.float32), np.empty(total, np.float32)
        packed = np.ascontiguousarray(np.concatenate(wavs)) if wavs else np.empty(0, np.float32)
        self._check(self.lib.mtts_stft_mel_batch(self.h, len(wavs), _ptr(n), _ptr(keep), _ptr(packed), _ptr(mel), _ptr(energy)))
        cuts = np.cumsum(T)[:-1]
        return np.split(mel, cuts), np.split(energy, cuts)

    def f0_batch(self, wavs):
        """YIN F0 of every waveform in one device call on this preprocessor's handle (audio/pitch.py at its defaults: 71 .. 800 Hz,
        threshold 0.15).  Returns ([f0 (T_u,) float64, 0 = unvoiced], [aperiodicity (T_u,) float32]), T_u = len(wav) // hop_length + 1."""
        if self._pitch is None:
            from .audio.pitch import PitchExtractor
            self._pitch = PitchExtractor(self.sampling_rate, self.hop_length, _handle=self._dev)
        return self._pitch.f0_batch(wavs)

    def phoneme_average(self, values, durations, interpolate=False):
        """preprocessor.py:231-261 for a list of frame-level arrays (all float64, or all float32) and their duration lists."""
        dt = np.float64 if np.asarray(values[0]).dtype == np.float64 else np.float32
        vals = [np.ascontiguousarray(np.asarray(v, dt)) for v in values]
        durs = [np.asarray(d, np.int64).astype(np.int32) for d in durations]
        nf, ns = np.asarray([len(v) for v in vals], np.int32), np.asarray([len(d) for d in durs], np.int32)
        out = np.empty(int(ns.sum()), dt)
        pv, pd = np.ascontiguousarray(np.concatenate(vals)), np.ascontiguousarray(np.concatenate(durs))
        self._check(self.lib.mtts_stft_phoneme_average(self.h, len(vals), _ptr(nf), _ptr(ns), _ptr(pd), _ptr(pv), int(dt == np.float64), int(bool(interpolate)),
                                                       _ptr(out)))
        return np.split(out, np.cumsum(ns)[:-1])

    def outlier_stats(self, values):
        """remove_outlier's keep mask and the kept values' (count, mean, M2) per utterance: ([bool mask], float64 (n_utts, 3))."""
        dt = np.float64 if np.asarray(values[0]).dtype == np.float64 else np.float32
        vals = [np.ascontiguousarray(np.asarray(v, dt)) for v in values]
        nv = np.asarray([len(v) for v in vals], np.int32)
        keep, parts = np.zeros(max(int(nv.sum()), 1), np.uint8), np.zeros((len(vals), 3), np.float64)
        pv = np.ascontiguousarray(np.concatenate(vals + [np.zeros(1, dt)]))
        self._check(self.lib.mtts_stft_outlier_stats(self.h, len(vals), _ptr(nv), _ptr(pv), int(dt == np.float64), _ptr(keep), _ptr(parts)))
        return [m.astype(bool) for m in np.split(keep[: int(nv.sum())], np.cumsum(nv)[:-1])], parts

    def merge_stats(self, state, partials):
        """StandardScaler.partial_fit's update of state = (count, mean, M2) with the partials in the order given; returns the new state."""
        st = np.array(state, np.float64)
        p = np.ascontiguousarray(np.asarray(partials, np.float64).reshape(-1, 3))
        self._check(self.lib.mtts_stft_merge_stats(self.h, _ptr(st), len(p), _ptr(p)))
        return st

    @staticmethod
    def mean_std(state):
        """(mean_, scale_) of the fitted scaler: the population std, 1 where it is zero (sklearn's _handle_zeros_in_scale)."""
        std = float(np.sqrt(state[2] / state[0])) if state[0] > 0 else 1.0
        return float(state[1]), (std if std > 0 else 1.0)

    def normalize_values(self, values, mean, std):
        """(values - mean) / std in float64 for a list of arrays of one dtype, and (min, max) over all of them."""
        dt = np.float64 if np.asarray(values[0]).dtype == np.float64 else np.float32
        vals = [np.ascontiguousarray(np.asarray(v, dt)) for v in values]
        pv = np.ascontiguousarray(np.concatenate(vals))
        out, mm = np.empty(len(pv), np.float64), np.empty(2, np.float64)
        self._check(self.lib.mtts_stft_normalize(self.h, len(pv), _ptr(pv), int(dt == np.float64), float(mean), float(std), _ptr(out), _ptr(mm)))
        return np.split(out, np.cumsum([len(v) for v in vals])[:-1]), float(mm[0]), float(mm[1])

    def normalize(self, in_dir, mean, std):
        """preprocessor.py:358-369: rewrite every file of in_dir as (x - mean) / std, return (min, max) of the normalised values."""
        names = sorted(os.listdir(in_dir))
        min_value, max_value = np.finfo(np.float64).max, np.finfo(np.float64).min
        groups = {}
        for nm in names:
            v = np.load(os.path.join(in_dir, nm))
            groups.setdefault(np.float64 if v.dtype == np.float64 else np.float32, []).append((nm, v))
        for dt, files in groups.items():
            live = [(nm, v) for nm, v in files if len(v) > 0]
            if not live:
                continue
            outs, lo, hi = self.normalize_values([np.asarray(v, dt) for _, v in live], mean, std)
            for (nm, _), o in zip(live, outs):
                np.save(os.path.join(in_dir, nm), o)
            min_value, max_value = min(min_value, lo), max(max_value, hi)
        return min_value, max_value

    # ---- the batched utterance path ----------------------------------------------------------------------------------------------
    def process_utterances(self, items, spk_ref_fn=None):
        """preprocessor.py:188-306 for a batch.  items: (speaker, basename, wav, phones, durations, f0, raw_text) with the wav already
        cut to the alignment's [start, end) and f0 float64 per frame.  Writes the duration / pitch / energy / mel files and returns, per
        item, None (dropped: at most one voiced frame) or Utterance(info, kept pitch, kept energy, n_frames, pitch_partial, energy_partial)."""
        results = [None] * len(items)
        live = []
        for k, (speaker, basename, wav, phones, durations, f0, raw_text) in enumerate(items):
            total = int(sum(durations))
            pitch = np.asarray(f0, np.float64)[:total]
            if np.sum(pitch != 0) <= 1:
                continue
            live.append((k, speaker, basename, np.asarray(wav, np.float32), list(phones), [int(d) for d in durations], pitch, raw_text, total))
        if not live:
            return results
        mels, energies = self.mel_batch([x[3] for x in live], [x[8] for x in live])
        pitches = [x[6] for x in live]
        durs = [x[5] for x in live]
        if self.pitch_phoneme_averaging:
            pitches = self.phoneme_average(pitches, durs, interpolate=True)
        if self.energy_phoneme_averaging:
            energies = self.phoneme_average(energies, durs, interpolate=False)
        pkeep, pparts = self.outlier_stats(pitches)
        ekeep, eparts = self.outlier_stats(energies)
        for j, (k, speaker, basename, wav, phones, durations, _, raw_text, _) in enumerate(live):
            np.save(os.path.join(self.out_dir, "duration", f"{speaker}-duration-{basename}.npy"), durations)
            np.save(os.path.join(self.out_dir, "pitch", f"{speaker}-pitch-{basename}.npy"), pitches[j])
            np.save(os.path.join(self.out_dir, "energy", f"{speaker}-energy-{basename}.npy"), energies[j])
            np.save(os.path.join(self.out_dir, "mel", f"{speaker}-mel-{basename}.npy"), mels[j])
            if spk_ref_fn is not None:
                os.makedirs(os.path.join(self.out_dir, "spk_ref_mel_slices"), exist_ok=True)
                np.save(os.path.join(self.out_dir, "spk_ref_mel_slices", f"{speaker}-mel-{basename}.npy"), spk_ref_fn(speaker, basename))
            info = "|".join([basename, speaker, "{" + " ".join(phones) + "}", raw_text])
            results[k] = Utterance(info, pitches[j][pkeep[j]], energies[j][ekeep[j]], int(mels[j].shape[0]), pparts[j].copy(), eparts[j].copy())
        return results

    def speaker_reference_fn(self, embedder, wav_loader=None, resample=None, trim=False):
        """A ready-made `spk_ref_fn` for `build_from_path` / `process_utterances` (preprocessor.py:263-299): (speaker, basename) -> the
        (n_partials, 160, 40) float32 `spk_ref_mel_slices` of the WHOLE raw file <raw_path>/<subset>/<speaker>/<basename>.wav, computed on
        the device by `embedder` (a meta_tts_amd.evaluation.SpeakerEmbedder; `encoder=False` is enough).  The speaker encoder takes
        16 kHz waveforms: a file at another rate needs `resample(wav, rate) -> 16 kHz float32 waveform` (an audio.resample.Resampler),
        else it is an error.  trim=True (or a dict of audio.vad.SilenceTrimmer keywords): the rest of resemblyzer's `preprocess_wav` on
        the device in front of the slices — normalisation to -30 dBFS (increase only) and silence trimming (this project's detector;
        parity with webrtcvad is unpinned).  Default: neither, as before."""
        from .evaluation import SAMPLING_RATE
        wav_loader = wav_loader or read_wav
        subsets = [d for ds in (self.train_set, self.val_set, self.test_set) for d in (ds if isinstance(ds, list) else [ds]) if isinstance(d, str)]

        def spk_ref_fn(speaker, basename):
            for dset in subsets:
                path = os.path.join(self.in_dir, dset, speaker, f"{basename}.wav")
                if os.path.exists(path):
                    break
            else:
                raise MttsError(f"speaker reference: no raw wav for {speaker}/{basename}")
            wav, rate = wav_loader(path)
            if int(rate) != SAMPLING_RATE:
                if resample is None:
                    raise MttsError(f"{path}: sampling rate {rate}, the speaker encoder takes {SAMPLING_RATE} Hz (no resampling here: pass resample=)")
                wav = resample(wav, rate)
            if trim:
                return embedder.reference_mel_slices(np.asarray(wav, np.float32), source_rate=SAMPLING_RATE, normalize_dbfs=-30.0, trim=trim)
            return embedder.reference_mel_slices(np.asarray(wav, np.float32))
        return spk_ref_fn

    def resample_to_config_rate(self, wavs, rates, preset="kaiser_best"):
        """The waveforms whose rate differs from the config's, resampled on the device: one `resample_batch` call per distinct rate."""
        from .audio.resample import Resampler
        out = [np.asarray(w, np.float32) for w in wavs]
        by_rate = {}
        for i, r in enumerate(rates):
            if int(r) != int(self.sampling_rate):
                by_rate.setdefault(int(r), []).append(i)
        for rate, idx in sorted(by_rate.items()):
            if (rate, preset) not in self._resamplers:
                self._resamplers[(rate, preset)] = Resampler(rate, int(self.sampling_rate), preset, _handle=self._dev)
            for i, w in zip(idx, self._resamplers[(rate, preset)].resample_batch([out[i] for i in idx])):
                out[i] = w
        return out

    def build_from_path(self, f0_fn=None, batch_utterances=32, wav_loader=None, spk_ref_fn=None, resample=False):
        """preprocessor.py:60-185.  f0_fn(wav, sampling_rate, hop_length) -> float64[T] (default: pyworld), or the string "device": one
        `f0_batch` call (YIN on the device) for all cut waveforms of a batch; wav_loader(path) -> (float32
        wav, rate) (default: scipy.io.wavfile); spk_ref_fn(speaker, basename) -> the spk_ref_mel_slices array (default: not written;
        `speaker_reference_fn` makes one on the device).
        `batch_utterances` utterances share each device call.  resample=True: a file at another rate than the config's is not an error;
        the wavs of a batch are resampled to the config's rate in one device call per distinct rate (kaiser_best) before they are cut
        to the alignment's [start, end) and handed to f0_fn.  Returns {subset: [metadata lines]}."""
        if isinstance(f0_fn, str) and f0_fn != "device":
            raise MttsError(f"build_from_path: f0_fn={f0_fn!r} (a callable, None for pyworld, or \"device\")")
        f0_fn = f0_fn or pyworld_f0
        wav_loader = wav_loader or read_wav
        for kind in ("mel", "pitch", "energy", "duration"):
            os.makedirs(os.path.join(self.out_dir, kind), exist_ok=True)
        dsets = []
        for dset in [self.train_set, self.val_set, self.test_set]:
            if isinstance(dset, list):
                dsets += dset
            elif isinstance(dset, str):
                dsets.append(dset)
        speakers, outs, n_frames = {}, {}, 0
        state = {"pitch": np.zeros(3), "energy": np.zeros(3)}
        i = 0

        def flush(pending, out):
            nonlocal n_frames
            # pending: (speaker, basename, whole wav, its rate, phones, durations, start, end, raw_text)
            wavs = [p[2] for p in pending]
            if resample:
                wavs = self.resample_to_config_rate(wavs, [p[3] for p in pending])
            cut = [np.asarray(wav, np.float32)[int(self.sampling_rate * p[6]): int(self.sampling_rate * p[7])] for p, wav in zip(pending, wavs)]
            f0s = self.f0_batch(cut)[0] if f0_fn == "device" else [np.asarray(f0_fn(wav, self.sampling_rate, self.hop_length), np.float64) for wav in cut]
            items = [(p[0], p[1], wav, p[4], p[5], f0, p[8]) for p, wav, f0 in zip(pending, cut, f0s)]
            for r in self.process_utterances(items, spk_ref_fn=spk_ref_fn):
                if r is None:
                    continue
                out.append(r.info)
                state["pitch"] = self.merge_stats(state["pitch"], r.pitch_partial)
                state["energy"] = self.merge_stats(state["energy"], r.energy_partial)
                n_frames += r.n_frames
            pending.clear()

        for dset in dsets:
            dset_dir = os.path.join(self.in_dir, dset)
            out, pending = [], []
            for speaker in sorted(os.listdir(dset_dir)):
                speakers[speaker] = i
                for wav_name in sorted(os.listdir(os.path.join(dset_dir, speaker))):
                    if ".wav" not in wav_name:
                        continue
                    basename = wav_name.split(".")[0]
                    tg_path = os.path.join(self.out_dir, "TextGrid", speaker, f"{basename}.TextGrid")
                    if not os.path.exists(tg_path):
                        continue
                    phones, durations, start, end = self.get_alignment(read_textgrid(tg_path).get_tier_by_name("phones"))
                    if start >= end:
                        continue
                    wav, sr = wav_loader(os.path.join(dset_dir, speaker, wav_name))
                    if int(sr) != int(self.sampling_rate) and not resample:
                        raise MttsError(f"{wav_name}: sampling rate {sr} differs from the config's {self.sampling_rate} (no resampling here: pass resample=True)")
                    with open(os.path.join(dset_dir, speaker, f"{basename}.lab")) as f:
                        raw_text = f.readline().strip("\n")
                    pending.append((speaker, basename, wav, int(sr), phones, durations, start, end, raw_text))
                    if len(pending) >= batch_utterances:
                        flush(pending, out)
                i += 1
            if pending:
                flush(pending, out)
            outs[dset] = out

        stats_path = os.path.join(self.out_dir, "stats.json")
        old = json.load(open(stats_path)) if os.path.exists(stats_path) else None   # an additional corpus keeps the first one's mean / std
        means = {}
        for feat, on in (("pitch", self.pitch_normalization), ("energy", self.energy_normalization)):
            if not on:
                means[feat] = (0, 1)
            elif old is not None:
                means[feat] = (old[feat][2], old[feat][3])
            else:
                means[feat] = self.mean_std(state[feat])
        pitch_min, pitch_max = self.normalize(os.path.join(self.out_dir, "pitch"), *means["pitch"])
        energy_min, energy_max = self.normalize(os.path.join(self.out_dir, "energy"), *means["energy"])
        with open(os.path.join(self.out_dir, "speakers.json"), "w") as f:
            f.write(json.dumps(speakers))
        with open(stats_path, "w") as f:
            f.write(json.dumps({"pitch": [float(pitch_min), float(pitch_max), float(means["pitch"][0]), float(means["pitch"][1])],
                                "energy": [float(energy_min), float(energy_max), float(means["energy"][0]), float(means["energy"][1])]}))
        self.total_hours = n_frames * self.hop_length / self.sampling_rate / 3600
        for dset, out in outs.items():
            with open(os.path.join(self.out_dir, f"{dset}.txt"), "w", encoding="utf-8") as f:
                for m in out:
                    f.write(m + "\n")
        return outs
