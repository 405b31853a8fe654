"""Speaker-similarity evaluation of a test run's result tree — the reference's `evaluation/` package on libmtts.so
(evaluation/wavs_to_dvector.py, pair_similarity.py, centroid_similarity.py, speaker_verification.py:32-59,301-305).

The hot path is wav -> d-vector: thousands of utterances, each about sixteen 160-frame partial utterances through LSTM(40, 256, 3).
`SpeakerEmbedder` owns an `mtts_stft` handle at the speaker encoder's front-end configuration (n_fft 400, hop 160, 40 mels, 16 kHz)
and an `mtts_dvector` handle, and sends whole batches of waveforms through ONE chain of launches (csrc/speakereval.h): packed STFT,
power spectrum, mel projection, the partial windows gathered on the device, the encoder.  The cosine similarities and the speaker
centroids are device kernels too (index arrays in place of the reference's np.repeat copies); the DET / ROC curves behind EER and AUC
are a few hundred scores and run on the host in numpy (sklearn's det_curve / roc_curve / auc restated; sklearn is not imported).

resemblyzer is not vendored by the reference and not part of this project: its `wav_to_mel_spectrogram` and
`VoiceEncoder.compute_partial_slices` are restated here from the published recipe.  Of its `preprocess_wav`, resampling to 16 kHz and
the -30 dBFS volume normalisation run on the device when asked for (`embed_utterances(source_rate=, normalize_dbfs=)`,
`WavsToDvector(resample=True)`; audio/resample.py, csrc/resample.h), and so does its silence trimming (`embed_utterances(trim=True)`,
`WavsToDvector(trim=True)`; audio/vad.py, csrc/vad.h): resemblyzer's post-processing exactly, around an energy detector of this project's
in place of webrtcvad's decision — parity with webrtcvad is UNPINNED.  Without those arguments every waveform handed to this module is
taken as 16 kHz float32 as it is.

The t-SNE behind the reference's scatter figure (evaluation/visualize.py) runs on the device too: `TSNE` keeps sklearn's surface for
what the reference uses and drives csrc/tsne.h — sklearn's method="exact" definition, not the Barnes-Hut approximation the reference's
call gets on the CPU; sklearn is not imported.  `VisualizeDvector` loads the modes' d-vectors, embeds them jointly, cuts out the
speakers of the figure and returns (or writes as CSV) the table the plot is drawn from.  The figures themselves (the reference's
matplotlib / seaborn plots) and MOS prediction (third-party networks) are out of scope.

Beyond the reference: `MelCepstralDistortion` and `ObjectiveEvaluation` score whether a synthesis SAYS what its recording says — mel-cepstral
distortion along a DTW path, with F0 error and voiced/unvoiced disagreement on the same path (csrc/dtw.h; the definition is this
project's own, include/mtts.h states it, and parity with SPTK / WORLD mel-cepstra is UNPINNED)."""
from __future__ import annotations

import ctypes as C
import json
import math
import os
import random
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np

from ._lib import WavSource as _WavSource
from .audio.stft import _Handle, _pack_wavs, forward_basis, mel_filterbank
from .engine import MttsError
from .speaker_encoder import EMBED, HIDDEN, LAYERS, MEL_N_CHANNELS, PARTIAL_FRAMES, DVectorEncoder

SAMPLING_RATE = 16000          # resemblyzer hparams: sampling_rate
MEL_WINDOW_LENGTH = 25         # ms -> n_fft = 400
MEL_WINDOW_STEP = 10           # ms -> hop = 160
N_FFT = SAMPLING_RATE * MEL_WINDOW_LENGTH // 1000
HOP = SAMPLING_RATE * MEL_WINDOW_STEP // 1000


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def frame_step_of(rate: float = 1.3) -> int:
    """Frames between two partial utterances: round(sampling_rate / rate / samples_per_frame) (np.round: half to even)."""
    return int(np.round((SAMPLING_RATE / rate) / HOP))


def compute_partial_slices(n_samples: int, rate: float = 1.3, min_coverage: float = 0.75):
    """resemblyzer's `VoiceEncoder.compute_partial_slices`: (wav_slices, mel_slices) of the 160-frame windows every
    `frame_step_of(rate)` frames; the last window is dropped when it covers less than `min_coverage` of its span and is not the
    only one.  The caller zero-extends the waveform to wav_slices[-1].stop (preprocessor.py:272-274)."""
    assert 0 < min_coverage <= 1
    n_frames = -(-(int(n_samples) + 1) // HOP)                    # ceil((n_samples + 1) / samples_per_frame)
    frame_step = frame_step_of(rate)
    assert 0 < frame_step <= PARTIAL_FRAMES
    wav_slices, mel_slices = [], []
    steps = max(1, n_frames - PARTIAL_FRAMES + frame_step + 1)
    for i in range(0, steps, frame_step):
        mel_slices.append(slice(i, i + PARTIAL_FRAMES))
        wav_slices.append(slice(i * HOP, (i + PARTIAL_FRAMES) * HOP))
    last = wav_slices[-1]
    coverage = (n_samples - last.start) / (last.stop - last.start)
    if coverage < min_coverage and len(mel_slices) > 1:
        mel_slices, wav_slices = mel_slices[:-1], wav_slices[:-1]
    return wav_slices, mel_slices


class SpeakerEmbedder:
    """The speaker encoder end to end on the device.  `state_dict`: the resemblyzer `VoiceEncoder` weights in torch's names
    (lstm.weight_ih_l0 ... linear.bias; None: deterministic synthetic weights, for tests and benchmarks); `encoder=False` builds the
    front-end only (`reference_mel_slices` for preprocessing).  Waveforms are 16 kHz float32 and are NOT resampled, normalised or
    trimmed unless `embed_utterances` is given `source_rate` / `normalize_dbfs` / `trim` (the detector behind `trim` is this project's
    own, audio/vad.py: parity with resemblyzer's webrtcvad is unpinned)."""

    def __init__(self, state_dict=None, max_partials: int = 2048, max_utts: int = 256, hidden: int = HIDDEN, emb: int = EMBED, layers: int = LAYERS,
                 rate: float = 1.3, min_coverage: float = 0.75, device: int = 0, lib_path=None, encoder: bool = True):
        self.rate, self.min_coverage, self.frame_step = rate, min_coverage, frame_step_of(rate)
        self.emb = emb
        self._dev = _Handle(N_FFT, HOP, MEL_N_CHANNELS, SAMPLING_RATE * 60, device, lib_path)
        self.lib = self._dev.lib
        self.forward_basis = forward_basis(N_FFT, N_FFT, "hann")
        self.mel_basis = mel_filterbank(SAMPLING_RATE, N_FFT, MEL_N_CHANNELS)
        self._dev.check(self.lib.mtts_stft_load(self._dev.h, _ptr(self.forward_basis), _ptr(self.mel_basis)))
        self.encoder = DVectorEncoder(state_dict, max_partials=max_partials, max_utts=max_utts, hidden=hidden, emb=emb, layers=layers, device=device,
                                      lib_path=lib_path) if encoder else None
        self._resamplers = {}   # source rate -> audio.resample.Resampler on this front-end's handle (embed_utterances(source_rate=))
        self._trimmers = {}     # configuration -> audio.vad.SilenceTrimmer on the same handle (embed_utterances(trim=True))
        self.last_trimmed_lengths = None   # int32 [n]: the trimmed 16 kHz lengths of the last embed_utterances(trim=...) call

    def set_streams(self, stft_stream: int, encoder_stream: Optional[int] = None):
        """HIP streams of the two handles (the stages are ordered by events when they differ)."""
        if self.lib.mtts_stft_set_stream(self._dev.h, C.c_void_p(stft_stream)) != 0:
            raise RuntimeError("mtts_stft_set_stream failed")
        if self.encoder is not None:
            self.encoder.set_stream(stft_stream if encoder_stream is None else encoder_stream)

    def close(self):
        if self.encoder is not None:
            self.encoder.close()
        self._dev.close()

    def wav_to_mel_spectrogram(self, wavs) -> List[np.ndarray]:
        """resemblyzer's `wav_to_mel_spectrogram` for a list of waveforms: [(T_u, 40) float32], T_u = len // 160 + 1."""
        ws, n, packed = _pack_wavs(wavs)
        T = n // HOP + 1
        mel = np.empty((int(T.sum()), MEL_N_CHANNELS), np.float32)
        self._dev.check(self.lib.mtts_stft_power_mel_batch(self._dev.h, len(ws), _ptr(n), _ptr(packed), _ptr(mel)))
        return np.split(mel, np.cumsum(T)[:-1])

    def resampler(self, source_rate: int, preset: str = "kaiser_best"):
        """The resampler source_rate -> 16 kHz on this front-end's handle (built on first use; 16 kHz itself: the identity)."""
        from .audio.resample import Resampler
        key = (int(source_rate), preset)
        if key not in self._resamplers:
            self._resamplers[key] = Resampler(int(source_rate), SAMPLING_RATE, preset, _handle=self._dev)
        return self._resamplers[key]

    def trimmer(self, **config):
        """The silence trimmer on this front-end's handle (built on first use; `config`: audio.vad.SilenceTrimmer's detector keywords —
        window_ms, ma_width, max_silence, floor_db, noise_quantile, margin_db; the rate is the encoder's 16 kHz)."""
        from .audio.vad import SilenceTrimmer
        fixed = sorted(set(config) & {"sampling_rate", "device", "lib_path", "max_samples", "_handle"})
        if fixed:
            raise ValueError(f"SpeakerEmbedder.trimmer: {', '.join(fixed)} cannot be set here (the trimmer runs on this front-end's handle at sampling_rate {SAMPLING_RATE})")
        key = tuple(sorted(config.items()))
        if key not in self._trimmers:
            self._trimmers[key] = SilenceTrimmer(sampling_rate=SAMPLING_RATE, _handle=self._dev, **config)
        return self._trimmers[key]

    def _run(self, wavs, want_vectors: bool, want_slices: bool, source_rate=None, normalize_dbfs=None, increase_only=True, trim=False):
        """One chained entry for all waveforms: the plain one, the resampled one (source_rate), or all of `preprocess_wav` (trim)."""
        _, n, packed = _pack_wavs(wavs)
        return self._chain(n, packed, None, want_vectors, want_slices, source_rate, normalize_dbfs, increase_only, trim)

    def _chain(self, n, packed, source, want_vectors: bool, want_slices: bool, source_rate=None, normalize_dbfs=None, increase_only=True, trim=False):
        """`n` [B] int32 lengths of waveforms that are either `packed` host float32 (source None: the three older entries) or described by
        `source`, a `_lib.WavSource` (mtts_dvector_embed_wavs_source; `packed` then only keeps its host memory alive)."""
        rs = vad = None
        if trim and source_rate is None:
            source_rate = SAMPLING_RATE      # the chained entry resamples with whatever bank the handle holds: make it the identity
        if source_rate is not None:
            rs = self.resampler(source_rate)
            rs.ensure_loaded()
        elif normalize_dbfs is not None:
            raise ValueError("normalize_dbfs needs source_rate (16000 for waveforms that are at the encoder's rate already)")
        # from the untrimmed 16 kHz lengths: with trim they bound the partials, and the entry reports the trimmed lengths and their counts
        counts = np.asarray([len(compute_partial_slices(rs.output_length(int(k)) if rs else int(k), self.rate, self.min_coverage)[1]) for k in n], np.int32)
        if trim:
            vad = self.trimmer(**(trim if isinstance(trim, dict) else {}))
            vad.ensure_loaded()
        got, n_trimmed = np.empty(len(n), np.int32), np.empty(len(n), np.int32)
        out = np.empty((len(n), self.emb), np.float32) if want_vectors else None
        slices = np.empty((int(counts.sum()), PARTIAL_FRAMES, MEL_N_CHANNELS), np.float32) if want_slices else None
        handles = (self.encoder.h if want_vectors else None, self._dev.h)
        rule = (PARTIAL_FRAMES, self.frame_step, float(self.min_coverage))
        outs = (_ptr(out) if want_vectors else None, _ptr(got), _ptr(slices) if want_slices else None)
        level = (float("nan") if normalize_dbfs is None else float(normalize_dbfs), int(bool(increase_only)))
        if source is None:
            args = (*handles, len(n), _ptr(n), _ptr(packed), *rule)
            entry, level, trimmed = {(False, False): (self.lib.mtts_dvector_embed_wavs, (), ()),
                                     (True, False): (self.lib.mtts_dvector_embed_wavs_resampled, level, ()),
                                     (True, True): (self.lib.mtts_dvector_embed_wavs_preprocessed, level, (_ptr(n_trimmed),))}[rs is not None, vad is not None]
            self._dev.check(entry(*args, *level, *outs, *trimmed))
        else:
            stages = (1 if rs is not None else 0) | (2 if vad is not None else 0)
            self._dev.check(self.lib.mtts_dvector_embed_wavs_source(*handles, C.byref(source), stages, len(n), _ptr(n), *rule, *level, *outs, _ptr(n_trimmed)))
        if vad is None:
            assert np.array_equal(got, counts), (got, counts)   # the device entry and compute_partial_slices state the same rule
        else:
            want = [len(compute_partial_slices(int(k), self.rate, self.min_coverage)[1]) for k in n_trimmed]
            assert np.array_equal(got, want) and np.all(got <= counts), (got, want, counts)
            self.last_trimmed_lengths = n_trimmed
        if not want_slices:
            return out, None
        parts = np.split(slices[: int(got.sum())], np.cumsum(got)[:-1])
        return out, ([s.copy() for s in parts] if vad is not None else parts)   # (copies: not views of a buffer sized for the untrimmed lengths)

    def embed_utterances(self, wavs, return_slices: bool = False, source_rate: Optional[int] = None, normalize_dbfs: Optional[float] = None,
                         increase_only: bool = True, trim=False):
        """`VoiceEncoder.embed_utterance` (rate 1.3, min_coverage 0.75) of a list of 16 kHz float32 waveforms -> (B, emb) float32, every
        row L2-normalised.  One chain of launches per chunk of utterances (as many as fit the encoder's max_partials).
        source_rate: the waveforms are at that rate and are resampled to 16 kHz on the device in front of the same chain (the 16 kHz
        signal never visits the host); normalize_dbfs: and normalised to that level (resemblyzer: -30, increase_only) — the result
        equals `embed_utterances(Resampler.resample_batch(wavs, normalize_dbfs))` bit for bit.
        trim: True (or a dict of audio.vad.SilenceTrimmer keywords): silence trimming behind those two steps, on the device as well — with
        source_rate and normalize_dbfs=-30 all of resemblyzer's `preprocess_wav` (source_rate may be 16000, and is taken as that when
        omitted: the chained entry runs whatever bank the handle holds, so the 16000 -> 16000 identity bank is loaded, a one-tap pass
        that copies every sample as it is — a side effect on the handle's resampler, which `resampler(rate)` users reload by
        themselves before each use); the result equals `embed_utterances(trimmer().trim_batch(resample_batch(...)))` bit for bit, and
        `last_trimmed_lengths` holds the trimmed lengths.  The detector is this project's (parity with webrtcvad unpinned)."""
        if self.encoder is None:
            raise MttsError("SpeakerEmbedder(encoder=False) has no encoder")
        out, slices = self._run(wavs, True, return_slices, source_rate, normalize_dbfs, increase_only, trim)
        return (out, slices) if return_slices else out

    def embed_utterance(self, wav):
        return self.embed_utterances([wav])[0]

    def embed_pcm16(self, wavs, return_slices: bool = False, source_rate: Optional[int] = None, normalize_dbfs: Optional[float] = None,
                    increase_only: bool = True, trim=False):
        """`embed_utterances` for a list of int16 arrays, 16-bit PCM as a .wav file holds it: the samples are uploaded at 2 bytes each and
        widened on the device (x = v / 32768, exact in float32), so the result — vectors, slices, `last_trimmed_lengths` — equals
        `embed_utterances([w.astype(np.float32) / 32768 for w in wavs], ...)` bit for bit.  Same keywords, same return values."""
        if self.encoder is None:
            raise MttsError("SpeakerEmbedder(encoder=False) has no encoder")
        ws = [np.asarray(w) for w in wavs]
        if not ws:
            raise MttsError("no waveforms")
        bad = [str(w.dtype) for w in ws if w.dtype != np.int16]
        if bad:
            raise TypeError(f"embed_pcm16 takes int16 arrays, got {bad[0]} (embed_utterances takes float samples)")
        n = np.asarray([w.size for w in ws], np.int32)
        packed = np.ascontiguousarray(np.concatenate([w.reshape(-1) for w in ws]))
        source = _WavSource(_WavSource.HOST_PCM16, packed.ctypes.data, 0, None, 0.0)
        out, slices = self._chain(n, packed, source, True, return_slices, source_rate, normalize_dbfs, increase_only, trim)
        return (out, slices) if return_slices else out

    def embed_device(self, ptr: int, row_stride: int, lengths, *, stream: int = 0, quantize: Optional[float] = None, source_rate: Optional[int] = None,
                     normalize_dbfs: Optional[float] = None, increase_only: bool = True, trim=False):
        """`embed_utterances` for float32 waveforms that are in device memory already: utterance u is the first lengths[u] floats of the
        row at `ptr + 4 * u * row_stride` (what lies behind them in a row is never read) -> (B, emb) float32.  `stream`: the HIP stream
        whose work fills the rows (`MelGAN.infer_device` returns its own); the front-end waits for it on the device, the host does not.
        quantize: `max_wav_value` — every sample first goes through what writing it to a 16-bit file and reading it back does,
        trunc(x * quantize) / 32768, so the result equals `embed_pcm16` of `(wav * max_wav_value).astype("int16")`; None: the floats as
        they are.  The other keywords are `embed_utterances`'."""
        if self.encoder is None:
            raise MttsError("SpeakerEmbedder(encoder=False) has no encoder")
        n = np.ascontiguousarray(lengths, dtype=np.int32).reshape(-1)
        if not len(n):
            raise MttsError("no waveforms")
        source = _WavSource(_WavSource.DEVICE_F32, int(ptr), int(row_stride), int(stream) or None, 0.0 if quantize is None else float(quantize))
        return self._chain(n, None, source, True, False, source_rate, normalize_dbfs, increase_only, trim)[0]

    def reference_mel_slices(self, wav, source_rate: Optional[int] = None, normalize_dbfs: Optional[float] = None, trim=False) -> np.ndarray:
        """The `spk_ref_mel_slices` payload of preprocessor.py:263-299 for one waveform: (n_partials, 160, 40) float32.  source_rate,
        normalize_dbfs, trim: as in `embed_utterances`."""
        return self._run([wav], False, True, source_rate, normalize_dbfs, True, trim)[1][0]

    # ---- scoring kernels ---------------------------------------------------------------------------------------------------------
    def _scorer(self):
        if self.encoder is None:
            raise MttsError("scoring runs on the encoder's handle: SpeakerEmbedder(encoder=False) has none")
        return self.encoder

    def cosine_similarity(self, a, b, index_a=None, index_b=None, eps: float = 1e-6) -> np.ndarray:
        """nn.CosineSimilarity(dim=1, eps) of a[index_a[i]] and b[index_b[i]] (default: row i of each) -> float32 [n]."""
        enc = self._scorer()
        a, b = np.ascontiguousarray(np.asarray(a, np.float32)), np.ascontiguousarray(np.asarray(b, np.float32))
        ia = np.ascontiguousarray(np.arange(len(a)) if index_a is None else index_a, dtype=np.int32)
        ib = np.ascontiguousarray(np.arange(len(b)) if index_b is None else index_b, dtype=np.int32)
        if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[1] or len(ia) != len(ib):
            raise ValueError(f"cosine_similarity: shapes {a.shape} {b.shape}, {len(ia)} / {len(ib)} indices")
        sim = np.empty(len(ia), np.float32)
        enc._check(self.lib.mtts_dvector_cosine_indexed(enc.h, _ptr(a), len(a), _ptr(b), len(b), a.shape[1], len(ia), _ptr(ia), _ptr(ib), float(eps), _ptr(sim)))
        return sim

    def centroids(self, enrollment_list) -> np.ndarray:
        """wavs_to_dvector.py:176-183: per speaker, the mean of its (ragged) list of d-vectors, L2-normalised -> (n_speaker, dim) float32."""
        enc = self._scorer()
        lists = [np.asarray(v, np.float32).reshape(len(v), -1) for v in enrollment_list]
        off = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(v) for v in lists])]), dtype=np.int32)
        vecs = np.ascontiguousarray(np.concatenate(lists, axis=0))
        out = np.empty((len(lists), vecs.shape[1]), np.float32)
        enc._check(self.lib.mtts_dvector_centroids(enc.h, _ptr(vecs), _ptr(off), len(lists), vecs.shape[1], _ptr(out)))
        return out


def read_wav_16k(path: str) -> np.ndarray:
    """`preprocessor.read_wav` (signed PCM scaled by its full range, unsigned 8-bit re-centred, float as it is, channels averaged)
    for a file that must be 16 kHz."""
    from .preprocessor import read_wav
    wav, rate = read_wav(path)
    if int(rate) != SAMPLING_RATE:
        raise MttsError(f"{path}: sampling rate {rate}, the speaker encoder takes {SAMPLING_RATE} Hz (no resampling here: pass a wav_loader that resamples)")
    return wav


def embed_synthesized(engine, vocoder, embedder: SpeakerEmbedder, slot: int, task: int, mel_lens, max_wav_value: float, **chain) -> np.ndarray:
    """The d-vectors of a test step's synthesis without a waveform leaving the device: `engine.mel_device(slot, task)` (the post-net mel
    of the last forward / synthesize) -> `vocoder.infer_device` -> `embedder.embed_device(quantize=max_wav_value, ...)`, which puts every
    sample through the 16-bit cut of `MelGAN.infer` before it is scored — the vectors are those of writing the `Saver`'s .synth.wav
    files and reading them back.  mel_lens [B]: the synthesised frames per utterance (`engine.durations(slot, task)[1]`).  `chain`:
    `embed_device`'s keywords; source_rate is the preprocess config's sampling rate (the vocoder's output rate) and is required.
    The `Saver` still writes its files; this only spares the evaluation the trip through them."""
    if "source_rate" not in chain:
        raise ValueError("embed_synthesized needs source_rate=<the preprocess config's sampling rate>: the vocoder does not synthesise at the encoder's 16 kHz")
    mel_lens = np.asarray(mel_lens).reshape(-1)
    ptr, t_cap, stride = engine.mel_device(slot, task, postnet=True)
    wav_ptr, row_stride, lengths, stream = vocoder.infer_device(ptr, stride, len(mel_lens), t_cap, mel_lens)
    return embedder.embed_device(wav_ptr, row_stride, lengths, stream=stream, quantize=max_wav_value, **chain)


# ---- the reference's class surface -----------------------------------------------------------------------------------------------------
class EvalConfig:
    """What evaluation/config.py holds: `corpus`, `data_dir_dict` ('recon', 'real', 'enrollment' and one entry per mode),
    `n_speaker`, `n_sample`, `mode_step_list` = [(mode, [steps])], and `work_dir` under which npy/<corpus>/, json/<corpus>/ and
    txt/<corpus>/ are written (the reference writes them under its working directory).  Optional, for `VisualizeDvector`:
    `tsne_mode_list`, `tsne_pseudo_speaker_list`, `tsne_legend_list`, `tsne_plot_color_list`."""

    def __init__(self, corpus: str, data_dir_dict: Dict[str, str], n_speaker: int, n_sample: int, mode_step_list, work_dir: str = ".",
                 tsne_mode_list=(), tsne_pseudo_speaker_list=(), tsne_legend_list=(), tsne_plot_color_list=()):
        self.corpus, self.data_dir_dict, self.n_speaker, self.n_sample = corpus, dict(data_dir_dict), int(n_speaker), int(n_sample)
        self.mode_step_list = [(m, list(s)) for m, s in mode_step_list]
        self.work_dir = work_dir
        # visualize.py's four (config.py:142-150 and the per-corpus tsne_pseudo_speaker_list); only VisualizeDvector reads them
        self.tsne_mode_list, self.tsne_pseudo_speaker_list = list(tsne_mode_list), list(tsne_pseudo_speaker_list)
        self.tsne_legend_list, self.tsne_plot_color_list = list(tsne_legend_list), list(tsne_plot_color_list)

    def path(self, kind: str, name: str) -> str:
        d = os.path.join(self.work_dir, kind, self.corpus)
        os.makedirs(d, exist_ok=True)
        return os.path.join(d, name)


def _testing_dir(data_dir: str) -> str:
    d = os.path.join(data_dir, "audio/Testing/step_100000")          # wavs_to_dvector.py:247-250
    return d if os.path.exists(d) else os.path.join(data_dir, "audio/Testing")


class WavsToDvector:
    """wavs_to_dvector.py: every wav of a test run -> d-vectors, saved as npy/<corpus>/<mode>_dvector.npy (an existing file is loaded
    instead, as in the reference).  `wav_loader(path) -> 16 kHz float32 waveform` (default: `read_wav_16k`).  All wavs of a mode go to
    the device in one `embed_utterances` call.  resample=True: files of any rate (a result tree's 22 050 Hz wavs) are read with
    `preprocessor.read_wav`, grouped by rate, and each group is resampled to 16 kHz and normalised to `normalize_dbfs` (resemblyzer's
    `preprocess_wav`; None: not normalised) on the device in front of the encoder, one call per group.  trim=True: and trimmed of long
    silences there (`embed_utterances(trim=True)`; this project's detector, parity with webrtcvad unpinned); default off.
    pcm16=True (default off): the files are read here as well, and mono 16-bit PCM files stay int16 and go through `embed_pcm16` — half
    the bytes on the host and in the upload, the same d-vectors bit for bit; files of any other sample format take the float path."""

    def __init__(self, config: EvalConfig, embedder: SpeakerEmbedder, wav_loader: Optional[Callable[[str], np.ndarray]] = None, pair_list=None,
                 rng: Optional[random.Random] = None, run: bool = True, resample: bool = False, normalize_dbfs: Optional[float] = -30.0, trim=False,
                 pcm16: bool = False):
        self.config, self.embedder = config, embedder
        self.resample, self.normalize_dbfs, self.trim, self.pcm16 = bool(resample), normalize_dbfs, trim, bool(pcm16)
        if (resample or pcm16) and wav_loader is not None:
            raise ValueError("WavsToDvector(resample=True) and WavsToDvector(pcm16=True) read the files themselves: wav_loader must be None")
        self.corpus, self.data_dir_dict = config.corpus, config.data_dir_dict
        self.n_sample, self.n_speaker, self.mode_step_list = config.n_sample, config.n_speaker, config.mode_step_list
        self.wav_loader = wav_loader or read_wav_16k
        self.rng = rng or random.Random()
        with open(os.path.join(self.data_dir_dict["recon"], "test_SQids.json")) as f:
            self.sq_list = json.load(f)
        self.speaker_id_map, self.inv_speaker_id_map = self.get_speaker_id_map()
        self.enrollment_filelist = self.get_enrollment_filelist()
        self.real_filelist = self.get_real_filelist()
        pair_json = config.path("json", "pair.json")
        if pair_list is not None:
            self.pair_list = pair_list
        elif os.path.exists(pair_json):
            with open(pair_json) as f:
                self.pair_list = json.load(f)
        else:
            self.pair_list = self.get_and_save_pair_list()
        if run:
            self.dvector_list_dict = self.get_dvector()

    def files_to_dvectors(self, paths: Sequence[str]) -> np.ndarray:
        if not self.resample and not self.pcm16:
            return self.embedder.embed_utterances([self.wav_loader(p) for p in paths], trim=self.trim)
        from .preprocessor import read_wav
        groups: Dict[tuple, List[int]] = {}   # (rate, held as int16) -> files
        wavs = []
        for i, p in enumerate(paths):
            wav, rate = read_wav(p, keep_pcm16=self.pcm16)
            if not self.resample and int(rate) != SAMPLING_RATE:
                raise MttsError(f"{p}: sampling rate {rate}, the speaker encoder takes {SAMPLING_RATE} Hz (WavsToDvector(resample=True) resamples)")
            wavs.append(wav)
            groups.setdefault((int(rate), wav.dtype == np.int16), []).append(i)
        if not wavs:
            raise MttsError("no waveforms")
        out = np.empty((len(wavs), self.embedder.emb), np.float32)
        for (rate, pcm), idx in sorted(groups.items()):
            embed = self.embedder.embed_pcm16 if pcm else self.embedder.embed_utterances
            chain = dict(source_rate=rate, normalize_dbfs=self.normalize_dbfs) if self.resample else {}
            out[idx] = embed([wavs[i] for i in idx], trim=self.trim, **chain)
        return out

    def get_speaker_id_map(self):
        fwd, inv = {}, {}
        for speaker_id in range(self.n_speaker):
            real = str(self.sq_list[speaker_id * self.n_sample]["qry_id"][0].split("_")[0])
            fwd[speaker_id], inv[real] = real, speaker_id
        return fwd, inv

    def get_enrollment_filelist(self):
        """All real wavs of each speaker (the reference takes a set; sorted here so that a run is reproducible)."""
        out = []
        for speaker_id in range(self.n_speaker):
            wav_dir = os.path.join(self.data_dir_dict["enrollment"], self.speaker_id_map[speaker_id])
            out.append([os.path.join(wav_dir, f) for f in sorted(os.listdir(wav_dir)) if f.endswith(".wav")])
        return out

    def get_real_filelist(self):
        out = []
        for speaker_id in range(self.n_speaker):
            for sample_id in range(self.n_sample):
                q = self.sq_list[speaker_id * self.n_sample + sample_id]
                out.append(os.path.join(self.data_dir_dict["real"], self.speaker_id_map[speaker_id], q["qry_id"][0] + ".wav"))
        return out

    def get_and_save_pair_list(self):
        """wavs_to_dvector.py:137-168: per test sample 4 positive files (the speaker's own) and 4 negative ones (one of each of 4 others)."""
        pair_list = [dict() for _ in range(self.n_speaker * self.n_sample)]
        for speaker_id in range(self.n_speaker):
            for sample_id in range(self.n_sample):
                data_id = speaker_id * self.n_sample + sample_id
                pair_list[data_id]["p"] = [os.path.basename(p) for p in self.rng.sample(self.enrollment_filelist[speaker_id], 4)]
                others = self.rng.sample([i for i in range(self.n_speaker) if i != speaker_id], 4)
                pair_list[data_id]["n"] = [os.path.basename(self.rng.sample(self.enrollment_filelist[s], 1)[0]) for s in others]
        with open(self.config.path("json", "pair.json"), "w", encoding="utf8") as fp:
            json.dump(pair_list, fp)
        return pair_list

    def get_centroid_dvector_list(self, enrollment_list):
        return self.embedder.centroids(enrollment_list)

    def get_pair_dvector_list(self):
        pos, neg = [], []
        for data_id in range(self.n_speaker * self.n_sample):
            pos += self.pair_list[data_id]["p"]
            neg += self.pair_list[data_id]["n"]
        path_of = lambda f: os.path.join(self.data_dir_dict["real"], f.split("_")[0], f)   # noqa: E731
        both = self.files_to_dvectors([path_of(f) for f in pos + neg])
        return np.stack([both[: len(pos)], both[len(pos):]])

    def get_enrollment_dvector_list(self):
        flat = self.files_to_dvectors([p for files in self.enrollment_filelist for p in files])
        cuts = np.cumsum([len(files) for files in self.enrollment_filelist])[:-1]
        out = np.empty(self.n_speaker, object)
        out[:] = np.split(flat, cuts)
        return out

    def get_real_dvector_list(self):
        return self.files_to_dvectors(self.real_filelist)

    def _find(self, wav_dir: str, suffix: str) -> Optional[str]:
        for wav_file in sorted(os.listdir(wav_dir)):     # (the reference takes the first os.listdir hit; a task directory holds one)
            if wav_file.endswith(suffix):
                return os.path.join(wav_dir, wav_file)
        return None

    def get_recon_dvector_list(self, data_dir: str):
        root = _testing_dir(data_dir)
        paths = [self._find(os.path.join(root, f"test_{data_id:03d}"), "recon.wav") for data_id in range(self.n_speaker * self.n_sample)]
        return self.files_to_dvectors([p for p in paths if p is not None])

    def get_syn_dvector_list(self, data_dir: str, step: int = 10):
        """wavs_to_dvector.py:266-301, including the 1-shot layout test_###_0 .. test_###_4."""
        root, paths = _testing_dir(data_dir), []
        for data_id in range(self.n_speaker * self.n_sample):
            d = os.path.join(root, f"test_{data_id:03d}")
            if os.path.exists(d):
                dirs = [d]
            else:
                assert os.path.exists(d + "_0"), d
                dirs = [f"{d}_{i}" for i in range(5)]
            for wav_dir in dirs:
                p = self._find(wav_dir, f"FTstep_{step}.synth.wav")
                if p is not None:
                    paths.append(p)
        return self.files_to_dvectors(paths)

    def get_dvector(self):
        d = {}
        makers = {"enrollment": self.get_enrollment_dvector_list, "centroid": lambda: self.get_centroid_dvector_list(d["enrollment"]),
                  "pair": self.get_pair_dvector_list, "real": self.get_real_dvector_list,
                  "recon": lambda: self.get_recon_dvector_list(self.data_dir_dict["recon"])}
        for mode in ["enrollment", "centroid", "pair", "real", "recon"]:
            path = self.config.path("npy", f"{mode}_dvector.npy")
            if os.path.exists(path):
                d[mode] = np.load(path, allow_pickle=True)
            else:
                d[mode] = makers[mode]()
                np.save(path, d[mode], allow_pickle=True)
        for mode, steps in self.mode_step_list:
            for step in steps:
                path = self.config.path("npy", f"{mode}_step{step}_dvector.npy")
                if os.path.exists(path):
                    d[f"{mode}_step{step}"] = np.load(path, allow_pickle=True)
                else:
                    d[f"{mode}_step{step}"] = self.get_syn_dvector_list(self.data_dir_dict[mode], step)
                    np.save(path, d[f"{mode}_step{step}"], allow_pickle=True)
        return d


class PairSimilarity:
    """pair_similarity.py: cosine similarity of every test d-vector with its 4 positive and 4 negative enrollment d-vectors."""

    def __init__(self, config: EvalConfig, embedder: SpeakerEmbedder):
        self.config, self.embedder = config, embedder
        self.corpus, self.mode_step_list = config.corpus, config.mode_step_list
        self.dvector_list_dict, self.pair_similarity_dict = {}, {}

    def _modes(self):
        return ["recon", "real"] + [f"{m}_step{s}" for m, steps in self.mode_step_list for s in steps]

    def load_dvector(self):
        for mode in ["pair"] + self._modes():
            self.dvector_list_dict[mode] = np.load(self.config.path("npy", f"{mode}_dvector.npy"), allow_pickle=True)

    def compute_pair_similarity(self, check_list) -> np.ndarray:
        """pair_similarity.py:68-88 -> [2, 4 * len(check_list)] (positive row, negative row).  The reference's np.repeat(check_list, 4)
        and, in the five-fold layout, np.repeat(pair, 5, axis=1) are index arrays here."""
        check = np.asarray(check_list, np.float32)
        pair = np.asarray(self.dvector_list_dict["pair"], np.float32)
        n = 4 * len(check)
        it = np.arange(n, dtype=np.int32) // 4
        if n == pair.shape[1]:
            ip = np.arange(n, dtype=np.int32)
        else:
            assert n == pair.shape[1] * 5, (n, pair.shape)
            ip = np.arange(n, dtype=np.int32) // 5
        return np.stack([self.embedder.cosine_similarity(check, pair[0], it, ip), self.embedder.cosine_similarity(check, pair[1], it, ip)])

    def get_pair_similarity(self):
        for mode in self._modes():
            path = self.config.path("npy", f"{mode}_pair_sim.npy")
            if os.path.exists(path):
                self.pair_similarity_dict[mode] = np.load(path, allow_pickle=True)
            else:
                self.pair_similarity_dict[mode] = self.compute_pair_similarity(self.dvector_list_dict[mode])
                np.save(path, self.pair_similarity_dict[mode], allow_pickle=True)

    def save_pair_similarity(self):
        np.save(self.config.path("npy", "pair_similarity.npy"), self.pair_similarity_dict, allow_pickle=True)

    def load_pair_similarity(self):
        self.pair_similarity_dict = np.load(self.config.path("npy", "pair_similarity.npy"), allow_pickle=True)[()]


def check_shuffle_map(map_list, n_speaker: int, n_sample: int):
    """The invariants centroid_similarity.py:160-168 asserts: no sample is mapped to its own speaker's centroid, and every speaker's
    centroid is drawn exactly n_sample times."""
    m = np.asarray(map_list).reshape(-1)
    if len(m) != n_speaker * n_sample or m.min() < 0 or m.max() >= n_speaker * n_sample:
        raise ValueError("shuffle map: wrong length or index out of range")
    spk = m // n_sample
    if np.any(spk == np.arange(len(m)) // n_sample):
        raise ValueError("shuffle map: a sample is mapped to its own speaker's centroid")
    if np.any(np.bincount(spk, minlength=n_speaker) != n_sample):
        raise ValueError("shuffle map: a speaker's centroid is not drawn n_sample times")


def custom_shuffle_map(n_speaker: int, n_sample: int, rng: Optional[random.Random] = None) -> List[int]:
    """centroid_similarity.py:134-159: a cross-speaker index map (into the n_sample-times repeated centroids), re-drawn until the last
    speaker still has n_sample foreign slots to draw from."""
    rng = rng or random.Random()
    if n_speaker < 2:
        raise ValueError("recon_random needs at least two speakers")
    while True:
        map_list, count, ok = [0] * (n_speaker * n_sample), [0] * n_speaker, True
        for i in range(n_speaker):
            pool = [j for j in range(n_speaker) if j != i for _ in range(n_sample - count[j])]
            if len(pool) < n_sample:
                ok = False
                break
            for t, tgt in enumerate(rng.sample(pool, n_sample)):
                map_list[i * n_sample + t] = tgt * n_sample + count[tgt]
                count[tgt] += 1
        if ok:
            check_shuffle_map(map_list, n_speaker, n_sample)
            return map_list


class CentroidSimilarity:
    """centroid_similarity.py: cosine similarity of every test d-vector with its speaker's centroid, plus `recon_random` (recon
    d-vectors against other speakers' centroids through a cross-speaker index map, supplied or generated)."""

    def __init__(self, config: EvalConfig, embedder: SpeakerEmbedder, shuffle_map=None, rng: Optional[random.Random] = None):
        self.config, self.embedder = config, embedder
        self.n_speaker, self.n_sample, self.mode_step_list = config.n_speaker, config.n_sample, config.mode_step_list
        self.shuffle_map = shuffle_map if shuffle_map is not None else custom_shuffle_map(self.n_speaker, self.n_sample, rng)
        check_shuffle_map(self.shuffle_map, self.n_speaker, self.n_sample)
        self.dvector_list_dict, self.similarity_list_dict = {}, {}

    def load_dvector(self):
        for mode in ["recon", "centroid", "real"] + [f"{m}_step{s}" for m, steps in self.mode_step_list for s in steps]:
            self.dvector_list_dict[mode] = np.load(self.config.path("npy", f"{mode}_dvector.npy"), allow_pickle=True)

    def compute_centroid_similarity(self, mode: str) -> np.ndarray:
        cent = np.asarray(self.dvector_list_dict["centroid"], np.float32)
        if mode == "recon_random":        # :77-80: shuffled, n_sample-times repeated centroids vs recon
            test = np.asarray(self.dvector_list_dict["recon"], np.float32)
            ic = np.asarray(self.shuffle_map, np.int32) // self.n_sample
        else:
            test = np.asarray(self.dvector_list_dict[mode], np.float32)
            per = self.n_sample if len(test) == self.n_speaker * self.n_sample else 5 * self.n_sample   # :101-110 (five-fold layout)
            assert len(test) == self.n_speaker * per, (len(test), self.n_speaker, per)
            ic = np.arange(len(test), dtype=np.int32) // per
        return self.embedder.cosine_similarity(cent, test, ic, np.arange(len(test), dtype=np.int32))

    def get_centroid_similarity(self):
        for mode in ["recon_random", "recon"] + [f"{m}_step{s}" for m, steps in self.mode_step_list for s in steps]:
            path = self.config.path("npy", f"{mode}_centroid_sim.npy")
            if os.path.exists(path):
                self.similarity_list_dict[mode] = np.load(path, allow_pickle=True)
            else:
                self.similarity_list_dict[mode] = self.compute_centroid_similarity(mode)
                np.save(path, self.similarity_list_dict[mode], allow_pickle=True)

    def save_centroid_similarity(self):
        np.save(self.config.path("npy", "centroid_similarity_dict.npy"), self.similarity_list_dict, allow_pickle=True)


# ---- DET / ROC on the host (sklearn.metrics restated: _binary_clf_curve, det_curve, roc_curve(drop_intermediate=True), auc) ------------
def _binary_clf_curve(y_true, y_score):
    y_true, y_score = np.asarray(y_true).reshape(-1) == 1, np.asarray(y_score).reshape(-1)
    order = np.argsort(y_score, kind="mergesort")[::-1]
    y_score, y_true = y_score[order], y_true[order]
    threshold_idxs = np.r_[np.where(np.diff(y_score))[0], y_true.size - 1]
    tps = np.cumsum(y_true * 1.0, dtype=np.float64)[threshold_idxs]
    fps = 1 + threshold_idxs - tps
    return fps, tps, y_score[threshold_idxs]


def det_curve(y_true, y_score, drop_intermediate: bool = False):
    """(fpr, fnr, thresholds), false positives decreasing (sklearn 1.7's det_curve; drop_intermediate=False is its default and
    what the reference's call gets)."""
    if len(np.unique(np.asarray(y_true))) != 2:
        raise ValueError("Only one class is present in y_true. Detection error tradeoff curve is not defined in that case.")
    fps, tps, thresholds = _binary_clf_curve(y_true, y_score)
    # a threshold at inf where everything is predicted negative (tps = fps = 0)
    tps, fps, thresholds = np.concatenate(([0], tps)), np.concatenate(([0], fps)), np.concatenate(([np.inf], thresholds))
    if drop_intermediate and len(fps) > 2:
        keep = np.where(np.concatenate([[True], np.logical_or(np.diff(tps[:-1]), np.diff(tps[1:])), [True]]))[0]
        fps, tps, thresholds = fps[keep], tps[keep], thresholds[keep]
    fns = tps[-1] - tps
    p_count, n_count = tps[-1], fps[-1]
    first_ind = fps.searchsorted(fps[0], side="right") - 1 if fps.searchsorted(fps[0], side="right") > 0 else None
    last_ind = tps.searchsorted(tps[-1]) + 1
    sl = slice(first_ind, last_ind)
    return fps[sl][::-1] / n_count, fns[sl][::-1] / p_count, thresholds[sl][::-1]


def roc_curve(y_true, y_score):
    fps, tps, thresholds = _binary_clf_curve(y_true, y_score)
    if len(fps) > 2:
        keep = np.where(np.r_[True, np.logical_or(np.diff(fps, 2), np.diff(tps, 2)), True])[0]
        fps, tps, thresholds = fps[keep], tps[keep], thresholds[keep]
    tps, fps, thresholds = np.r_[0, tps], np.r_[0, fps], np.r_[np.inf, thresholds]
    return fps / fps[-1], tps / tps[-1], thresholds


def auc(x, y) -> float:
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    dx = np.diff(x)
    direction = 1
    if np.any(dx < 0):
        if not np.all(dx <= 0):
            raise ValueError("x is neither increasing nor decreasing")
        direction = -1
    trapezoid = getattr(np, "trapezoid", None) or np.trapz
    return float(direction * trapezoid(y, x))


def equal_error_rate(y_true, y_score, drop_intermediate: bool = False):
    """(EER, threshold) as speaker_verification.py:32-59 reads them off the DET curve: the point where |fpr - fnr| is smallest, the mean of
    the two rates there.  The one routine behind SpeakerVerification.get_eer and the batch EER of ge2e.GE2ETrainer."""
    fpr, fnr, thresholds = det_curve(y_true, y_score, drop_intermediate)
    min_index = np.argmin(np.abs(fpr - fnr))
    return np.mean((fpr[min_index], fnr[min_index])), thresholds[min_index]


class SpeakerVerification:
    """speaker_verification.py:32-59 (EER and its threshold per mode from the pair similarities, written to txt/<corpus>/<output>)
    and :281-315 (AUC per mode: real positives against the mode's positives)."""

    def __init__(self, config: EvalConfig, output_path: str = "eer.txt", det_drop_intermediate: bool = False):
        self.config = config
        self.output_path = config.path("txt", output_path)
        self.det_drop_intermediate = det_drop_intermediate
        self.pair_similarity_dict, self.threshold_dict, self.eer_dict, self.auc_dict = {}, {}, {}, {}

    def load_pair_similarity(self):
        self.pair_similarity_dict = np.load(self.config.path("npy", "pair_similarity.npy"), allow_pickle=True)[()]

    def get_eer(self, write: bool = True):
        for mode, s_list in self.pair_similarity_dict.items():
            y_score = s_list.flatten()
            y_true = np.ones_like(s_list)
            y_true[1, :] = 0
            self.eer_dict[mode], self.threshold_dict[mode] = equal_error_rate(y_true.flatten(), y_score, self.det_drop_intermediate)
        if write:
            with open(self.output_path, "w+") as f:
                for mode in self.pair_similarity_dict:
                    f.write(mode + ":\n")
                    f.write(f"threshold:{self.threshold_dict[mode]:.4f}\t")
                    f.write(f"EER:{self.eer_dict[mode]:.4f}\n")
        return self.eer_dict

    def get_auc(self):
        real_score = self.pair_similarity_dict["real"][0]
        for mode, s_list in self.pair_similarity_dict.items():
            if s_list.shape[1] != len(real_score):   # the reference's labels assume as many real scores as mode scores (not the five-fold layout)
                continue
            y_score = np.concatenate([real_score, s_list[0]])
            y_true = np.repeat(np.array([1, 0]), s_list.shape[1])
            fpr, tpr, _ = roc_curve(y_true, y_score)
            self.auc_dict[mode] = auc(fpr, tpr)
        return self.auc_dict


# ---- t-SNE of d-vectors (evaluation/visualize.py) ------------------------------------------------------------------------------------------
class TSNE:
    """sklearn.manifold.TSNE's surface for what the reference uses, on csrc/tsne.h: two components, squared Euclidean distances, and
    the EXACT gradient (sklearn's method="exact") where the reference's call gets Barnes-Hut.  `n_iter=` is accepted as the alias of
    `max_iter=` that it was before sklearn 1.7.  The schedule is sklearn 1.7's `_tsne` / `_gradient_descent`, driven from the host in
    chunks of 50 iterations: 250 exploration iterations at momentum 0.5 on early_exaggeration x P, the rest at momentum 0.8, update and
    gains starting afresh in each phase; every 50 iterations the KL divergence and the gradient norm come back and the run stops after
    `n_iter_without_progress` iterations without a new best KL or at a gradient norm <= `min_grad_norm`.  `n_iter_` is sklearn's (the
    index of the last iteration).  One deliberate difference: sklearn's `kl_divergence_` is the KL of the state its last iteration
    STARTED from; here it is the KL of `embedding_` itself (one more pass over the pairs)."""

    _EXPLORATION_MAX_ITER = 250
    _N_ITER_CHECK = 50
    MAX_POINTS = 12288     # csrc/tsne.h TSNE_MAX_POINTS: the dense P is n^2 x 4 bytes (298 MB at 8 640 points, 604 MB at the cap)

    def __init__(self, n_components: int = 2, *, perplexity: float = 30.0, early_exaggeration: float = 12.0, learning_rate="auto", max_iter: Optional[int] = None,
                 n_iter: Optional[int] = None, n_iter_without_progress: int = 300, min_grad_norm: float = 1e-7, init="pca", random_state=None,
                 device: int = 0, lib_path=None):
        if n_components != 2:
            raise ValueError(f"TSNE: n_components={n_components}: only 2 components are built (the pair kernel is written for two)")
        if max_iter is not None and n_iter is not None:
            raise ValueError("TSNE: give max_iter or its alias n_iter, not both")
        max_iter = 1000 if max_iter is None and n_iter is None else int(n_iter if max_iter is None else max_iter)
        if max_iter < 250:
            raise ValueError(f"TSNE: max_iter={max_iter} must be at least 250")
        if not (isinstance(init, np.ndarray) or init in ("pca", "random")):
            raise ValueError(f"TSNE: init={init!r}: 'pca', 'random' or an ndarray of shape (n, 2)")
        if not (learning_rate == "auto" or float(learning_rate) > 0):
            raise ValueError(f"TSNE: learning_rate={learning_rate!r}: 'auto' or a positive number")
        self.n_components, self.perplexity, self.early_exaggeration = 2, float(perplexity), float(early_exaggeration)
        self.learning_rate, self.max_iter, self.n_iter_without_progress = learning_rate, max_iter, int(n_iter_without_progress)
        self.min_grad_norm, self.init, self.random_state = float(min_grad_norm), init, random_state
        self.device, self.lib_path = device, lib_path
        self.min_gain = 0.01

    # ---- host pieces ---------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def auto_learning_rate(n: int, early_exaggeration: float) -> float:
        return float(max(n / early_exaggeration / 4, 50))

    @staticmethod
    def pca_init(X) -> np.ndarray:
        """sklearn's init="pca": the first two principal components (float64 SVD of the centred data), as float32, rescaled so that PC1
        has standard deviation 1e-4.  Signs as sklearn 1.7's PCA fixes them, `svd_flip(U, Vt, u_based_decision=False)`: the entry of
        largest magnitude in each RIGHT singular vector (a row of Vt) is positive."""
        X = np.asarray(X, np.float64)
        U, S, Vt = np.linalg.svd(X - X.mean(0), full_matrices=False)
        U, Vt = U[:, :2], Vt[:2]
        signs = np.sign(Vt[np.arange(2), np.abs(Vt).argmax(1)])
        signs[signs == 0] = 1
        emb = (U * signs * S[:2]).astype(np.float32)
        return emb / np.std(emb[:, 0]) * 1e-4

    def _initial(self, X) -> np.ndarray:
        n = len(X)
        if isinstance(self.init, np.ndarray):
            if self.init.shape != (n, 2):
                raise ValueError(f"TSNE: init has shape {self.init.shape}, expected {(n, 2)}")
            return np.ascontiguousarray(self.init, np.float32)
        if self.init == "pca":
            return np.ascontiguousarray(self.pca_init(X), np.float32)
        rs = self.random_state if isinstance(self.random_state, np.random.RandomState) else np.random.RandomState(self.random_state)
        return np.ascontiguousarray(1e-4 * rs.standard_normal(size=(n, 2)).astype(np.float32))

    def _schedule(self, run: Callable, restart: Callable):
        """TSNE._tsne over `run(n_iter, exaggeration, momentum) -> (kl, grad_norm)` (both of the chunk's last iteration) and
        `restart()` (update = 0, gains = 1 on the current embedding) -> (sklearn's `error` of the last phase, n_iter_)."""
        def descend(it, max_iter, momentum, exaggeration, n_iter_without_progress):
            error = best_error = np.finfo(float).max
            best_iter = i = it
            while i < max_iter:
                last = min((i // self._N_ITER_CHECK + 1) * self._N_ITER_CHECK, max_iter) - 1     # the next check, or the last iteration
                error, grad_norm = run(last - i + 1, exaggeration, momentum)
                i = last
                if (i + 1) % self._N_ITER_CHECK == 0:
                    if error < best_error:
                        best_error, best_iter = error, i
                    elif i - best_iter > n_iter_without_progress:
                        break
                    if grad_norm <= self.min_grad_norm:
                        break
                i += 1
            return error, min(i, max_iter - 1) if max_iter > it else it

        restart()
        error, it = descend(0, self._EXPLORATION_MAX_ITER, 0.5, self.early_exaggeration, self._EXPLORATION_MAX_ITER)
        if it < self._EXPLORATION_MAX_ITER or self.max_iter - self._EXPLORATION_MAX_ITER > 0:
            restart()
            error, it = descend(it + 1, self.max_iter, 0.8, 1.0, self.n_iter_without_progress)
        return error, it

    # ---- the device ------------------------------------------------------------------------------------------------------------------------
    def fit_transform(self, X, y=None) -> np.ndarray:
        from . import _lib
        X = np.ascontiguousarray(np.asarray(X), dtype=np.float32)
        if X.ndim != 2:
            raise ValueError(f"TSNE: X has shape {X.shape}, expected (n, dim)")
        n, dim = X.shape
        if n < 2:
            raise ValueError(f"TSNE: {n} point(s): at least 2 are needed")
        if self.perplexity >= n:
            raise ValueError(f"perplexity ({self.perplexity}) must be less than n_samples ({n})")
        if n > self.MAX_POINTS:
            raise ValueError(f"TSNE: n_samples={n} exceeds the cap of {self.MAX_POINTS} points (the dense P would be {n * n * 4 >> 20} MB; Barnes-Hut is not built)")
        if not np.isfinite(X).all():
            raise ValueError("TSNE: X holds a non-finite value")
        self.learning_rate_ = self.auto_learning_rate(n, self.early_exaggeration) if self.learning_rate == "auto" else float(self.learning_rate)
        Y0 = self._initial(X)
        lib = _lib.load(self.lib_path)
        h = C.c_void_p()
        if lib.mtts_tsne_create(n, dim, self.device, C.byref(h)) != 0:
            raise MttsError(lib.mtts_tsne_last_error(None).decode())

        def check(rc):
            if rc != 0:
                raise MttsError(lib.mtts_tsne_last_error(h).decode())

        try:
            check(lib.mtts_tsne_affinities(h, _ptr(X), n, dim, self.perplexity, None, None))
            check(lib.mtts_tsne_set_state(h, _ptr(Y0), None, None))
            Y = np.empty((n, 2), np.float32)

            def run(k, exaggeration, momentum):
                kl, gn = C.c_double(), C.c_double()
                check(lib.mtts_tsne_run(h, k, exaggeration, momentum, self.learning_rate_, self.min_gain, C.byref(kl), C.byref(gn)))
                return kl.value, gn.value

            def restart():
                check(lib.mtts_tsne_get_state(h, _ptr(Y), None, None))
                check(lib.mtts_tsne_set_state(h, _ptr(Y), None, None))

            _, self.n_iter_ = self._schedule(run, restart)
            grad, kl = np.empty((n, 2), np.float32), C.c_double()
            check(lib.mtts_tsne_gradient(h, 1.0, _ptr(grad), C.byref(kl)))
            check(lib.mtts_tsne_get_state(h, _ptr(Y), None, None))
        finally:
            lib.mtts_tsne_destroy(h)
        self.embedding_, self.kl_divergence_ = Y, kl.value
        return Y

    def fit(self, X, y=None):
        self.fit_transform(X)
        return self


class VisualizeDvector:
    """visualize.py without the figure: `load_dvector`, `tsne`, `get_speaker_dvectors`, `get_speaker_id_list_dict`, and in place of
    `visualize_dvector` the table it hands to seaborn (`scatter_table`, `save_table`).  `tsne`: a `TSNE` (default: the reference's
    perplexity 40 and 300 iterations)."""

    def __init__(self, config: EvalConfig, tsne: Optional[TSNE] = None, seed: int = 531, lib_path=None):
        self.config, self.corpus = config, config.corpus
        self.tsne_mode_list, self.tsne_pseudo_speaker_list = config.tsne_mode_list, config.tsne_pseudo_speaker_list
        self.tsne_plot_color_list, self.tsne_legend_list = config.tsne_plot_color_list, config.tsne_legend_list
        if not self.tsne_mode_list or len(self.tsne_legend_list) != len(self.tsne_mode_list):
            raise ValueError("VisualizeDvector: EvalConfig needs tsne_mode_list and a tsne_legend_list of the same length")
        self.n_speaker, self.n_sample, self.seed = config.n_speaker, config.n_sample, seed
        self._tsne = tsne or TSNE(n_components=2, perplexity=40, n_iter=300, lib_path=lib_path)
        with open(os.path.join(config.data_dir_dict["recon"], "test_SQids.json")) as f:
            self.sq_list = json.load(f)
        self.speaker_id_map, self.inv_speaker_id_map = self.get_speaker_id_map()
        self.tsne_speaker_list = [self.speaker_id_map[i] for i in self.tsne_pseudo_speaker_list]

    get_speaker_id_map = WavsToDvector.get_speaker_id_map

    def load_dvector(self):
        self.dvector_list_dict = {mode: np.load(self.config.path("npy", f"{mode}_dvector.npy"), allow_pickle=True) for mode in self.tsne_mode_list}

    def tsne(self):
        cat = np.concatenate([self.dvector_list_dict[mode] for mode in self.tsne_mode_list], axis=0)
        transformed = self._tsne.fit_transform(cat)
        self.trans_dvector_list_dict_all, pointer = {}, 0
        for mode in self.tsne_mode_list:
            n_vector = self.dvector_list_dict[mode].shape[0]
            self.trans_dvector_list_dict_all[mode] = transformed[pointer:pointer + n_vector, :]
            pointer += n_vector

    def get_speaker_dvectors(self):
        self.trans_dvector_list_dict = {
            mode: np.concatenate([self.trans_dvector_list_dict_all[mode][spk * self.n_sample:(spk + 1) * self.n_sample, :] for spk in self.tsne_pseudo_speaker_list], axis=0)
            for mode in self.tsne_mode_list}

    def get_speaker_id_list_dict(self):
        ids = np.array([f"{speaker_id}" for speaker_id in self.tsne_speaker_list for _ in range(self.n_sample)])
        self.speaker_id_list_dict = {mode: ids.copy() for mode in self.tsne_mode_list}

    def scatter_table(self, rng: Optional[np.random.RandomState] = None) -> Dict[str, np.ndarray]:
        """visualize.py:99-138: the `data` dict of the scatter plot.  The three columns are shuffled jointly (`rng`: default
        RandomState(seed), the reference's np.random.seed(seed)) through the reference's string array, and points outside
        x in (-12, 12), y > -12 are masked out."""
        rng = rng or np.random.RandomState(self.seed)
        transformed = np.concatenate([self.trans_dvector_list_dict[mode] for mode in self.tsne_mode_list], axis=0)
        cat_id_list = np.concatenate([self.speaker_id_list_dict[mode] for mode in self.tsne_mode_list], axis=0)
        mode_list = np.concatenate([np.array([legend] * len(self.tsne_speaker_list) * self.n_sample) for legend in self.tsne_legend_list], axis=0)
        joint_list = np.concatenate((transformed, np.expand_dims(cat_id_list, axis=1), np.expand_dims(mode_list, axis=1)), axis=1)
        rng.shuffle(joint_list)
        transformed = joint_list[:, :2].astype(float)
        cat_id_list, mode_list = joint_list[:, 2], joint_list[:, 3]
        mask = np.logical_and.reduce([transformed[:, 0] < 12, transformed[:, 0] > -12, transformed[:, 1] > -12])
        return {"dim-1": transformed[mask, 0], "dim-2": transformed[mask, 1], "Speaker": cat_id_list[mask], "Approach": mode_list[mask]}

    def save_table(self, path: str, rng: Optional[np.random.RandomState] = None) -> Dict[str, np.ndarray]:
        import csv
        data = self.scatter_table(rng)
        with open(path, "w", newline="", encoding="utf8") as f:
            w = csv.writer(f)
            w.writerow(list(data))
            w.writerows(zip(*(data[k].tolist() for k in data)))
        return data


# ---- mel-cepstral distortion along a DTW path (csrc/dtw.h; this project's own step: the reference scores the voice only) ------------------
class MelCepstralDistortion:
    """Does a synthesis say what its recording says?  Mel-cepstral distortion along a dynamic-time-warping path, with log-F0 error and
    voiced/unvoiced disagreement on the same path, on an `mtts_dtw` handle (include/mtts.h states the definition; parity with SPTK /
    WORLD mel-cepstra is unpinned).  Mels are natural-log mels as `TacotronSTFT` produces them, one (T, n_mel) array per utterance.
    max_frames bounds either side of a pair, max_cells the sum of Ta x Tb of one chunk of a call (the direction map, one byte per
    cell, is the only device buffer of that size; longer calls are cut into chunks, with the same results bit for bit)."""

    COLUMNS = ("D", "L", "MCD", "n_voiced_both", "cents_rmse", "n_vuv_mismatch")

    def __init__(self, n_mel: int = 80, n_coef: int = 13, max_frames: int = 2048, max_cells: int = 1 << 28, lib_path=None, *, max_pairs: int = 4096,
                 device: int = 0):
        from . import _lib
        self.n_mel, self.n_coef, self.max_frames, self.max_cells, self.max_pairs = int(n_mel), int(n_coef), int(max_frames), int(max_cells), int(max_pairs)
        self.lib = _lib.load(lib_path)
        self.h = None
        h = C.c_void_p()
        if self.lib.mtts_dtw_create(self.n_mel, self.n_coef, self.max_frames, self.max_cells, self.max_pairs, device, C.byref(h)) != 0:
            raise MttsError(self.lib.mtts_dtw_last_error(None).decode())
        self.h = h
        self.basis = self.dct_basis()
        self._check(self.lib.mtts_dtw_load_basis(self.h, _ptr(self.basis)))

    def _check(self, rc):
        if rc < 0:
            raise MttsError(self.lib.mtts_dtw_last_error(self.h).decode())
        return rc

    def close(self):
        if getattr(self, "h", None):
            self.lib.mtts_dtw_destroy(self.h)
        self.h = None

    __del__ = close

    def dct_basis(self) -> np.ndarray:
        """Rows 1 .. n_coef of the orthonormal DCT-II over n_mel points (scipy.fft.dct(type=2, norm="ortho") without c0): float64 [n_coef][n_mel]."""
        N = self.n_mel
        # B[k-1][n] = sqrt(2 / N) cos(pi (2 n + 1) k / (2 N)); the angle as an integer count q of pi / (2 N), folded into the first octant
        q = np.outer(np.arange(1, self.n_coef + 1), 2 * np.arange(N) + 1) % (4 * N)
        q = np.where(q > 2 * N, 4 * N - q, q)
        sign = np.where(q > N, -1.0, 1.0)
        q = np.where(q > N, 2 * N - q, q)
        val = np.where(2 * q > N, np.sin(np.pi * (N - q) / (2.0 * N)), np.cos(np.pi * q / (2.0 * N)))
        return np.ascontiguousarray(np.sqrt(2.0 / N) * sign * val)

    def _pack(self, mels, what):
        ms = [np.ascontiguousarray(np.asarray(m, np.float32)) for m in mels]
        for u, m in enumerate(ms):
            if m.ndim != 2 or m.shape[1] != self.n_mel:
                raise ValueError(f"{what}[{u}] has shape {m.shape}, expected (T, {self.n_mel})")
        if not ms:
            raise MttsError("no utterances")
        return np.asarray([len(m) for m in ms], np.int32), np.ascontiguousarray(np.concatenate(ms, axis=0))

    def cepstra(self, mels) -> List[np.ndarray]:
        """[(T_u, n_mel) log-mel] -> [(T_u, n_coef) float64], one device call."""
        T, packed = self._pack(mels, "mels")
        out = np.empty((int(T.sum()), self.n_coef), np.float64)
        self._check(self.lib.mtts_dtw_cepstra(self.h, len(T), _ptr(T), _ptr(packed), _ptr(out)))
        return np.split(out, np.cumsum(T)[:-1])

    def mcd_batch(self, mels_a, mels_b, f0_a=None, f0_b=None, return_paths: bool = False):
        """Pair p aligns mels_a[p] with mels_b[p] -> float64 [n_pairs][6]: D, L, MCD [dB], n_voiced_both, cents RMSE, n_vuv_mismatch (see
        `COLUMNS`; the last three NaN without F0, the RMSE NaN when no step has both frames voiced).  f0_a / f0_b: per utterance a
        float64 track with one value per mel frame, 0 = unvoiced (`PitchExtractor.f0_batch`); both or neither.  return_paths: also
        the list of (L_p, 2) int32 paths, (0, 0) first."""
        if len(mels_a) != len(mels_b):
            raise ValueError(f"mcd_batch: {len(mels_a)} mels_a but {len(mels_b)} mels_b")
        Ta, pa = self._pack(mels_a, "mels_a")
        Tb, pb = self._pack(mels_b, "mels_b")
        f0 = [None, None, None, None]
        for side, tracks in enumerate((f0_a, f0_b)):
            if tracks is not None:
                if len(tracks) != len(Ta):
                    raise ValueError(f"mcd_batch: {len(tracks)} F0 tracks for {len(Ta)} pairs")
                ts = [np.ascontiguousarray(np.asarray(t, np.float64).reshape(-1)) for t in tracks]
                f0[2 * side] = np.asarray([len(t) for t in ts], np.int32)
                f0[2 * side + 1] = np.ascontiguousarray(np.concatenate(ts))
        out = np.empty((len(Ta), 6), np.float64)
        L = np.empty(len(Ta), np.int32)
        cap = Ta.astype(np.int64) + Tb - 1
        path = np.empty((int(cap.sum()), 2), np.int32) if return_paths else None
        self._check(self.lib.mtts_dtw_mcd_batch(self.h, len(Ta), _ptr(Ta), _ptr(pa), _ptr(Tb), _ptr(pb), *[None if v is None else _ptr(v) for v in f0], _ptr(out), _ptr(L),
                                                None if path is None else _ptr(path)))
        if not return_paths:
            return out
        starts = np.concatenate([[0], np.cumsum(cap)[:-1]])
        return out, [path[s:s + n].copy() for s, n in zip(starts, L)]


class ObjectiveEvaluation:
    """MCD / F0 figures of a test run's result tree, next to the speaker-similarity classes above and over the same files: for every
    mode and step of `config.mode_step_list` each synthesised wav against its real wav, and each recon wav (the vocoder on the
    ground-truth mel) against its real wav as the floor the vocoder sets.  `mcd`: a `MelCepstralDistortion`; `stft`: the `TacotronSTFT`
    whose log-mels are compared (its handle's batched front-end computes them); `pitch`: a `PitchExtractor` at the same sampling rate
    and hop, or None for MCD only; `wav_loader(path) -> float32 waveform at the STFT's sampling rate` (default:
    `preprocessor.read_wav`, refusing another rate).

    An evaluation set is thousands of utterances, more than one call of the front-end holds (csrc/melfront.h refuses about a million
    frames, and its spectrum workspace is 4 KB per frame), so the work is cut twice, with the same tables bit for bit whatever the cut:
    a mode is scored `pairs_per_call` pairs at a time (only that many synthesised mels are alive at once), and the files of such a block
    go to the front-end in calls of at most `frames_per_call` mel frames (default 65 536: a 270 MB spectrum at filter length 1 024)
    and `MAX_UTTS_PER_CALL` utterances; an utterance longer than the budget goes alone.  Only the features of the REAL files are kept
    (every mode and step is scored against them); a table row is one test file, in `mode_filelist` order."""

    MAX_UTTS_PER_CALL = 4096

    def __init__(self, config: EvalConfig, mcd: MelCepstralDistortion, stft, pitch=None, wav_loader: Optional[Callable[[str], np.ndarray]] = None, *,
                 frames_per_call: int = 1 << 16, pairs_per_call: int = 512):
        self.config, self.mcd, self.stft, self.pitch = config, mcd, stft, pitch
        if mcd.n_mel != stft.n_mel_channels:
            raise ValueError(f"ObjectiveEvaluation: the MCD handle takes {mcd.n_mel} mel channels, the STFT produces {stft.n_mel_channels}")
        if pitch is not None and (pitch.hop_length != stft.hop_length or pitch.sampling_rate != stft.sampling_rate):
            raise ValueError("ObjectiveEvaluation: the pitch extractor's sampling rate and hop length must be the STFT's (one F0 value per mel frame)")
        self.frames_per_call, self.pairs_per_call = int(frames_per_call), int(pairs_per_call)
        if self.frames_per_call < 1 or self.frames_per_call * int(stft.hop_length) >= 1 << 31 or self.frames_per_call > (1 << 30) // (int(stft.filter_length) + 2):
            raise ValueError(f"ObjectiveEvaluation: frames_per_call = {frames_per_call} outside what one front-end call holds at hop {stft.hop_length}, filter length {stft.filter_length}")
        if self.pairs_per_call < 1:
            raise ValueError(f"ObjectiveEvaluation: pairs_per_call = {pairs_per_call} must be at least 1")
        self.n_speaker, self.n_sample, self.mode_step_list, self.data_dir_dict = config.n_speaker, config.n_sample, config.mode_step_list, config.data_dir_dict
        self.wav_loader = wav_loader or self._read_wav
        with open(os.path.join(self.data_dir_dict["recon"], "test_SQids.json")) as f:
            self.sq_list = json.load(f)
        self.speaker_id_map, self.inv_speaker_id_map = self.get_speaker_id_map()
        self.real_filelist = self.get_real_filelist()
        self.mcd_dict: Dict[str, np.ndarray] = {}
        self._real_features = {}      # real file -> (mel, f0): the only features kept
        self.front_end_calls = 0      # mtts_stft_mel_batch calls so far

    get_speaker_id_map = WavsToDvector.get_speaker_id_map
    get_real_filelist = WavsToDvector.get_real_filelist
    _find = WavsToDvector._find

    def _read_wav(self, path: str) -> np.ndarray:
        from .preprocessor import read_wav
        wav, rate = read_wav(path)
        if int(rate) != int(self.stft.sampling_rate):
            raise MttsError(f"{path}: sampling rate {rate}, the STFT takes {self.stft.sampling_rate} Hz (pass a wav_loader that resamples)")
        return wav

    def _modes(self):
        return ["recon"] + [f"{m}_step{s}" for m, steps in self.mode_step_list for s in steps]

    def _front_end(self, wavs):
        """One front-end call (and one F0 call) for waveforms the caller has kept within the budget -> ([mel], [f0] or [None])."""
        n = np.asarray([len(w) for w in wavs], np.int32)
        T = n.astype(np.int64) // self.stft.hop_length + 1
        mel, energy = np.empty((int(T.sum()), self.stft.n_mel_channels), np.float32), np.empty(int(T.sum()), np.float32)
        packed = np.ascontiguousarray(np.concatenate(wavs))
        self.stft._check(self.stft.lib.mtts_stft_mel_batch(self.stft.h, len(wavs), _ptr(n), None, _ptr(packed), _ptr(mel), _ptr(energy)))
        self.front_end_calls += 1
        mels = [m.copy() for m in np.split(mel, np.cumsum(T)[:-1])]      # (copies: a kept mel must not pin its whole call's buffer)
        return mels, (self.pitch.f0_batch(wavs)[0] if self.pitch is not None else [None] * len(wavs))

    def features(self, paths: Sequence[str]):
        """([log-mel (T_u, n_mel) float32], [f0 (T_u,) float64] or None) of the files, in order.  The files are read and sent to the
        front-end in calls of at most `frames_per_call` frames and `MAX_UTTS_PER_CALL` utterances; an utterance's rows are the same
        bits whatever else shares its call.  Nothing is kept."""
        mels, f0s, wavs, frames = [], [], [], 0

        def flush():
            if wavs:
                m, f = self._front_end(wavs)
                mels.extend(m)
                f0s.extend(f)
                wavs.clear()

        for p in paths:
            w = np.ascontiguousarray(np.asarray(self.wav_loader(p), np.float32).reshape(-1))
            T = len(w) // self.stft.hop_length + 1
            if wavs and (frames + T > self.frames_per_call or len(wavs) >= self.MAX_UTTS_PER_CALL):
                flush()
                frames = 0
            wavs.append(w)
            frames += T
        flush()
        return mels, (f0s if self.pitch is not None else None)

    def real_features(self, paths: Sequence[str]):
        """`features` of real files, each computed once and kept: every mode and step is scored against the same recordings."""
        todo = [p for p in dict.fromkeys(paths) if p not in self._real_features]
        if todo:
            mels, f0s = self.features(todo)
            for k, p in enumerate(todo):
                self._real_features[p] = (mels[k], None if f0s is None else f0s[k])
        got = [self._real_features[p] for p in paths]
        return [m for m, _ in got], ([f for _, f in got] if self.pitch is not None else None)

    def mode_filelist(self, mode: str):
        """(test files of the mode, the real file each is scored against): one per test sample in data_id order, five in the 1-shot
        layout test_###_0 .. 4.  A test sample without its directory or its wav is an error, as in `get_syn_dvector_list`: a table has
        a row for every file of every sample, so that the rows of all modes line up."""
        if mode == "recon":
            root, suffix = _testing_dir(self.data_dir_dict["recon"]), "recon.wav"
        else:
            name, step = mode.rsplit("_step", 1)
            root, suffix = _testing_dir(self.data_dir_dict[name]), f"FTstep_{step}.synth.wav"
        test, real = [], []
        for data_id in range(self.n_speaker * self.n_sample):
            d = os.path.join(root, f"test_{data_id:03d}")
            if os.path.exists(d):
                dirs = [d]
            elif mode != "recon" and os.path.exists(d + "_0"):
                dirs = [f"{d}_{i}" for i in range(5)]
            else:
                raise MttsError(f"ObjectiveEvaluation: mode {mode}: test sample {data_id} has no directory {d}")
            for wav_dir in dirs:
                p = self._find(wav_dir, suffix) if os.path.exists(wav_dir) else None
                if p is None:
                    raise MttsError(f"ObjectiveEvaluation: mode {mode}: test sample {data_id} has no *{suffix} in {wav_dir}")
                test.append(p)
                real.append(self.real_filelist[data_id])
        return test, real

    def compute_mcd(self, mode: str) -> np.ndarray:
        test, real = self.mode_filelist(mode)
        rows = []
        for lo in range(0, len(test), self.pairs_per_call):
            mels_t, f0_t = self.features(test[lo:lo + self.pairs_per_call])
            mels_r, f0_r = self.real_features(real[lo:lo + self.pairs_per_call])
            rows.append(self.mcd.mcd_batch(mels_t, mels_r, f0_t, f0_r))
        return np.concatenate(rows, axis=0)

    def get_mcd(self):
        """One [n][6] table per mode (`MelCepstralDistortion.COLUMNS`), saved as npy/<corpus>/<mode>_mcd.npy; an existing file is loaded instead."""
        for mode in self._modes():
            path = self.config.path("npy", f"{mode}_mcd.npy")
            if os.path.exists(path):
                self.mcd_dict[mode] = np.load(path)
            else:
                self.mcd_dict[mode] = self.compute_mcd(mode)
                np.save(path, self.mcd_dict[mode])
        return self.mcd_dict

    @staticmethod
    def summarize(table: np.ndarray):
        """(mean MCD [dB], mean cents RMSE over the pairs that have one, V/UV disagreement in % of all path steps); NaN without F0."""
        t = np.asarray(table, np.float64)
        rmse = t[:, 4][np.isfinite(t[:, 4])]
        with_f0 = np.isfinite(t[:, 5]).all() and len(t) > 0
        return float(t[:, 2].mean()), (float(rmse.mean()) if len(rmse) else float("nan")), (float(100.0 * t[:, 5].sum() / t[:, 1].sum()) if with_f0 else float("nan"))

    def save_mcd(self, output_path: str = "mcd.txt"):
        """npy/<corpus>/mcd_dict.npy and the text summary txt/<corpus>/<output_path>, next to eer.txt."""
        np.save(self.config.path("npy", "mcd_dict.npy"), self.mcd_dict, allow_pickle=True)
        with open(self.config.path("txt", output_path), "w+") as f:
            for mode, table in self.mcd_dict.items():
                m, c, v = self.summarize(table)
                f.write(mode + ":\n")
                f.write(f"MCD:{m:.4f}\tF0_RMSE_cents:{c:.2f}\tVUV_percent:{v:.2f}\n")

    def load_mcd(self):
        self.mcd_dict = np.load(self.config.path("npy", "mcd_dict.npy"), allow_pickle=True)[()]
        return self.mcd_dict


def _student_t_ppf(p: float, df: float) -> float:
    """The p-quantile of Student's t with df degrees of freedom, for where scipy is not importable: bisection on the distribution
    function, itself the regularised incomplete beta function I_x(df / 2, 1 / 2) by Lentz's continued fraction."""
    def betainc(a, b, x):
        if x <= 0.0 or x >= 1.0:
            return 0.0 if x <= 0.0 else 1.0
        if x > (a + 1.0) / (a + b + 2.0):
            return 1.0 - betainc(b, a, 1.0 - x)
        front = math.exp(math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b) + a * math.log(x) + b * math.log1p(-x)) / a
        tiny, f, c, d = 1e-300, 1.0, 1.0, 0.0
        for i in range(400):
            m = i // 2
            num = 1.0 if i == 0 else (m * (b - m) * x / ((a + 2 * m - 1) * (a + 2 * m)) if i % 2 == 0 else -(a + m) * (a + b + m) * x / ((a + 2 * m) * (a + 2 * m + 1)))
            d = 1.0 + num * d
            d = 1.0 / (d if abs(d) > tiny else tiny)
            c = 1.0 + num / (c if abs(c) > tiny else tiny)
            f *= c * d
            if abs(1.0 - c * d) < 1e-15:
                break
        return front * (f - 1.0)

    def cdf(t):
        tail = 0.5 * betainc(0.5 * df, 0.5, df / (df + t * t))
        return 1.0 - tail if t > 0 else tail

    if not 0.0 < p < 1.0 or df <= 0:
        return float("nan")
    lo, hi = -1.0, 1.0
    while cdf(lo) > p:
        lo *= 2.0
    while cdf(hi) < p:
        hi *= 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if cdf(mid) < p else (lo, mid)
    return 0.5 * (lo + hi)


class NeuralMOS:
    """compute_mos.py's `NeuralMOS` for MOSNet: the naturalness score of every wav of a test run's result tree, over the file lists of the
    reference (:65-96) — `real`, `recon`, and `<mode>_step<k>` for every mode of `config.mode_step_list` except scratch_encoder / encoder /
    dvec — found through the helpers the other evaluation classes use.  `mosnet`: a `meta_tts_amd.mosnet.MOSNet`; `wav_loader(path) ->
    (float32 waveform, sampling rate)` (default `preprocessor.read_wav`): a file is read at its own rate and resampled to 16 kHz on the
    device in front of the STFT, where the reference's `librosa.load(sr=16000)` resamples on the host.  A test sample without its
    directory or wav is refused (the reference asserts one candidate), not skipped: every table has a row per test sample.  `compute_mbnet`
    (its model code is not in the reference tree) and the plots are not built."""

    SKIPPED_MODES = ("scratch_encoder", "encoder", "dvec")   # compute_mos.py:78

    def __init__(self, config: EvalConfig, mosnet, wav_loader: Optional[Callable[[str], tuple]] = None, *, frames_per_call: Optional[int] = None):
        self.config, self.mosnet, self.frames_per_call = config, mosnet, frames_per_call
        self.corpus, self.data_dir_dict = config.corpus, config.data_dir_dict
        self.n_sample, self.n_speaker, self.mode_step_list = config.n_sample, config.n_speaker, config.mode_step_list
        self.wav_loader = wav_loader or self._read_wav
        with open(os.path.join(self.data_dir_dict["recon"], "test_SQids.json")) as f:
            self.sq_list = json.load(f)
        self.speaker_id_map, self.inv_speaker_id_map = self.get_speaker_id_map()
        self.file_list = self.setup_filelist()

    get_speaker_id_map = WavsToDvector.get_speaker_id_map
    get_real_filelist = WavsToDvector.get_real_filelist
    _find = WavsToDvector._find

    @staticmethod
    def _read_wav(path: str):
        from .preprocessor import read_wav
        return read_wav(path)

    def _test_files(self, mode: str, data_dir: str, suffix: str):
        root, out = _testing_dir(data_dir), []
        for data_id in range(self.n_speaker * self.n_sample):
            d = os.path.join(root, f"test_{data_id:03d}")
            if not os.path.isdir(d):
                raise MttsError(f"NeuralMOS: mode {mode}: test sample {data_id} has no directory {d}")
            p = self._find(d, suffix)
            if p is None:
                raise MttsError(f"NeuralMOS: mode {mode}: test sample {data_id} has no *{suffix} in {d}")
            out.append(p)
        return out

    def setup_filelist(self):
        file_list = {"real": self.get_real_filelist()}
        for p in file_list["real"]:
            if not os.path.exists(p):
                raise MttsError(f"NeuralMOS: real wav {p} does not exist")
        file_list["recon"] = self._test_files("recon", self.data_dir_dict["recon"], ".recon.wav")
        for mode, steps in self.mode_step_list:
            if mode in self.SKIPPED_MODES:
                continue
            for step in steps:
                file_list[f"{mode}_step{step}"] = self._test_files(f"{mode}_step{step}", self.data_dir_dict[mode], f"FTstep_{step}.synth.wav")
        return file_list

    def score_files(self, paths: Sequence[str]) -> np.ndarray:
        """MOSNet scores of the files, in order: read, grouped by sampling rate, one `score_wavs` per rate."""
        wavs, groups = [], {}
        for i, p in enumerate(paths):
            wav, rate = self.wav_loader(p)
            wavs.append(np.asarray(wav, np.float32).reshape(-1))
            groups.setdefault(int(rate), []).append(i)
        out = np.empty(len(wavs), np.float32)
        for rate, idx in sorted(groups.items()):
            out[idx] = self.mosnet.score_wavs([wavs[i] for i in idx], source_rate=rate, frames_per_call=self.frames_per_call)[0]
        return out

    def compute_mosnet(self):
        """csv/<corpus>/mosnet_<mode>.csv per mode (`test_id, mos` and one `test_XXX, score` row per test sample); a mode whose csv
        exists is skipped, as in the reference.  Returns {mode: scores} of the modes computed now."""
        done = {}
        for mode, files in self.file_list.items():
            path = self.config.path("csv", f"mosnet_{mode}.csv")
            if os.path.exists(path):
                continue
            for _id, filepath in enumerate(files):      # compute_mos.py:132-134
                basename, realbase = os.path.basename(filepath).split(".")[0], os.path.basename(self.file_list["real"][_id]).split(".")[0]
                if basename != realbase:
                    raise MttsError(f"NeuralMOS: mode {mode}: test sample {_id} is {basename}, the real file is {realbase}")
            scores = self.score_files(files)
            with open(path, "w") as f:
                f.write("test_id, mos\n")
                for _id, score in enumerate(scores):
                    f.write(f"test_{_id:03}, {float(score)}\n")
            done[mode] = scores
        return done

    @staticmethod
    def get_mean_confidence_interval(data, confidence: float = 0.95):
        """compute_mos.py:175-180: (mean, half width of the Student-t interval), scipy.stats.sem's ddof = 1."""
        a = 1.0 * np.array(data)
        n = len(a)
        m, se = np.mean(a), (np.std(a, ddof=1) / np.sqrt(n) if n > 1 else float("nan"))
        try:
            from scipy import stats
            q = stats.t.ppf((1 + confidence) / 2.0, n - 1)
        except ImportError:
            q = _student_t_ppf((1 + confidence) / 2.0, n - 1)
        return m, se * q

    def add_up(self, net: str = "mosnet"):
        """txt/<corpus>/<net>.txt: one `mode, mean, ci` line per mode, from the csv files."""
        rows = []
        with open(self.config.path("txt", f"{net}.txt"), "w") as fo:
            for mode in self.file_list:
                with open(self.config.path("csv", f"{net}_{mode}.csv")) as f:
                    scores = [float(line.strip().split(",")[1].strip()) for line in f.readlines()[1:]]
                mean, ci = self.get_mean_confidence_interval(scores)
                fo.write(f"{mode}, {mean}, {ci}\n")
                rows.append((mode, mean, ci))
        return rows
