"""Forced alignment on libmtts.so (csrc/align.h through include/mtts.h: mtts_align_*): phoneme durations from features and phone sequences,
so that a corpus without third-party TextGrids — a new speaker's few-shot recordings — gets past `Preprocessor.build_from_path`.

What this is: the classical flat-start monophone aligner, the first pass of every HMM forced aligner.  One diagonal Gaussian per phone
class over natural-log mel frames, Baum-Welch re-estimation in closed form (`fit`), Viterbi to durations (`align`).  No network, no
optimiser; the objective rises monotonically by construction.  What it is not: parity with MFA, Kaldi and HTK is UNPINNED, and alignment
quality on real speech is not measured.  Grapheme-to-phoneme conversion stays the caller's: every entry here takes phone sequences.

`write_textgrid` writes the durations in Praat's long TextGrid format so that `preprocessor.read_textgrid` + `Preprocessor.get_alignment`
give them back exactly; `align_corpus` does that for every wav of a preprocessing config's subsets, after which the unchanged
`build_from_path` runs on them."""
from __future__ import annotations

import ctypes as C
import os
from typing import Callable, List, Optional, Sequence

import numpy as np

from .engine import MttsError


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class MonophoneAligner:
    """phone_set: the phone classes (a sequence of names; class id = position).  optional: the phones whose states may be skipped (a
    silence between words); two of them next to each other in a sequence are refused.  max_frames / max_states bound one utterance,
    max_cells the sum of frames x states of one chunk of a call (the alpha / gamma workspace, float64 per cell), max_utts its utterances;
    longer calls are cut into chunks with the same results bit for bit."""

    def __init__(self, phone_set: Sequence[str], n_feat: int = 80, optional: Sequence[str] = ("sp",), *, max_frames: int = 4096, max_states: int = 1024,
                 max_cells: int = 1 << 25, max_utts: int = 1024, var_floor: float = 0.01, min_occ: float = 1e-3, lib_path=None, device: int = 0):
        from . import _lib
        self.phone_set = [str(p) for p in phone_set]
        if len(set(self.phone_set)) != len(self.phone_set):
            raise ValueError("phone_set holds a phone twice")
        self.optional = tuple(str(p) for p in optional)
        self.index = {p: i for i, p in enumerate(self.phone_set)}
        self.n_feat, self.n_classes = int(n_feat), len(self.phone_set)
        self.limits = dict(max_frames=int(max_frames), max_states=int(max_states), max_cells=int(max_cells), max_utts=int(max_utts))
        self.var_floor, self.min_occ = float(var_floor), float(min_occ)
        self.lib = _lib.load(lib_path)
        self.h = None
        h = C.c_void_p()
        if self.lib.mtts_align_create(self.n_feat, self.n_classes, int(max_frames), int(max_states), int(max_cells), int(max_utts), device, C.byref(h)) != 0:
            raise MttsError(self.lib.mtts_align_last_error(None).decode())
        self.h = h
        self._check(self.lib.mtts_align_set_floor(self.h, self.var_floor, self.min_occ))

    def _check(self, rc):
        if rc < 0:
            raise MttsError(self.lib.mtts_align_last_error(self.h).decode())
        return rc

    def close(self):
        if getattr(self, "h", None):
            self.lib.mtts_align_destroy(self.h)
        self.h = None

    __del__ = close

    # ---- packing ----------------------------------------------------------------------------------------------------------------------
    def _features(self, features):
        xs = [np.ascontiguousarray(np.asarray(x, np.float32)) for x in features]
        if not xs:
            raise MttsError("no utterances")
        for u, x in enumerate(xs):
            if x.ndim != 2 or x.shape[1] != self.n_feat:
                raise ValueError(f"features[{u}] has shape {x.shape}, expected (T, {self.n_feat})")
        return xs

    def _states(self, phone_seqs):
        cls, opt = [], []
        for u, seq in enumerate(phone_seqs):
            for p in seq:
                if p not in self.index:
                    raise ValueError(f"phone_seqs[{u}]: {p!r} is not in the phone set")
            cls.append(np.asarray([self.index[p] for p in seq], np.int32))
            opt.append(np.asarray([p in self.optional for p in seq], np.uint8))
        return cls, opt

    def _batch(self, xs, cls, opt):
        return (len(xs), np.asarray([len(x) for x in xs], np.int32), np.asarray([len(c) for c in cls], np.int32), np.ascontiguousarray(np.concatenate(cls)),
                np.ascontiguousarray(np.concatenate(opt)), np.ascontiguousarray(np.concatenate(xs, axis=0)))

    def _args(self, features, phone_seqs):
        xs = self._features(features)
        if len(phone_seqs) != len(xs):
            raise ValueError(f"{len(xs)} feature arrays but {len(phone_seqs)} phone sequences")
        cls, opt = self._states(phone_seqs)
        return xs, cls, opt

    # ---- model ------------------------------------------------------------------------------------------------------------------------
    def flat_start(self, features):
        """Every class = the mean and variance of all frames of `features` (one call; float64, two passes)."""
        xs = self._features(features)
        T = np.asarray([len(x) for x in xs], np.int32)
        self._check(self.lib.mtts_align_flat_start(self.h, len(xs), _ptr(T), _ptr(np.ascontiguousarray(np.concatenate(xs, axis=0)))))

    def get_model(self):
        """-> (mean [V][F], var [V][F], global_var [F]) float64."""
        mean, var, g = np.empty((self.n_classes, self.n_feat)), np.empty((self.n_classes, self.n_feat)), np.empty(self.n_feat)
        self._check(self.lib.mtts_align_get_model(self.h, _ptr(mean), _ptr(var), _ptr(g)))
        return mean, var, g

    def set_model(self, mean, var, global_var):
        mean, var, g = (np.ascontiguousarray(np.asarray(a, np.float64)) for a in (mean, var, global_var))
        if mean.shape != (self.n_classes, self.n_feat) or var.shape != mean.shape or g.shape != (self.n_feat,):
            raise ValueError(f"set_model: shapes {mean.shape}, {var.shape}, {g.shape}; expected ({self.n_classes}, {self.n_feat}) twice and ({self.n_feat},)")
        self._check(self.lib.mtts_align_set_model(self.h, _ptr(mean), _ptr(var), _ptr(g)))

    def state_dict(self) -> dict:
        mean, var, g = self.get_model()
        return {"phone_set": list(self.phone_set), "optional": list(self.optional), "n_feat": self.n_feat, "mean": mean, "var": var, "global_var": g,
                "var_floor": self.var_floor, "min_occ": self.min_occ}

    def load_state_dict(self, state: dict):
        """The model, the floor and the occupancy threshold of `state_dict()`; a restored aligner continues a fit bit-identically
        (`fit(..., flat_start=False)`)."""
        if list(state["phone_set"]) != self.phone_set or int(state["n_feat"]) != self.n_feat:
            raise ValueError("load_state_dict: the state was made with another phone set or feature width")
        self.optional = tuple(state["optional"])
        self.var_floor, self.min_occ = float(state["var_floor"]), float(state["min_occ"])
        self._check(self.lib.mtts_align_set_floor(self.h, self.var_floor, self.min_occ))
        self.set_model(state["mean"], state["var"], state["global_var"])

    # ---- EM, posteriors, Viterbi ------------------------------------------------------------------------------------------------------
    def em_iteration(self, features, phone_seqs, batch_utterances: int = 64):
        """One Baum-Welch iteration over the corpus in batches of `batch_utterances` -> (total LL, per-utterance LL float64)."""
        xs, cls, opt = self._args(features, phone_seqs)
        self._check(self.lib.mtts_align_em_begin(self.h))
        lls = np.empty(len(xs), np.float64)
        for k in range(0, len(xs), max(1, int(batch_utterances))):
            sl = slice(k, k + max(1, int(batch_utterances)))
            n, T, S, c, o, x = self._batch(xs[sl], cls[sl], opt[sl])
            ll = np.empty(n, np.float64)
            self._check(self.lib.mtts_align_em_accumulate(self.h, n, _ptr(T), _ptr(S), _ptr(c), _ptr(o), _ptr(x), _ptr(ll)))
            lls[sl] = ll
        total = C.c_double()
        self._check(self.lib.mtts_align_em_finish(self.h, C.byref(total)))
        return float(total.value), lls

    def fit(self, features, phone_seqs, n_iter: int = 8, batch_utterances: int = 64, flat_start: bool = True) -> List[float]:
        """Flat start on all of `features` (unless flat_start=False: continue from the loaded model), then `n_iter` EM iterations.
        Returns each iteration's total log-likelihood (of the model the iteration started from), which never decreases."""
        if flat_start:
            self.flat_start(features)
        return [self.em_iteration(features, phone_seqs, batch_utterances)[0] for _ in range(int(n_iter))]

    def posteriors(self, features, phone_seqs):
        """-> (LL float64 [n], [gamma (T_u, S_u) float64]): the soft alignment of every utterance under the current model."""
        xs, cls, opt = self._args(features, phone_seqs)
        n, T, S, c, o, x = self._batch(xs, cls, opt)
        cells = T.astype(np.int64) * S
        ll, gamma = np.empty(n, np.float64), np.empty(int(cells.sum()), np.float64)
        self._check(self.lib.mtts_align_posteriors(self.h, n, _ptr(T), _ptr(S), _ptr(c), _ptr(o), _ptr(x), _ptr(ll), _ptr(gamma)))
        starts = np.concatenate([[0], np.cumsum(cells)[:-1]])
        return ll, [gamma[a:a + m].reshape(t, s) for a, m, t, s in zip(starts, cells, T, S)]

    def align(self, features, phone_seqs, return_scores: bool = False):
        """-> [durations (S_u,) int32] (frames per phone, 0 for a skipped optional phone, sum = T_u) and, with return_scores, the
        Viterbi paths' log-likelihoods float64 [n]."""
        xs, cls, opt = self._args(features, phone_seqs)
        n, T, S, c, o, x = self._batch(xs, cls, opt)
        dur, score = np.empty(int(S.sum()), np.int32), np.empty(n, np.float64)
        self._check(self.lib.mtts_align_align(self.h, n, _ptr(T), _ptr(S), _ptr(c), _ptr(o), _ptr(x), _ptr(dur), _ptr(score)))
        durs = np.split(dur, np.cumsum(S)[:-1])
        return (durs, score) if return_scores else durs


def write_textgrid(path, phones: Sequence[str], durations: Sequence[int], hop_length: int, sampling_rate: int):
    """A long-format TextGrid with one interval tier `phones`: phone k lasts durations[k] frames of hop_length samples; zero-length
    intervals are left out.  Boundaries are printed as the shortest decimal that reads back as the float64 nearest to frames x
    hop_length / sampling_rate, so that `read_textgrid` + `Preprocessor.get_alignment` (which rounds time x sampling_rate / hop_length)
    give the same frame counts back exactly."""
    if len(phones) != len(durations):
        raise ValueError(f"write_textgrid: {len(phones)} phones but {len(durations)} durations")
    edges = np.concatenate([[0], np.cumsum(np.asarray(durations, np.int64))])
    if (np.diff(edges) < 0).any():
        raise ValueError("write_textgrid: negative duration")
    t = lambda frames: repr(float(int(frames) * int(hop_length) / int(sampling_rate)))   # noqa: E731
    ivs = [(t(edges[k]), t(edges[k + 1]), str(p)) for k, p in enumerate(phones) if edges[k + 1] > edges[k]]
    xmax = t(edges[-1])
    lines = ['File type = "ooTextFile"', 'Object class = "TextGrid"', "", "xmin = 0.0", f"xmax = {xmax}", "tiers? <exists>", "size = 1", "item []:",
             "\titem [1]:", '\t\tclass = "IntervalTier"', '\t\tname = "phones"', "\t\txmin = 0.0", f"\t\txmax = {xmax}", f"\t\tintervals: size = {len(ivs)}"]
    for k, (a, b, p) in enumerate(ivs):
        p = p.replace('"', '""')
        lines += [f"\t\t\tintervals [{k + 1}]:", f"\t\t\t\txmin = {a}", f"\t\t\t\txmax = {b}", f'\t\t\t\ttext = "{p}"']
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")


def align_corpus(preprocessor, phones_fn: Callable[[str, str], Optional[Sequence[str]]], *, aligner: Optional[MonophoneAligner] = None, optional: Sequence[str] = ("sp",),
                 n_iter: int = 8, batch_utterances: int = 32, wav_loader=None, lib_path=None, **aligner_kwargs):
    """Writes `<preprocessed_path>/TextGrid/<speaker>/<basename>.TextGrid` for every wav of the preprocessor's configured subsets, so
    that the unchanged `build_from_path` finds an alignment for each.  phones_fn(speaker, basename) -> the utterance's phone sequence
    (None: leave the utterance out); turning text into phones is the caller's business — no grapheme-to-phoneme step and no lexicon
    here.  Features are the natural-log mels of `preprocessor.mel_batch` (the `MelFront` front-end), `batch_utterances` wavs per call,
    all kept in host memory for the fit.  Without `aligner`, one is made over the sorted phones seen, flat-started and fitted for
    `n_iter` iterations; a given aligner is fitted the same way unless n_iter = 0 (then it only aligns, with the model it holds).
    A wav at another rate than the config's is an error (resample first).  Returns {(speaker, basename): durations}."""
    from .preprocessor import read_wav
    wav_loader = wav_loader or read_wav
    pp = preprocessor
    dsets = [d for ds in (pp.train_set, pp.val_set, pp.test_set) for d in (ds if isinstance(ds, list) else [ds]) if isinstance(d, str)]
    keys, seqs, mels, pending = [], [], [], []

    def flush():
        if pending:
            mels.extend(pp.mel_batch(pending)[0])
            pending.clear()

    for dset in dsets:
        dset_dir = os.path.join(pp.in_dir, dset)
        for speaker in sorted(os.listdir(dset_dir)):
            for wav_name in sorted(os.listdir(os.path.join(dset_dir, speaker))):
                if ".wav" not in wav_name:
                    continue
                basename = wav_name.split(".")[0]
                phones = phones_fn(speaker, basename)
                if phones is None:
                    continue
                wav, sr = wav_loader(os.path.join(dset_dir, speaker, wav_name))
                if int(sr) != int(pp.sampling_rate):
                    raise MttsError(f"{wav_name}: sampling rate {sr} differs from the config's {pp.sampling_rate} (no resampling here)")
                keys.append((speaker, basename))
                seqs.append([str(p) for p in phones])
                pending.append(wav)
                if len(pending) >= batch_utterances:
                    flush()
    flush()
    if not keys:
        return {}
    own = aligner is None
    if own:
        n_mel = int(mels[0].shape[1])
        aligner = MonophoneAligner(sorted({p for s in seqs for p in s}), n_feat=n_mel, optional=optional, lib_path=lib_path,
                                   **{"max_frames": max(len(m) for m in mels), "max_states": max(len(s) for s in seqs), **aligner_kwargs})
    try:
        if n_iter > 0:
            aligner.fit(mels, seqs, n_iter=n_iter, batch_utterances=batch_utterances)
        durs = aligner.align(mels, seqs)
    finally:
        if own:
            aligner.close()
    out = {}
    for (speaker, basename), seq, d in zip(keys, seqs, durs):
        write_textgrid(os.path.join(pp.out_dir, "TextGrid", speaker, f"{basename}.TextGrid"), seq, d, pp.hop_length, pp.sampling_rate)
        out[(speaker, basename)] = d
    return out
