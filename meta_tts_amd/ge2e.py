"""GE2E training of the d-vector speaker encoder on the device (include/mtts.h: mtts_dvector_ge2e_*; kernels: csrc/ge2e.h).

The reference names its from-scratch encoder class `GE2E` (lightning/model/speaker_encoder.py:11-31) and takes resemblyzer's pretrained
weights; the objective that name promises is not in its tree.  What runs here is the softmax variant of the generalized end-to-end loss
(Wan et al. 2018) as include/mtts.h defines it, with the trainer rule stated there (w0 = 10, b0 = -5, the gradients of w and b x 0.01,
joint clip to 3, Adam 1e-4).  Parity with any published GE2E code is UNPINNED; tests/ge2e_oracle.py restates the definition in float64.

A step never leaves the device: the training forward, the loss, its backward into the LSTM sweep, the joint norm and both Adam updates
are enqueued on the encoder's stream; the host waits only for a loss or a similarity matrix it asked for."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np

from .speaker_encoder import DVectorEncoder, tensor_shapes

_WHICH = {"value": 0, "grad": 1, "adam_m": 2, "adam_v": 3}


def batch_eer(sim: np.ndarray, speakers_per_batch: int, utterances_per_speaker: int) -> float:
    """Equal error rate of one batch's similarity matrix [N M][N] with labels k == j, by the routine SpeakerVerification.get_eer uses."""
    from .evaluation import equal_error_rate
    sim = np.asarray(sim, np.float64).reshape(speakers_per_batch * utterances_per_speaker, speakers_per_batch)
    y_true = (np.arange(speakers_per_batch)[None, :] == np.repeat(np.arange(speakers_per_batch), utterances_per_speaker)[:, None]).astype(np.float64)
    return float(equal_error_rate(y_true.flatten(), sim.flatten())[0])


class GE2ETrainer:
    """Owns the loss's two scalars and the optimizer state of `encoder` (a DVectorEncoder whose max_utts and max_partials hold
    speakers_per_batch * utterances_per_speaker); the encoder stays usable for `embed` between steps.  A step does not download the
    weights: it marks the encoder's host copy stale, and `encoder.state_dict()` / `encoder_state_dict()` export them when next asked.
    `step`: the optimizer steps the encoder's Adam state already stands for (0: a fresh encoder).  The trainer sets the handle's
    count to it, so the bias correction, `steps` and `state_dict()["step"]` are one number from the first step on."""

    def __init__(self, encoder: DVectorEncoder, speakers_per_batch: int, utterances_per_speaker: int, lr: float = 1e-4, betas=(0.9, 0.999),
                 eps: float = 1e-8, max_norm: float = 3.0, scalar_grad_scale: float = 0.01, init_w: float = 10.0, init_b: float = -5.0,
                 step: int = 0):
        self.encoder, self.lib = encoder, encoder.lib
        self.N, self.M = int(speakers_per_batch), int(utterances_per_speaker)
        self.lr, self.betas, self.eps, self.max_norm, self.scalar_grad_scale = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(max_norm), float(scalar_grad_scale)
        self.steps = int(step)
        if not encoder.training:
            encoder.enable_training()
        encoder._check(self.lib.mtts_dvector_ge2e_enable(encoder.h, float(init_w), float(init_b)))
        encoder.set_optimizer_step(self.steps)

    # ---- the step --------------------------------------------------------------------------------------------------------------------
    def _shape(self):
        return (self.N * self.M, self.encoder.frames, self.encoder.cfg["n_mels"])

    def forward_backward(self, mels, return_loss: bool = True, return_sim: bool = False):
        """mels: numpy [N M][frames][n_mels], speaker-major.  -> loss (float), the similarity matrix [N M][N], both as a tuple, or None;
        nothing is waited for when neither is asked for."""
        mels = np.ascontiguousarray(np.asarray(mels, np.float32))
        if mels.shape != self._shape():
            raise ValueError(f"mels must be {self._shape()} (speaker-major), got {mels.shape}")
        return self._run(mels.ctypes.data_as(C.c_void_p), 0, return_loss, return_sim, keep=mels)

    def forward_backward_device(self, mels_dev: int, return_loss: bool = True, return_sim: bool = False):
        """The same over a [N M][frames][n_mels] float32 stack already in device memory (its address), read in place."""
        return self._run(C.c_void_p(int(mels_dev)), 1, return_loss, return_sim)

    def _run(self, ptr, on_device, return_loss, return_sim, keep=None):
        loss = np.zeros(1, np.float32) if return_loss else None
        sim = np.empty((self.N * self.M, self.N), np.float32) if return_sim else None
        self._keep = (keep, loss, sim)   # (an enqueued copy reads / writes them)
        self.encoder._check(self.lib.mtts_dvector_ge2e_forward_backward(
            self.encoder.h, ptr, on_device, self.N, self.M, loss.ctypes.data_as(C.c_void_p) if return_loss else None,
            sim.ctypes.data_as(C.c_void_p) if return_sim else None))
        if return_loss and return_sim:
            return float(loss[0]), sim
        return float(loss[0]) if return_loss else sim

    def step(self):
        """Scale the gradients of w and b, clip the joint norm, Adam on the encoder and on (w, b) — on the device."""
        self.encoder._check(self.lib.mtts_dvector_ge2e_step(self.encoder.h, self.lr, self.betas[0], self.betas[1], self.eps, self.max_norm, self.scalar_grad_scale))
        self.steps += 1
        self.encoder.state_stale = True

    def train_step(self, mels, return_eer: bool = False):
        """forward_backward + step -> (loss, eer); eer (of this batch, before the update) is None unless asked for."""
        if return_eer:
            loss, sim = self.forward_backward(mels, True, True)
            eer: Optional[float] = batch_eer(sim, self.N, self.M)
        else:
            loss, eer = self.forward_backward(mels, True, False), None
        self.step()
        return loss, eer

    # ---- the two scalars -------------------------------------------------------------------------------------------------------------
    def scalars(self, which: str = "value") -> np.ndarray:
        """(w, b): "value", "grad", "adam_m" or "adam_v"."""
        out = np.empty(2, np.float32)
        self.encoder._check(self.lib.mtts_dvector_ge2e_get(self.encoder.h, _WHICH[which], out.ctypes.data_as(C.c_void_p)))
        return out

    def set_scalars(self, which: str, wb):
        a = np.ascontiguousarray(np.asarray(wb, np.float32).reshape(2))
        self.encoder._check(self.lib.mtts_dvector_ge2e_set(self.encoder.h, _WHICH[which], a.ctypes.data_as(C.c_void_p)))

    @property
    def similarity_weight(self) -> float:
        return float(self.scalars()[0])

    @property
    def similarity_bias(self) -> float:
        return float(self.scalars()[1])

    # ---- checkpoints -----------------------------------------------------------------------------------------------------------------
    def _names(self):
        return list(tensor_shapes(**self.encoder.cfg))

    def encoder_state_dict(self) -> Dict[str, np.ndarray]:
        """The encoder's tensors under their own names: what DVectorEncoder.load_state_dict, and so SpeakerEmbedder, takes."""
        return self.encoder.state_dict()

    def state_dict(self) -> Dict[str, np.ndarray]:
        sd = self.encoder_state_dict()
        for key, which in (("adam_m.", 2), ("adam_v.", 3)):
            for n in self._names():
                sd[key + n] = self.encoder.export(n, which)
        wb, m, v = self.scalars("value"), self.scalars("adam_m"), self.scalars("adam_v")
        sd["similarity_weight"], sd["similarity_bias"] = wb[0:1].copy(), wb[1:2].copy()
        sd["adam_m.similarity_weight"], sd["adam_m.similarity_bias"] = m[0:1].copy(), m[1:2].copy()
        sd["adam_v.similarity_weight"], sd["adam_v.similarity_bias"] = v[0:1].copy(), v[1:2].copy()
        sd["step"] = np.asarray([self.steps], np.int64)
        return sd

    def load_state_dict(self, sd):
        self.encoder.load_state_dict(sd)
        for key, which in (("adam_m.", 2), ("adam_v.", 3)):
            for n in self._names():
                self.encoder.import_state(n, which, sd[key + n])
        cat = lambda p: np.concatenate([np.asarray(sd[p + "similarity_weight"], np.float32).reshape(1), np.asarray(sd[p + "similarity_bias"], np.float32).reshape(1)])
        self.set_scalars("value", cat(""))
        self.set_scalars("adam_m", cat("adam_m."))
        self.set_scalars("adam_v", cat("adam_v."))
        self.steps = int(np.asarray(sd["step"]).reshape(-1)[0])
        self.encoder.set_optimizer_step(self.steps)


class SpeakerBatchSampler:
    """Host-side batches for GE2ETrainer: per batch N distinct speakers, M distinct utterances of each and a uniform window of `frames`
    frames in each utterance, from one seeded numpy RandomState.  mels_by_speaker: {speaker: [mel [T_i][n_mels], ...]}."""

    def __init__(self, mels_by_speaker: Dict[str, List[np.ndarray]], speakers_per_batch: int, utterances_per_speaker: int, frames: int, seed: int = 0):
        self.N, self.M, self.frames = int(speakers_per_batch), int(utterances_per_speaker), int(frames)
        self.speakers = sorted(mels_by_speaker)
        if len(self.speakers) < self.N:
            raise ValueError(f"the corpus has {len(self.speakers)} speakers, a batch needs {self.N}")
        self.usable = {}
        for s in self.speakers:
            ok = [np.asarray(m, np.float32) for m in mels_by_speaker[s] if np.asarray(m).shape[0] >= self.frames]
            if len(ok) < self.M:
                raise ValueError(f"speaker {s} has {len(ok)} utterances of at least {self.frames} frames, a batch needs {self.M}")
            self.usable[s] = ok
        self.rng = np.random.RandomState(seed)

    def draw(self):
        """-> (mels [N M][frames][n_mels] speaker-major, picks [(speaker, utterance index among the usable ones, first frame)] per row)."""
        picks, rows = [], []
        for s in (self.speakers[k] for k in self.rng.choice(len(self.speakers), self.N, replace=False)):
            for u in self.rng.choice(len(self.usable[s]), self.M, replace=False):
                mel = self.usable[s][int(u)]
                t0 = int(self.rng.randint(0, mel.shape[0] - self.frames + 1))
                picks.append((s, int(u), t0))
                rows.append(mel[t0:t0 + self.frames])
        return np.stack(rows).astype(np.float32), picks

    def __iter__(self):
        while True:
            yield self.draw()[0]


def mels_from_wavs(embedder, wavs: Sequence[np.ndarray]) -> List[np.ndarray]:
    """The 40-channel power-mel frames [(T_u, 40) float32] of 16 kHz waveforms through `embedder`'s packed front-end (a SpeakerEmbedder;
    its wav_to_mel_spectrogram): what SpeakerBatchSampler is fed."""
    return [np.ascontiguousarray(m) for m in embedder.wav_to_mel_spectrogram(list(wavs))]
