"""Griffin-Lim as a vocoder: `GriffinLim(stft).infer(mels, max_wav_value, lengths)` has the duck type of vocoder.MelGAN.infer
(lightning/utils.py:20-30), so `Saver.on_test_batch_end(..., vocoder=GriffinLim(stft))` writes the test-stage wavs without weights.

Utterance b is inv_mel_spec's computation (audio/tools.py:18-37) on its first ceil(lengths[b] / hop) frames — hop * (frames - 2)
samples, cropped to lengths[b] — with its starting phases drawn from numpy's global generator in batch order, so a batched call
equals consecutive single calls.  All utterances go through the same device launches.  The waveform is clipped to [-1, 1] before the
int16 scale (Griffin-Lim, unlike MelGAN's tanh, can overshoot)."""
from __future__ import annotations

import math

import numpy as np

from .audio_processing import random_angles


class GriffinLim:
    def __init__(self, stft, n_iters: int = 60):
        """stft: a meta_tts_amd.audio.stft.TacotronSTFT carrying the mel basis the mels were made with."""
        self.stft, self.n_iters = stft, int(n_iters)
        self.hop = stft.hop_length

    def mel2wav(self, mels, frame_lens=None):
        """(B, n_mel, T) log-mels -> list of float32 waveforms (hop * (frames_b - 2) samples each)."""
        mels = np.asarray(mels, np.float32)
        frames = [mels.shape[2]] * len(mels) if frame_lens is None else [min(int(f), mels.shape[2]) for f in frame_lens]
        sel = [mels[b, :, :frames[b]] for b in range(len(mels))]
        n_bins = self.stft.filter_length // 2 + 1
        angles = [random_angles((1, n_bins, f - 1))[0] for f in frames]
        return self.stft.inv_mel_with_angles(sel, angles, self.n_iters)

    def infer(self, mels, max_wav_value, lengths=None):
        frame_lens = None if lengths is None else [int(math.ceil(l / self.hop)) for l in lengths]
        wavs = self.mel2wav(mels, frame_lens)
        out = [(np.clip(w, -1.0, 1.0) * max_wav_value).astype("int16") for w in wavs]
        if lengths is not None:
            out = [w[: int(l)] for w, l in zip(out, lengths)]
        return out
