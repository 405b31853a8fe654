"""audio/tools.py:8-37."""
import numpy as np

from .audio_processing import random_angles


def get_mel_from_wav(audio, _stft):
    """wav (n_samples,) -> (melspec (n_mel, T) float32, energy (T,) float32); the waveform is clipped to [-1, 1] first."""
    audio = np.clip(np.asarray(audio, np.float32)[None, :], -1, 1)
    melspec, energy = _stft.mel_spectrogram(audio)
    return melspec[0].astype(np.float32), energy[0].astype(np.float32)


def inv_mel_spec(mel, out_filename, _stft, griffin_iters=60):
    """log-mel (n_mel, T) -> float32 wav of hop * (T - 2) samples at `_stft.sampling_rate` written to `out_filename`:
    magnitude = 1000 * exp(mel)^T @ mel_basis without the last frame, then `griffin_iters` Griffin-Lim iterations from phases drawn
    from numpy's global generator (tools.py:18-37, audio_processing.py:66-80), all on the device."""
    from scipy.io.wavfile import write
    mel = np.asarray(mel.detach().cpu().numpy() if hasattr(mel, "detach") else mel, np.float32)
    angles = random_angles((1, _stft.filter_length // 2 + 1, mel.shape[1] - 1))[0]
    audio = _stft.inv_mel_with_angles([mel], [angles], griffin_iters)[0]
    write(out_filename, _stft.sampling_rate, audio)
