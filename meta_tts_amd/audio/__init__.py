"""Feature front-end and its inverse: waveform -> log-mel spectrogram + energy (mirror of the reference's `audio` package surface that
the preprocessor uses: `Audio.stft.TacotronSTFT`, `Audio.tools.get_mel_from_wav`) and back — `STFT.transform` / `STFT.inverse`,
`audio_processing.griffin_lim`, `tools.inv_mel_spec`, and `griffin.GriffinLim`, a weight-free vocoder for the Saver; `PitchExtractor`
(pitch.py) is the batched device F0 estimator the preprocessor can use in place of pyworld."""
from . import audio_processing, griffin, pitch, stft, tools  # noqa: F401
from .pitch import PitchExtractor  # noqa: F401
