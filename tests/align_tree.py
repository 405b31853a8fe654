"""A tiny synthetic RAW corpus for tests/test_align.py: `<raw>/train/<speaker>/<basename>.wav` + `.lab`, no TextGrids.  Every phone is a
tone of its own frequency on known durations (in frames of one hop), so a phone sequence is recoverable from the mel frames; `sp` is a
near-silent optional phone.  Also the preprocessing config the tree is read with."""
import os

import numpy as np

SAMPLING_RATE, HOP, FILTER = 22050, 256, 1024
TONES = {"AA": 330.0, "IY": 880.0, "S": 2400.0, "M": 1500.0, "sp": 0.0}
# speaker / basename -> [(phone, frames)]
UTTERANCES = {
    ("spkA", "spkA_u0"): [("AA", 6), ("S", 5), ("IY", 7), ("M", 5)],
    ("spkA", "spkA_u1"): [("M", 5), ("AA", 6), ("sp", 4), ("S", 6), ("IY", 5)],
    ("spkB", "spkB_u0"): [("IY", 6), ("M", 6), ("sp", 4), ("AA", 5), ("S", 6)],
    ("spkB", "spkB_u1"): [("S", 7), ("IY", 5), ("AA", 6), ("M", 6)],
}


def config(root):
    return {"path": {"raw_path": os.path.join(root, "raw"), "preprocessed_path": os.path.join(root, "out")},
            "preprocessing": {"val_size": 0, "audio": {"sampling_rate": SAMPLING_RATE, "max_wav_value": 32768.0},
                              "stft": {"filter_length": FILTER, "hop_length": HOP, "win_length": FILTER},
                              "mel": {"n_mel_channels": 80, "mel_fmin": 0, "mel_fmax": 8000},
                              "pitch": {"feature": "phoneme_level", "normalization": True},
                              "energy": {"feature": "phoneme_level", "normalization": True}},
            "subsets": {"train": "train"}}


def phones(speaker, basename):
    return [p for p, _ in UTTERANCES[(speaker, basename)]]


def waveform(segments, seed):
    """frames x HOP samples minus one hop's worth of slack, so that len // HOP + 1 == the frame count."""
    r = np.random.default_rng(seed)
    parts = []
    for p, frames in segments:
        t = np.arange(frames * HOP) / SAMPLING_RATE
        tone = 0.3 * np.sin(2 * np.pi * TONES[p] * t) if TONES[p] > 0 else np.zeros(len(t))
        parts.append(tone + 1e-3 * r.standard_normal(len(t)))
    wav = np.concatenate(parts).astype(np.float32)
    return wav[: len(wav) - HOP // 2]


def write_raw(root):
    from scipy.io import wavfile
    cfg = config(root)
    for k, ((spk, base), segs) in enumerate(sorted(UTTERANCES.items())):
        d = os.path.join(cfg["path"]["raw_path"], "train", spk)
        os.makedirs(d, exist_ok=True)
        wavfile.write(os.path.join(d, base + ".wav"), SAMPLING_RATE, waveform(segs, k))
        with open(os.path.join(d, base + ".lab"), "w") as f:
            f.write(f"raw text of {base}\n")
    return cfg
