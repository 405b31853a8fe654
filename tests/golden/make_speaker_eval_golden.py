"""Writes tests/golden/speaker_eval.npz: the outputs of the reference's own evaluation code on seeded synthetic d-vectors.

    python tests/golden/make_speaker_eval_golden.py /path/to/reference

Runs on the CPU.  It imports, from <reference>/evaluation: `PairSimilarity.compute_pair_similarity`,
`WavsToDvector.get_centroid_dvector_list`, `CentroidSimilarity.get_centroid_similarity` (with its `custom_shuffle`) and
`SpeakerVerification.get_eer`; the AUC is sklearn's roc_curve / auc on the scores speaker_verification.py:301-305 builds (real
positives labelled 1, the mode's positives labelled 0).  Modules the reference imports but that are not needed for these functions
(resemblyzer, torchaudio, seaborn, ...) are stubbed when absent.  Only arrays are stored, next to float64 evaluations of the same
formulas on the same float32 inputs (the arbiter's third party)."""
import importlib
import io
import os
import random
import sys
import tempfile
from unittest import mock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
N_SPEAKER, N_SAMPLE, DIM = 4, 3, 256
MIN_GAP = 1e-6
MODES = [("m1", [0, 5]), ("m5", [0])]          # m1: one output per task; m5: the five-fold (1-shot) layout


def _stub_missing(names):
    for name in names:
        try:
            importlib.import_module(name)
        except Exception:  # noqa: BLE001
            m = mock.MagicMock(name=name)
            m.__path__ = []
            sys.modules[name] = m


def dvectors(g, speaker_means, speakers, noise=0.35):
    """ReLU-like non-negative unit vectors around their speaker's mean (what the encoder's head produces)."""
    v = np.maximum(speaker_means[speakers] + noise * g.standard_normal((len(speakers), DIM)), 0)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def cos64(a, b, eps=1e-6):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return (a * b).sum(1) / (np.maximum(np.linalg.norm(a, axis=1), eps) * np.maximum(np.linalg.norm(b, axis=1), eps))


def main(reference):
    sys.path.insert(0, os.path.join(reference, "evaluation"))
    _stub_missing(["resemblyzer", "torchaudio", "seaborn", "tqdm", "tqdm.contrib", "matplotlib", "matplotlib.pyplot", "pylab", "PIL"])
    import torch  # noqa: F401
    from sklearn.metrics import auc, roc_curve
    import config as ref_config
    ref_config.corpus = "Synthetic"
    ref_config.n_speaker, ref_config.n_sample = N_SPEAKER, N_SAMPLE
    ref_config.mode_step_list = MODES
    from centroid_similarity import CentroidSimilarity
    from pair_similarity import PairSimilarity
    from speaker_verification import SpeakerVerification
    from wavs_to_dvector import WavsToDvector

    g = np.random.default_rng(22)   # the first seed from 20 on for which the MIN_GAP assertions below hold
    means = np.abs(g.standard_normal((1, DIM)) + 0.12 * g.standard_normal((N_SPEAKER, DIM)))   # close speakers: the two score classes overlap, EER > 0
    spk_of_test = np.repeat(np.arange(N_SPEAKER), N_SAMPLE)
    out = {"n_speaker": N_SPEAKER, "n_sample": N_SAMPLE, "modes": np.asarray([f"{m}_step{s}" for m, steps in MODES for s in steps])}
    dv = {"recon": dvectors(g, means, spk_of_test, 0.25), "real": dvectors(g, means, spk_of_test, 0.2)}
    for m, steps in MODES:
        for k, s in enumerate(steps):
            spk = np.repeat(spk_of_test, 5) if m == "m5" else spk_of_test
            dv[f"{m}_step{s}"] = dvectors(g, means, spk, 0.5 - 0.1 * k)
    # pairs: 4 positives of the sample's speaker, 4 negatives of four... (here: of the other speakers, cycled)
    pos_spk = np.repeat(spk_of_test, 4)
    neg_spk = np.asarray([[(s + 1 + j % (N_SPEAKER - 1)) % N_SPEAKER for j in range(4)] for s in spk_of_test]).reshape(-1)
    assert not np.any(neg_spk == pos_spk)
    dv["pair"] = np.stack([dvectors(g, means, pos_spk), dvectors(g, means, neg_spk)])
    enroll_sizes = [3, 5, 4, 6]                 # ragged
    enrollment = [dvectors(g, means, np.full(n, s)) for s, n in enumerate(enroll_sizes)]
    for k, v in dv.items():
        out[f"dvector|{k}"] = v
    out["enrollment"] = np.concatenate(enrollment)
    out["enrollment_sizes"] = np.asarray(enroll_sizes)

    # ---- centroids (wavs_to_dvector.py:176-183) ----
    w = object.__new__(WavsToDvector)
    w.n_speaker = N_SPEAKER
    centroid = np.asarray(w.get_centroid_dvector_list(enrollment))
    assert centroid.dtype == np.float32
    out["centroid"] = centroid
    c64 = np.stack([e.astype(np.float64).mean(0) for e in enrollment])
    c64 /= np.linalg.norm(c64, axis=1, keepdims=True)
    out["centroid_f64"] = c64
    dv["centroid"] = centroid

    # ---- pair similarity (pair_similarity.py:68-88) ----
    p = PairSimilarity()
    p.dvector_list_dict = dv
    pair_sim = {}
    for mode in ["recon", "real"] + list(out["modes"]):
        ps = p.compute_pair_similarity(dv[mode])
        assert ps.dtype == np.float32 and ps.shape == (2, 4 * len(dv[mode]))
        pair_sim[mode] = ps
        out[f"pair_sim|{mode}"] = ps
        rep = np.repeat(dv[mode], 4, axis=0)
        pr = dv["pair"] if len(rep) == dv["pair"].shape[1] else np.repeat(dv["pair"], 5, axis=1)
        out[f"pair_sim_f64|{mode}"] = np.stack([cos64(rep, pr[0]), cos64(rep, pr[1])])

    # ---- centroid similarity (centroid_similarity.py:45-124), with one recorded shuffle ----
    with tempfile.TemporaryDirectory() as tmp:
        cwd = os.getcwd()
        os.chdir(tmp)
        try:
            os.makedirs("npy/Synthetic")
            os.makedirs("txt/Synthetic")
            c = object.__new__(CentroidSimilarity)
            c.corpus, c.n_speaker, c.n_sample, c.mode_step_list = "Synthetic", N_SPEAKER, N_SAMPLE, MODES
            c.dvector_list_dict = dv
            random.seed(7)
            labelled = c.custom_shuffle(np.arange(N_SPEAKER, dtype=np.float32)[:, None]).numpy().reshape(-1).astype(np.int64)
            count, shuffle_map = [0] * N_SPEAKER, []
            for s in labelled:                    # the index map custom_shuffle builds: target speaker * n_sample + its running count
                shuffle_map.append(int(s) * N_SAMPLE + count[s])
                count[s] += 1
            out["shuffle_map"] = np.asarray(shuffle_map)
            random.seed(7)
            stdout, sys.stdout = sys.stdout, io.StringIO()
            try:
                c.get_centroid_similarity()
            finally:
                sys.stdout = stdout
            for mode, sim in c.similarity_list_dict.items():
                assert sim.dtype == np.float32
                out[f"centroid_sim|{mode}"] = sim
                test = dv["recon"] if mode == "recon_random" else dv[mode]
                idx = labelled if mode == "recon_random" else np.arange(len(test)) // (len(test) // N_SPEAKER)
                out[f"centroid_sim_f64|{mode}"] = cos64(c64[idx], test)

            # ---- EER (speaker_verification.py:32-59) and AUC (:301-305) ----
            v = object.__new__(SpeakerVerification)
            v.output_path = "txt/Synthetic/eer.txt"
            v.pair_similarity_dict = pair_sim
            stdout, sys.stdout = sys.stdout, io.StringIO()
            try:
                v.get_eer()
            finally:
                sys.stdout = stdout
            out["eer_txt"] = open(v.output_path).read()
        finally:
            os.chdir(cwd)
    for mode, ps in pair_sim.items():
        # no two scores of opposite label may tie, else EER / AUC / threshold would depend on how equal scores are ordered — and they are kept
        # 1e-6 apart (MIN_GAP), so that similarities that differ from these in the last float32 bits (2e-7) give the same EER and AUC
        gap = np.abs(ps[0][:, None].astype(np.float64) - ps[1][None, :]).min()
        assert gap >= MIN_GAP, (mode, gap)
        both = np.concatenate([pair_sim["real"][0], ps[0]]).astype(np.float64)
        if mode != "real":
            assert np.abs(pair_sim["real"][0][:, None].astype(np.float64) - ps[0][None, :]).min() >= MIN_GAP, mode   # (the AUC's two classes)
        out[f"eer|{mode}"] = np.float64(v.eer_dict[mode])
        out[f"threshold|{mode}"] = np.asarray(v.threshold_dict[mode])
        if ps.shape[1] == pair_sim["real"].shape[1]:   # (the reference's labels assume as many real scores as mode scores: not the five-fold layout)
            fpr, tpr, _ = roc_curve(np.repeat(np.array([1, 0]), ps.shape[1]), both, pos_label=1)
            out[f"auc|{mode}"] = np.float64(auc(fpr, tpr))
        print(mode, "eer", v.eer_dict[mode], "threshold", v.threshold_dict[mode], "auc", out.get(f"auc|{mode}"))
    np.savez_compressed(os.path.join(HERE, "speaker_eval.npz"), **out)
    print("wrote", os.path.join(HERE, "speaker_eval.npz"), os.path.getsize(os.path.join(HERE, "speaker_eval.npz")), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
