"""Device preprocessing stage (csrc/preprocess.h through include/mtts.h: mtts_stft_mel_batch / phoneme_average / outlier_stats /
merge_stats / normalize, meta_tts_amd/preprocessor.py) against tests/golden/preprocess.npz — the outputs of the reference's own
`Preprocessor.build_from_path` on a tiny synthetic corpus (tests/golden/make_preprocess_golden.py).  The small STFT configurations
run through the SIMT emulator on the CPU; the same checks and the LibriTTS configuration run on the MI355X.

Gates (and where they come from):
  * mel / frame energy vs the fixture: the project's own front-end gates — GPU mel atol 5e-5, energy rtol = atol 1e-5; emulator mel
    atol 2e-4, energy rtol = atol 2e-5 (the GEMMs are the ones tests/test_stft.py checks).
  * everything float64 in, float64 math (phoneme pitch, its statistics, normalised pitch, min / max; the statistics / normalise
    kernels fed the fixture's own values): rtol 1e-12 — a mean over d <= 64 frames and a merge over <= 1e3 values differ from the
    reference by summation order only, <= ~1e3 * 2^-53 ~ 1e-13.
  * float32 segment means fed the fixture's frame energy: rtol 1e-5 (d * 2^-24, d <= 64).
  * end to end (device STFT -> energy): with gate_E the frame-energy rtol above, |d phoneme energy| <= gate_E * value + d * 2^-24 (a
    mean is a convex combination), |d mean| <= gate_E * mean|x|, |d std| <= gate_E * rms(x) (std is 1-Lipschitz in the rms of the
    perturbation).  The normalised energy on disk is (e - mean) / std, so its error is bounded by
    (|d e| + |d mean|) / std + |normalised| * |d std| / std; the same bound holds for its min / max.
  * exact: durations, phones, metadata lines, speakers.json, frame counts, dropped utterances, keep masks, file names, shapes, dtypes."""
import json
import os

import numpy as np
import pytest

import __graft_entry__ as ge
from meta_tts_amd import data as D
from meta_tts_amd import preprocessor as P

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "preprocess.npz"))
EMU = dict(mel=2e-4, energy=2e-5)
GPU = dict(mel=5e-5, energy=1e-5)
SMALL_TAGS = ["small", "small_frame"]
ALL_TAGS = SMALL_TAGS + ["libritts"]


def _s(key):
    return str(G[key][()])


class _Corpus:
    """The inputs of one fixture run: config, utterances, tiers, waveforms, f0."""

    def __init__(self, tag, root, lib_path):
        self.tag, self.name = tag, _s(f"{tag}|corpus")
        self.cfg = {"path": {"raw_path": os.path.join(root, "raw"), "preprocessed_path": os.path.join(root, "out")},
                    "preprocessing": json.loads(_s(f"{tag}|cfg")), "subsets": {"train": "train"}}
        self.utts = [u.split("/") for u in G[f"{self.name}|utts"]]
        longest = max(len(G[f"{self.name}|{b}|wav"]) for _, b in self.utts)
        self.pp = P.Preprocessor(self.cfg, max_samples=longest + 64, lib_path=lib_path)
        self.kept = [ln.split("|")[0] for ln in _s(f"{tag}|train_txt").split("\n")]
        self.phoneme = self.cfg["preprocessing"]["pitch"]["feature"] == "phoneme_level"
        for kind in ("mel", "pitch", "energy", "duration"):
            os.makedirs(os.path.join(self.pp.out_dir, kind), exist_ok=True)

    def tier(self, base):
        k = f"{self.name}|{base}|tg_"
        return P.Tier("phones", [P.Interval(float(a), float(b), str(t)) for a, b, t in zip(G[k + "start"], G[k + "end"], G[k + "text"])])

    def item(self, spk, base):
        sr = self.pp.sampling_rate
        phones, durations, start, end = self.pp.get_alignment(self.tier(base))
        wav = G[f"{self.name}|{base}|wav"][int(sr * start): int(sr * end)]
        return (spk, base, wav, phones, durations, G[f"{self.name}|{base}|f0"], f"raw text of {base}")

    def items(self):
        return [self.item(s, b) for s, b in self.utts]

    def write_raw(self):
        """The corpus as files: float32 wavs, long-format TextGrids (with a words tier and an empty interval to skip), .lab texts."""
        from scipy.io import wavfile
        f0 = {}
        for spk, base in self.utts:
            d, t = os.path.join(self.pp.in_dir, "train", spk), os.path.join(self.pp.out_dir, "TextGrid", spk)
            os.makedirs(d, exist_ok=True)
            os.makedirs(t, exist_ok=True)
            wavfile.write(os.path.join(d, base + ".wav"), self.pp.sampling_rate, G[f"{self.name}|{base}|wav"])
            open(os.path.join(d, base + ".lab"), "w").write(f"raw text of {base}\nsecond line\n")
            ivs = self.tier(base)._objects
            xmax = ivs[-1].end_time + 0.01
            lines = ['File type = "ooTextFile"', 'Object class = "TextGrid"', "", "xmin = 0.0", f"xmax = {xmax!r}", "tiers? <exists>", "size = 2", "item []:",
                     "\titem [1]:", '\t\tclass = "IntervalTier"', '\t\tname = "words"', "\t\txmin = 0.0", f"\t\txmax = {xmax!r}", "\t\tintervals: size = 1",
                     "\t\t\tintervals [1]:", "\t\t\t\txmin = 0.0", f"\t\t\t\txmax = {xmax!r}", '\t\t\t\ttext = "words"',
                     "\titem [2]:", '\t\tclass = "IntervalTier"', '\t\tname = "phones"', "\t\txmin = 0.0", f"\t\txmax = {xmax!r}",
                     f"\t\tintervals: size = {len(ivs) + 1}"]
            for k, iv in enumerate(ivs):
                lines += [f"\t\t\tintervals [{k + 1}]:", f"\t\t\t\txmin = {iv.start_time!r}", f"\t\t\t\txmax = {iv.end_time!r}", f'\t\t\t\ttext = "{iv.text}"']
            lines += [f"\t\t\tintervals [{len(ivs) + 1}]:", f"\t\t\t\txmin = {ivs[-1].end_time!r}", f"\t\t\t\txmax = {xmax!r}", '\t\t\t\ttext = ""']
            open(os.path.join(t, base + ".TextGrid"), "w").write("\n".join(lines) + "\n")
            it = self.item(spk, base)
            f0[(len(it[2]), float(it[2][0]), float(it[2][-1]))] = it[5]
        assert len(f0) == len(self.utts)
        return lambda wav, sr, hop: f0[(len(wav), float(wav[0]), float(wav[-1]))]


def _assert_mel(mel, ref, atol):
    assert mel.shape == ref.shape and mel.dtype == np.float32
    live = ref > np.log(2e-5)       # log of a clamped value: compared above the clamp, at the clamp elsewhere (tests/test_stft.py)
    print("mel max |d|", float(np.abs(mel[live] - ref[live]).max()), "gate", atol)
    np.testing.assert_allclose(mel[live], ref[live], rtol=0, atol=atol)
    assert np.all(mel[~live] <= np.log(3e-5))


def _all_kept(c, feat):
    return np.concatenate([G[f"{c.tag}|{b}|{feat}_raw"][G[f"{c.tag}|{b}|{feat}_keep"]] for b in c.kept]).astype(np.float64)


# ---- process_utterances: raw (un-normalised) values, keep masks, frame counts, drops ------------------------------------------------
def _check_utterances(lib_path, tag, gate, tmp_path):
    c = _Corpus(tag, str(tmp_path), lib_path)
    res = c.pp.process_utterances(c.items())
    assert [r is not None for r in res] == [b in c.kept for _, b in c.utts]                      # dropped utterances
    assert [r.info for r in res if r is not None] == _s(f"{tag}|train_txt").split("\n")          # phones / metadata lines
    for (spk, base), r, it in zip(c.utts, res, c.items()):
        if r is None:
            continue
        k = f"{tag}|{base}|"
        dur = np.load(os.path.join(c.pp.out_dir, "duration", f"{spk}-duration-{base}.npy"))
        assert dur.dtype == np.int64 and np.array_equal(dur, G[k + "duration"]) and r.n_frames == G[k + "mel"].shape[0] == dur.sum()
        _assert_mel(np.load(os.path.join(c.pp.out_dir, "mel", f"{spk}-mel-{base}.npy")), G[k + "mel"], gate["mel"])
        pitch = np.load(os.path.join(c.pp.out_dir, "pitch", f"{spk}-pitch-{base}.npy"))
        energy = np.load(os.path.join(c.pp.out_dir, "energy", f"{spk}-energy-{base}.npy"))
        assert pitch.dtype == np.float64 and energy.dtype == np.float32
        assert pitch.shape == G[k + "pitch_raw"].shape and energy.shape == G[k + "energy_raw"].shape
        np.testing.assert_allclose(pitch, G[k + "pitch_raw"], rtol=1e-12, atol=0)
        ref = G[k + "energy_raw"].astype(np.float64)
        d = dur if c.phoneme else np.ones(len(ref))
        err = np.abs(energy - ref)
        print(base, "energy max |d| / value", float((err / np.maximum(ref, 1e-30))[ref > 0].max()), "gate", gate["energy"])
        assert np.all(err <= gate["energy"] * np.abs(ref) + d * 2.0 ** -24)
        assert np.array_equal(r.pitch, pitch[G[k + "pitch_keep"]]) and np.array_equal(r.energy, energy[G[k + "energy_keep"]])   # keep masks
        assert r.pitch_partial[0] == G[k + "pitch_keep"].sum() and r.energy_partial[0] == G[k + "energy_keep"].sum()
    c.pp.close()


# ---- the segment / outlier / statistics / normalise kernels fed the fixture's own values (isolated from the STFT) ----------------------
def _check_isolated(lib_path, tag, tmp_path):
    c = _Corpus(tag, str(tmp_path), lib_path)
    pp, items = c.pp, {it[1]: it for it in c.items()}
    durs = [items[b][4] for b in c.kept]
    if c.phoneme:
        fe = [G[f"{tag}|{b}|frame_energy"][: sum(d)] for b, d in zip(c.kept, durs)]
        for b, e in zip(c.kept, pp.phoneme_average(fe, durs)):
            assert e.dtype == np.float32
            np.testing.assert_allclose(e, G[f"{tag}|{b}|energy_raw"], rtol=1e-5, atol=0)
        f0 = [np.asarray(items[b][5], np.float64)[: sum(d)] for b, d in zip(c.kept, durs)]
        for b, p in zip(c.kept, pp.phoneme_average(f0, durs, interpolate=True)):
            np.testing.assert_allclose(p, G[f"{tag}|{b}|pitch_raw"], rtol=1e-12, atol=0)
    stats = G[f"{tag}|stats"]
    for feat, off in (("pitch", 0), ("energy", 4)):
        raw = [G[f"{tag}|{b}|{feat}_raw"] for b in c.kept]
        masks, parts = pp.outlier_stats(raw)
        for b, m, v in zip(c.kept, masks, raw):
            assert np.array_equal(m, G[f"{tag}|{b}|{feat}_keep"])
            assert np.array_equal(v[m], pp.remove_outlier(v))
        mean, std = pp.mean_std(pp.merge_stats(np.zeros(3), parts))
        np.testing.assert_allclose([mean, std], stats[off + 2: off + 4], rtol=1e-12, atol=0)
        outs, lo, hi = pp.normalize_values(raw, stats[off + 2], stats[off + 3])
        for b, o in zip(c.kept, outs):
            assert o.dtype == np.float64
            np.testing.assert_allclose(o, G[f"{tag}|{b}|{feat}"], rtol=1e-12, atol=0)
        np.testing.assert_allclose([lo, hi], stats[off: off + 2], rtol=1e-12, atol=0)
    c.pp.close()


# ---- build_from_path: the tree on disk, then the tree through data.py ------------------------------------------------------------------
def _check_tree(lib_path, tag, gate, tmp_path, engine=False):
    c = _Corpus(tag, str(tmp_path), lib_path)
    f0_fn = c.write_raw()
    outs = c.pp.build_from_path(f0_fn=f0_fn, batch_utterances=4)
    out = c.pp.out_dir
    assert outs["train"] == _s(f"{tag}|train_txt").split("\n")
    assert open(os.path.join(out, "train.txt")).read() == _s(f"{tag}|train_txt") + "\n"
    assert open(os.path.join(out, "speakers.json")).read() == _s(f"{tag}|speakers")
    files = json.loads(_s(f"{tag}|files"))
    for kind in ("mel", "pitch", "energy", "duration"):
        assert sorted(os.listdir(os.path.join(out, kind))) == files[kind]
    assert not os.path.exists(os.path.join(out, "spk_ref_mel_slices"))
    ref, got = G[f"{tag}|stats"], json.load(open(os.path.join(out, "stats.json")))
    got = np.asarray(got["pitch"] + got["energy"])
    np.testing.assert_allclose(got[:4], ref[:4], rtol=1e-12, atol=0)                       # pitch min, max, mean, std
    x = _all_kept(c, "energy")
    gE = gate["energy"]
    d_mean, d_std = abs(got[6] - ref[6]), abs(got[7] - ref[7])
    print("energy |d mean|", d_mean, "gate", gE * np.abs(x).mean(), "|d std|", d_std, "gate", gE * np.sqrt((x ** 2).mean()))
    assert d_mean <= gE * np.abs(x).mean() and d_std <= gE * np.sqrt((x ** 2).mean())
    norm_tol = lambda raw, norm, dd: ((gE * np.abs(raw) + dd * 2.0 ** -24 + d_mean) + np.abs(norm) * d_std) / ref[7] + 1e-12 * np.abs(norm)
    lo_hi = []
    for base in c.kept:
        spk, k = base.split("_")[0], f"{tag}|{base}|"
        load = lambda kind: np.load(os.path.join(out, kind, f"{spk}-{kind}-{base}.npy"))
        dur, pitch, energy = load("duration"), load("pitch"), load("energy")
        assert dur.dtype == np.int64 and np.array_equal(dur, G[k + "duration"])
        _assert_mel(load("mel"), G[k + "mel"], gate["mel"])
        assert pitch.dtype == G[k + "pitch"].dtype == np.float64 and energy.dtype == G[k + "energy"].dtype == np.float64
        np.testing.assert_allclose(pitch, G[k + "pitch"], rtol=1e-12, atol=0)
        dd = dur if c.phoneme else np.ones(len(energy))
        tol = norm_tol(G[k + "energy_raw"].astype(np.float64), G[k + "energy"], dd)
        assert energy.shape == G[k + "energy"].shape and np.all(np.abs(energy - G[k + "energy"]) <= tol)
        i, j = int(np.argmin(G[k + "energy"])), int(np.argmax(G[k + "energy"]))
        lo_hi.append((G[k + "energy"][i], tol[i], G[k + "energy"][j], tol[j]))
    lo, hi = min(lo_hi, key=lambda t: t[0]), max(lo_hi, key=lambda t: t[2])
    assert abs(got[4] - ref[4]) <= max(t[1] for t in lo_hi) and abs(got[5] - ref[5]) <= max(t[3] for t in lo_hi), (got[4:6], ref[4:6], lo, hi)
    # a second corpus keeps the first one's mean / std (preprocessor.py:120-139): the files are normalised a second time with them
    before = np.load(os.path.join(out, "pitch", files["pitch"][0]))
    c.pp.build_from_path(f0_fn=f0_fn, batch_utterances=2)
    again = json.load(open(os.path.join(out, "stats.json")))
    assert again["pitch"][2:] == list(got[2:4]) and again["energy"][2:] == list(got[6:8])
    assert np.load(os.path.join(out, "pitch", files["pitch"][0])).shape == before.shape
    c.pp.close()
    # ---- round trip: tree -> FeatureDataset -> collate gives the 12-tuple with the fixture's values
    c2 = _Corpus(tag, str(tmp_path / "rt"), lib_path)
    c2.pp.build_from_path(f0_fn=c2.write_raw(), batch_utterances=3)
    c2.pp.close()
    vocab = {p: i + 1 for i, p in enumerate(sorted({str(t) for _, b in c.utts for t in G[f"{c.name}|{b}|tg_text"]}))}
    ds = D.FeatureDataset(c2.pp.out_dir, "train.txt", lambda text: [vocab[p] for p in text.strip("{}").split(" ")])
    assert len(ds) == len(c.kept) and ds.speaker_map == json.loads(_s(f"{tag}|speakers"))
    batch = D.reprocess([ds[i] for i in range(len(ds))], np.arange(len(ds)))
    ids, raw, spk, texts, tlens, tmax, mels, mlens, mmax, pit, ene, dur = batch
    assert ids == c.kept and raw == [f"raw text of {b}" for b in c.kept]
    assert list(spk) == [ds.speaker_map[b.split("_")[0]] for b in c.kept]
    assert list(tlens) == [len(G[f"{tag}|{b}|duration"]) for b in c.kept] and list(mlens) == [G[f"{tag}|{b}|mel"].shape[0] for b in c.kept]
    for i, b in enumerate(c.kept):
        k = f"{tag}|{b}|"
        assert np.array_equal(dur[i, : tlens[i]], G[k + "duration"]) and not dur[i, tlens[i]:].any()
        n = len(G[k + "pitch"])
        np.testing.assert_allclose(pit[i, :n], G[k + "pitch"].astype(np.float32), rtol=1e-6, atol=0)        # the collate casts pitch to float32
        dd = G[k + "duration"] if c.phoneme else np.ones(n)
        assert np.all(np.abs(ene[i, :n] - G[k + "energy"]) <= norm_tol(G[k + "energy_raw"].astype(np.float64), G[k + "energy"], dd))
        _assert_mel(mels[i, : mlens[i]], G[k + "mel"], gate["mel"])
    if engine:
        from meta_tts_amd import synth
        from meta_tts_amd.config import ModelDims
        from meta_tts_amd.engine import Engine
        dims = ModelDims()
        assert dims.n_mel == mels.shape[2]
        eng = Engine(dims, max_tasks=1, max_B=len(ids), max_S=int(tmax) + 8, max_T=int(mmax) + 8)
        eng.load_params(synth.make_params(dims, 0))
        eng.set_batches(0, [batch])
        eng.forward(0, use_fast=False, train=True)
        loss = eng.loss(0)
        eng.synchronize()
        eng.close()
        print("engine loss on the preprocessed batch", loss[0])
        assert np.all(np.isfinite(loss))


# ---- batch invariance ---------------------------------------------------------------------------------------------------------------------
def _check_invariance(lib_path, tag, tmp_path):
    c = _Corpus(tag, str(tmp_path), lib_path)
    items = c.items()

    def run(groups):
        got = {}
        for g in groups:
            for i, r in zip(g, c.pp.process_utterances([items[i] for i in g])):
                if r is None:
                    got[i] = None
                    continue
                spk, base = c.utts[i]
                files = tuple(np.load(os.path.join(c.pp.out_dir, kind, f"{spk}-{kind}-{base}.npy")).tobytes() for kind in ("mel", "pitch", "energy", "duration"))
                got[i] = files + (r.pitch.tobytes(), r.energy.tobytes(), r.pitch_partial.tobytes(), r.energy_partial.tobytes(), r.n_frames)
        live = [i for i in range(len(items)) if got[i] is not None]
        stats = [c.pp.merge_stats(np.zeros(3), np.stack([np.frombuffer(got[i][k], np.float64) for i in live])).tobytes() for k in (6, 7)]
        return got, stats

    n = len(items)
    one = run([list(range(n))])
    two = run([list(range(n // 2)), list(range(n // 2, n))])
    perm = run([list(np.random.RandomState(3).permutation(n))])
    single = run([[i] for i in range(n)])
    for other in (two, perm, single):
        assert other[0] == one[0]        # per-utterance outputs bit-identical
        assert other[1] == one[1]        # statistics merged in the original order bit-identical
    c.pp.close()


def _check_errors(lib_path, tmp_path):
    from meta_tts_amd.engine import MttsError
    c = _Corpus("small", str(tmp_path), lib_path)
    pp = c.pp
    w = np.zeros(200, np.float32)
    with pytest.raises(MttsError, match="too short"):
        pp.mel_batch([w, w[:32]])                                               # n_samples <= filter_length / 2
    with pytest.raises(MttsError, match="no frame|keep_frames"):
        pp.mel_batch([w], [0])
    v = np.arange(1, 7, dtype=np.float64)
    with pytest.raises(MttsError, match="S > T"):
        pp.phoneme_average([v], [[1] * 7])
    with pytest.raises(MttsError, match="negative duration"):
        pp.phoneme_average([v], [[3, -1, 2]])
    with pytest.raises(MttsError, match="no voiced frame"):
        pp.phoneme_average([np.zeros(6)], [[3, 3]], interpolate=True)
    with pytest.raises(MttsError, match="std == 0"):
        pp.normalize_values([v], 0.0, 0.0)
    with pytest.raises(MttsError, match="4096"):
        pp.outlier_stats([np.zeros(5000, np.float32)])
    mels, en = pp.mel_batch([w + 0.1, w[:100] + 0.2], [-1, 3])                 # still usable after the errors; keep < 0 keeps all
    assert [m.shape for m in mels] == [(200 // 16 + 1, 12), (3, 12)] and [e.shape for e in en] == [(13,), (3,)]
    # the aliased in-place loop on a case small enough to follow by hand: durations [1, 0, 0, 2] over [1, 2, 3, 4]
    ref = np.array([1.0, 2.0, 3.0, 4.0])
    pos = 0
    for i, d in enumerate([1, 0, 0, 2]):
        ref[i] = np.mean(ref[pos: pos + d]) if d > 0 else 0
        pos += d
    assert ref.tolist() == [1.0, 0.0, 0.0, 0.0]                                  # mean(ref[1:3]) reads the two zeros just written
    assert pp.phoneme_average([np.array([1.0, 2.0, 3.0, 4.0])], [[1, 0, 0, 2]])[0].tolist() == ref.tolist()
    pp.close()


def test_textgrid_reader_and_alignment(tmp_path):
    """The long-format reader drops empty intervals and other tiers; get_alignment trims silences and rounds as the reference does."""
    c = _Corpus("small", str(tmp_path), ge.build_emulator())
    c.write_raw()
    for spk, base in c.utts:
        tg = P.read_textgrid(os.path.join(c.pp.out_dir, "TextGrid", spk, base + ".TextGrid"))
        assert [t.name for t in tg.tiers] == ["words", "phones"]
        got, want = tg.get_tier_by_name("phones")._objects, c.tier(base)._objects
        assert [tuple(x) for x in got] == [tuple(x) for x in want]
        phones, durations, start, end = c.pp.get_alignment(tg.get_tier_by_name("phones"))
        assert phones[0] == "T" and phones[-1] == "IY1" and "sp" in phones and "sil" not in phones
        assert start == want[0].end_time and end == want[-2].end_time and len(phones) == len(durations)
        if base in c.kept:
            assert durations == G[f"small|{base}|duration"].tolist()
    with pytest.raises(P.MttsError, match="pyworld"):
        P.pyworld_f0(np.zeros(100, np.float32), 8000, 16)
    c.pp.close()


@pytest.mark.parametrize("tag", SMALL_TAGS)
def test_process_utterances_emulator(tag, tmp_path):
    _check_utterances(ge.build_emulator(), tag, EMU, tmp_path)


@pytest.mark.parametrize("tag", SMALL_TAGS)
def test_kernels_on_fixture_values_emulator(tag, tmp_path):
    _check_isolated(ge.build_emulator(), tag, tmp_path)


@pytest.mark.parametrize("tag", SMALL_TAGS)
def test_tree_and_round_trip_emulator(tag, tmp_path):
    _check_tree(ge.build_emulator(), tag, EMU, tmp_path)


def test_batch_invariance_emulator(tmp_path):
    _check_invariance(ge.build_emulator(), "small", tmp_path)


def test_named_errors_emulator(tmp_path):
    _check_errors(ge.build_emulator(), tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ALL_TAGS)
def test_process_utterances_gpu(tag, tmp_path):
    ge.build_device()
    _check_utterances(None, tag, GPU, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ALL_TAGS)
def test_kernels_on_fixture_values_gpu(tag, tmp_path):
    ge.build_device()
    _check_isolated(None, tag, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ALL_TAGS)
def test_tree_and_round_trip_gpu(tag, tmp_path):
    ge.build_device()
    _check_tree(None, tag, GPU, tmp_path, engine=tag == "libritts")


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["small", "libritts"])
def test_batch_invariance_gpu(tag, tmp_path):
    ge.build_device()
    _check_invariance(None, tag, tmp_path)


@pytest.mark.gpu
def test_named_errors_gpu(tmp_path):
    ge.build_device()
    _check_errors(None, tmp_path)
