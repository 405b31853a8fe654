"""The flat-start monophone aligner (csrc/align.h through include/mtts.h: mtts_align_*; meta_tts_amd/align.py).  CPU tests run the device
code through the SIMT emulator; the `gpu` parameter of the same tests runs it on the MI355X.

The definition is the project's own (include/mtts.h), restated in float64 numpy in the same order in tests/align_oracle.py, and the
oracle's lattice likelihood is itself pinned to torch's CTC loss in float64.  Device and oracle are both float64, so the gates are
worst-case rounding bounds, not measured figures.  With u = 2^-53:
  * an emission is a sum of F brackets, each (a subtraction, two products with a once-rounded reciprocal, a logarithm, an addition)
    plus the running addition: at most (F + 8) u B of error, B = the largest sum_f (|(x - mu)^2 / var| + |log(2 pi var)|) of the case.
  * a frame of the forward pass is one logsumexp of at most three terms plus one add.  logsumexp is 1-Lipschitz in its terms, so the
    error it inherits does not grow; its own error is the differences (each term enters the sum with at most u |a - m| exp(a - m) <=
    u / e), three exponentials and a logarithm of a value in [1, 3] at up to 3 ulp each (the bound the OpenCL specification allows a
    double-precision exp / log), and two additions: under 16 u in all.  Adding m and adding the emission round values bounded by A = max
    |alpha|: 2 u A.  Per frame: (F + 8) u B + 2 u A + 16 u; over T frames, x 4 for the compiler's freedom to contract a multiply-add
    (which changes single roundings, not the bound's order):  |LL - LL_oracle| <= G = 4 T ((F + 8) B + 2 A + 16) u.
  * gamma = exp((alpha + beta) - LL): alpha's error up to frame t and beta's from frame t on together are at most G, LL's is G, the two
    additions 2 u A and the exponential 3 ulp: the exponent is off by at most 3 G, so |gamma - gamma_oracle| <= 3 G gamma_oracle (+ the
    smallest normal number, for values that underflow).
  * the model after one iteration from the SAME starting model: every gamma carries a relative error r0 <= 3 G, every per-state sum
    over T frames, per-utterance sum over S states and fold over n utterances another (T + S + n) u, the two divisions and the floor 4 u:
    r = 2 r0 + (T + S + n + 4) u, |mu - mu_oracle| <= 4 r max|x|, |var - var_oracle| <= 4 . 3 r max x^2 (the quotient, and mu^2 twice).
    The EM test feeds the oracle the device's own previous model before every iteration, so that this one-step bound is all there is.
Durations, back-pointers and end states are exact, which needs every decision on the oracle's path to be safe from rounding: the
oracle reports its smallest decision margin (best against second-best finite predecessor along the path, and between the end states,
relative to the score) and every case asserts it above 1e-9.  The constructed tie cases have margin 0 by construction and pin the tie
rules instead; so do the decisions between two adjacent states of one class ("same_class_adjacent"), whose candidates are the same
additions of the same numbers — exact ties in any arithmetic, left out of that case's margin and asserted to be there."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import align_oracle as O
import align_tree
from meta_tts_amd import _lib
from meta_tts_amd import align as A
from meta_tts_amd.engine import MttsError

U = 2.0 ** -53
MARGIN = 4.0
TINY = 2.3e-308
SHOW = bool(os.environ.get("MTTS_SELFTEST_ALIGN_SHOW"))    # print every measured figure next to its gate (python -m pytest -s)


def show(*a):
    if SHOW:
        print("[align]", *a)


@pytest.fixture(scope="module", params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def lib_path(request):
    return ge.build_emulator() if request.param == "emu" else ge.build_device()


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Dev:
    """A raw mtts_align handle."""

    def __init__(self, lib_path, n_feat=8, n_classes=6, max_frames=320, max_states=512, max_cells=1 << 22, max_utts=64, model=None):
        self.lib = _lib.load(lib_path)
        self.F, self.V = n_feat, n_classes
        self.h = C.c_void_p()
        if self.lib.mtts_align_create(n_feat, n_classes, max_frames, max_states, max_cells, max_utts, 0, C.byref(self.h)) != 0:
            raise MttsError(self.lib.mtts_align_last_error(None).decode())
        if model is not None:
            self.set_model(model)

    def check(self, rc):
        if rc != 0:
            assert rc < 0
            raise MttsError(self.lib.mtts_align_last_error(self.h).decode())

    def error(self):
        return self.lib.mtts_align_last_error(self.h).decode()

    def set_model(self, m):
        self.check(self.lib.mtts_align_set_model(self.h, *[_ptr(np.ascontiguousarray(a, np.float64)) for a in (m.mean, m.var, m.gvar)]))

    def get_model(self):
        mean, var, g = np.empty((self.V, self.F)), np.empty((self.V, self.F)), np.empty(self.F)
        self.check(self.lib.mtts_align_get_model(self.h, _ptr(mean), _ptr(var), _ptr(g)))
        return O.Model(mean, var, g)

    @staticmethod
    def pack(utts):
        """[(x, cls, opt)] -> the arrays of a batch entry, in its argument order."""
        return [len(utts), np.asarray([len(u[0]) for u in utts], np.int32), np.asarray([len(u[1]) for u in utts], np.int32),
                np.ascontiguousarray(np.concatenate([np.asarray(u[1], np.int32) for u in utts])),
                np.ascontiguousarray(np.concatenate([np.asarray(u[2], np.uint8) for u in utts])),
                np.ascontiguousarray(np.concatenate([np.asarray(u[0], np.float32) for u in utts]))]

    def flat_start(self, utts):
        n, T, _, _, _, x = self.pack(utts)
        self.check(self.lib.mtts_align_flat_start(self.h, n, _ptr(T), _ptr(x)))

    def posteriors(self, utts):
        n, T, S, c, o, x = self.pack(utts)
        cells = T.astype(np.int64) * S
        ll, g = np.full(n, -7.0), np.full(int(cells.sum()), -7.0)
        self.check(self.lib.mtts_align_posteriors(self.h, n, _ptr(T), _ptr(S), _ptr(c), _ptr(o), _ptr(x), _ptr(ll), _ptr(g)))
        return ll, [a.reshape(t, s) for a, t, s in zip(np.split(g, np.cumsum(cells)[:-1]), T, S)]

    def align(self, utts):
        n, T, S, c, o, x = self.pack(utts)
        dur, score = np.full(int(S.sum()), -7, np.int32), np.full(n, -7.0)
        self.check(self.lib.mtts_align_align(self.h, n, _ptr(T), _ptr(S), _ptr(c), _ptr(o), _ptr(x), _ptr(dur), _ptr(score)))
        return np.split(dur, np.cumsum(S)[:-1]), score

    def em(self, batches):
        """One iteration over the corpus given as a list of batches -> (total LL, per-utterance LL)."""
        self.check(self.lib.mtts_align_em_begin(self.h))
        lls = []
        for b in batches:
            n, T, S, c, o, x = self.pack(b)
            ll = np.full(n, -7.0)
            self.check(self.lib.mtts_align_em_accumulate(self.h, n, _ptr(T), _ptr(S), _ptr(c), _ptr(o), _ptr(x), _ptr(ll)))
            lls.append(ll)
        total = C.c_double()
        self.check(self.lib.mtts_align_em_finish(self.h, C.byref(total)))
        return total.value, np.concatenate(lls)

    def close(self):
        self.lib.mtts_align_destroy(self.h)


def ll_gate(x, model, cls, opt):
    """G of the module docstring for one utterance (absolute)."""
    b = O.emission(x, model, cls)
    alpha, _ = O.forward(b, opt)
    a = float(np.abs(alpha[np.isfinite(alpha)]).max())
    return MARGIN * len(x) * ((x.shape[1] + 8) * O.emission_scale(x, model, cls) + 2 * a + 16) * U


# ---- inputs and their oracle results, computed once --------------------------------------------------------------------------------------------
MAX_FRAMES = 320
# name -> (T, S, F, V, optional states, classes ("distinct", "random", "pairs": every class twice in a row, or a list), seed)
CASES = {
    "1x1": (1, 1, 8, 6, (), "random", 0), "5x1": (5, 1, 8, 6, (), "random", 0), "7x7": (7, 7, 8, 9, (), "distinct", 0),
    "258x255": (258, 255, 8, 6, (), "random", 1), "259x256": (259, 256, 8, 6, (), "random", 2), "260x257": (260, 257, 8, 6, (), "random", 3),   # across the lane stride
    "maxTx3": (MAX_FRAMES, 3, 8, 6, (), "random", 0),
    "opt_first": (9, 4, 8, 6, (0,), "distinct", 0), "opt_last": (9, 4, 8, 6, (3,), "distinct", 0), "opt_both": (9, 5, 8, 6, (0, 4), "distinct", 0),
    "opt_middle": (9, 5, 8, 6, (2,), "distinct", 1), "opt_all_skipped": (2, 5, 8, 6, (0, 2, 4), "distinct", 0),
    "opt_many": (40, 21, 8, 6, tuple(range(0, 21, 2)), "random", 0),
    "F1": (12, 4, 1, 6, (1,), "random", 0), "F128": (12, 4, 128, 6, (1,), "random", 0),
    "V1_1state": (4, 1, 8, 1, (), "random", 0),
    "V1_4states": (9, 4, 8, 1, (1,), "random", 0),                      # one class, every decision an exact tie
    "same_class_adjacent": (14, 6, 8, 6, (), "pairs", 0),
}
_cache = {}


def case(name):
    if name not in _cache:
        T, S, F, V, opts, kind, seed = CASES[name]
        r = np.random.default_rng(100 + seed)
        if kind == "distinct":
            cls = r.permutation(V)[:S]
        elif kind == "pairs":
            cls = np.repeat(r.permutation(V)[:(S + 1) // 2], 2)[:S]
        else:
            cls = r.integers(0, V, S)
            for s in range(1, S):          # no class twice in a row (that is the "pairs" case): step to the next class
                if cls[s] == cls[s - 1] and V > 1:
                    cls[s] = (cls[s] + 1) % V
        opt = np.zeros(S, np.uint8)
        opt[list(opts)] = 1
        model, x = O.random_model(V, F, 200 + seed), O.random_features(T, F, 300 + seed)
        LL, gamma = O.posteriors(x, model, cls, opt)
        ties = kind == "pairs" or (V == 1 and S > 1)                    # the same class twice in a row: exact ties, decided by the tie rule
        dur, score, margin = O.align(x, model, cls, opt, ignore_exact_ties=ties)
        assert margin > 1e-9, (name, margin)
        assert not ties or O.align(x, model, cls, opt)[2] == 0.0
        assert dur.sum() == T and all(d >= 1 for d, o in zip(dur, opt) if not o)
        _cache[name] = dict(utt=(x, cls.astype(np.int32), opt), model=model, LL=LL, gamma=gamma, dur=dur, score=score, margin=margin, gate=ll_gate(x, model, cls, opt))
    return _cache[name]


# ---- 1. the oracle ----------------------------------------------------------------------------------------------------------------------------
def _ctc(log_probs, targets, blank):
    import torch
    lp = torch.from_numpy(np.ascontiguousarray(log_probs))[:, None, :]
    return -float(torch.nn.functional.ctc_loss(lp, torch.tensor([list(targets)]), torch.tensor([lp.shape[0]]), torch.tensor([len(targets)]), blank=blank,
                                               reduction="none")[0])


def test_oracle_is_torch_ctc():
    """One class per state, all distinct.  Without optional states the oracle's LL is -ctc_loss (float64, reduction none) over the class
    scores with the blank column at -inf; with one shared optional class at every even position it is CTC with that class as a finite
    blank — the two lattices are the same by construction.  1e-12 relative; measured 4e-16 and 3e-16.  The loss only: torch's CTC
    gradient assumes normalised rows and is not gamma."""
    for T, n in ((9, 4), (12, 5), (30, 7)):
        model, x = O.random_model(n + 1, 8, T), O.random_features(T, 8, T + 1)
        scores = O.class_scores(x, model)                              # [T][n + 1]: column 0 is the blank
        labels = np.arange(1, n + 1)
        _, LL = O.forward(scores[:, labels], np.zeros(n, bool))
        hard = scores.copy()
        hard[:, 0] = -np.inf
        ref = _ctc(hard, labels, 0)
        show("ctc, no blank", T, n, abs(LL - ref) / abs(ref))
        assert abs(LL - ref) <= 1e-12 * abs(ref)
        cls = np.zeros(2 * n + 1, np.int64)
        cls[1::2] = labels
        _, LL = O.forward(scores[:, cls], cls == 0)
        ref = _ctc(scores, labels, 0)
        show("ctc, finite blank", T, n, abs(LL - ref) / abs(ref))
        assert abs(LL - ref) <= 1e-12 * abs(ref)


def test_oracle_gamma_sums_to_one():
    for name in CASES:
        g = case(name)["gamma"]
        assert np.abs(g.sum(axis=1) - 1.0).max() <= 1e-12 * max(1, g.shape[0]), name


def test_oracle_gamma_is_the_derivative():
    """gamma(t, s) = d LL / d b(t, s), by central differences on a 5 x 3 case (optional middle state): 1e-7 (measured 2e-10)."""
    model, x = O.random_model(3, 4, 5), O.random_features(5, 4, 6)
    cls, opt = np.arange(3), np.asarray([0, 1, 0], bool)
    b = O.emission(x, model, cls)
    alpha, LL = O.forward(b, opt)
    gamma = np.exp(alpha + O.backward(b, opt) - LL)
    for t in range(5):
        for s in range(3):
            hi, lo = b.copy(), b.copy()
            hi[t, s] += 1e-5
            lo[t, s] -= 1e-5
            fd = (O.forward(hi, opt)[1] - O.forward(lo, opt)[1]) / 2e-5
            assert abs(fd - gamma[t, s]) <= 1e-7, (t, s, fd, gamma[t, s])


def test_oracle_unique_path():
    """T = S without optional states: one path, LL = the diagonal sum of the emissions, gamma the identity."""
    c = case("7x7")
    x, cls, opt = c["utt"]
    diag = float(np.trace(O.emission(x, c["model"], cls)))
    assert abs(c["LL"] - diag) <= c["gate"] and abs(c["score"] - diag) <= c["gate"]
    assert np.array_equal(c["dur"], np.ones(7, np.int32)) and np.abs(c["gamma"] - np.eye(7)).max() <= 3 * c["gate"]


# ---- 2. kernels against the oracle --------------------------------------------------------------------------------------------------------
def check_against(c, ll, gamma, dur, score, tag):
    G = c["gate"]
    want = c["gamma"]
    err = np.abs(gamma - want)
    show(tag, "|LL err| / gate", abs(ll - c["LL"]) / G, "gamma worst err / gate", float((err / (3 * G * want + TINY)).max()), "margin", c["margin"])
    assert abs(ll - c["LL"]) <= G and abs(score - c["score"]) <= G
    assert gamma.shape == want.shape and (err <= 3 * G * want + TINY).all()
    assert np.array_equal(dur, c["dur"])


@pytest.mark.parametrize("name", list(CASES))
def test_kernels_against_oracle(lib_path, name):
    """LL and the Viterbi score within G, gamma within 3 G gamma (module docstring); durations exactly.  Margins of the cases (oracle):
    see case().  Measured worst error / gate: emulator 0 (LL), 4.5e-5 (gamma); MI355X 3.2e-3 (LL, "7x7"), 1.9e-3 (gamma)."""
    c = case(name)
    T, S, F, V = CASES[name][:4]
    d = Dev(lib_path, F, V, max_frames=MAX_FRAMES, model=c["model"])
    try:
        ll, gamma = d.posteriors([c["utt"]])
        dur, score = d.align([c["utt"]])
    finally:
        d.close()
    check_against(c, ll[0], gamma[0], dur[0], score[0], name)


def test_tie_rules(lib_path):
    """Constructed exact ties.  F = 1, unit variances.  (a) one class, three states, six frames: every path has the same score bit for bit,
    stay wins wherever it is reachable: durations [1, 1, 4].  (b) states A, B (optional), C with means +1, -1, 3 and frames 0, 0, 3: at
    (2, C) advance from B and skip from A tie exactly ((0 - 1)^2 = (0 + 1)^2) and beat stay: advance wins, durations [1, 1, 1] (skip
    would give [2, 0, 1]).  (c) one class, states [mandatory, optional], three frames: the end states tie, S - 1 wins: [1, 2] (S - 2
    would give [3, 0])."""
    one = O.Model([[0.0]], [[1.0]], [1.0])
    abc = O.Model([[1.0], [-1.0], [3.0]], np.ones((3, 1)), [1.0])
    cases = [(one, (np.zeros((6, 1), np.float32), [0, 0, 0], [0, 0, 0]), [1, 1, 4]),
             (abc, (np.asarray([[0.0], [0.0], [3.0]], np.float32), [0, 1, 2], [0, 1, 0]), [1, 1, 1]),
             (one, (np.zeros((3, 1), np.float32), [0, 0], [0, 1]), [1, 2])]
    for model, utt, want in cases:
        dur, _, margin = O.align(utt[0], model, utt[1], utt[2])
        assert margin == 0.0 and list(dur) == want
        d = Dev(lib_path, 1, len(model.mean), model=model)
        try:
            got, _ = d.align([utt])
        finally:
            d.close()
        assert list(got[0]) == want


# ---- 3. bit identity ----------------------------------------------------------------------------------------------------------------------
def five():
    r = np.random.default_rng(7)
    utts = []
    for k, (T, S) in enumerate(((20, 5), (33, 9), (11, 3), (40, 12), (25, 7))):
        opt = np.zeros(S, np.uint8)
        opt[2::3] = 1
        utts.append((O.random_features(T, 8, 500 + k), r.integers(0, 6, S).astype(np.int32), opt))
    return utts, O.random_model(6, 8, 77)


def plan_chunks(utts, max_cells, max_utts):
    """The chunk planner of csrc/alignplan.h restated (greedy, in order, an utterance never split) -> the utterance count of every chunk;
    tools/align_plan_check.cpp holds the planner itself to these invariants."""
    counts, cells = [], 0
    for x, c, _ in utts:
        n = len(x) * len(c)
        if counts and (cells + n > max_cells or counts[-1] >= max_utts):
            counts.append(0)
            cells = 0
        if not counts:
            counts.append(0)
        counts[-1] += 1
        cells += n
    return counts


def test_bit_identity_of_an_utterance(lib_path):
    """Utterance 1 of five (cells 100, 297, 33, 480, 175; sum T S = 1085): LL, gamma, durations and score are the same bits alone, first,
    last and in the middle of the batch, and with the limits forcing the batch [0, 2, 1, 3, 4] into 1, 2, 3 and 5 chunks: max_cells
    2^20 -> {0 2 1 3 4}; 700 -> {0 2 1} {3 4}; 480 -> {0 2 1} {3} {4}; max_utts 1 -> every utterance in a chunk of its own."""
    utts, model = five()
    me = utts[1]
    assert [len(x) * len(c) for x, c, _ in utts] == [100, 297, 33, 480, 175]
    results = []
    mid = [0, 2, 1, 3, 4]
    for max_cells, max_utts, order, chunks in ((1 << 20, 64, [1], [1]), (1 << 20, 64, [1, 0, 2, 3, 4], [5]), (1 << 20, 64, [0, 2, 3, 4, 1], [5]), (1 << 20, 64, mid, [5]),
                                               (700, 64, mid, [3, 2]), (480, 64, mid, [3, 1, 1]), (1 << 20, 1, mid, [1] * 5), (480, 1, [1, 0, 2, 3, 4], [1] * 5)):
        assert plan_chunks([utts[i] for i in order], max_cells, max_utts) == chunks
        d = Dev(lib_path, max_cells=max_cells, max_utts=max_utts, model=model)
        try:
            batch = [utts[i] for i in order]
            ll, gamma = d.posteriors(batch)
            dur, score = d.align(batch)
        finally:
            d.close()
        k = order.index(1)
        results.append((ll[k].tobytes(), gamma[k].tobytes(), dur[k].tobytes(), score[k].tobytes()))
        assert gamma[k].shape == (len(me[0]), len(me[1]))
    assert all(r == results[0] for r in results[1:])


def test_bit_identity_of_the_model(lib_path):
    """The model after one iteration: the same bits for the limits cutting one em_accumulate call into 1 chunk, 3 chunks ({0 1 2} {3} {4})
    and 5 chunks (max_utts = 1: every utterance in a chunk of its own, the fold running once per utterance against the running sums),
    and for the corpus in one em_accumulate call or in three (those cut again into 1 + 1 + 1, into 1 + 2 + 1 and into 1 + 3 + 1 chunks)."""
    utts, model = five()
    got = []
    three, other = [utts[:2], utts[2:3], utts[3:]], [utts[:1], utts[1:4], utts[4:]]
    for max_cells, max_utts, batches, chunks in ((1 << 20, 64, [utts], [[5]]), (480, 64, [utts], [[3, 1, 1]]), (1 << 20, 1, [utts], [[1] * 5]),
                                                 (1 << 20, 64, three, [[2], [1], [2]]), (600, 64, other, [[1], [2, 1], [1]]), (1 << 20, 1, other, [[1], [1] * 3, [1]])):
        assert [plan_chunks(b, max_cells, max_utts) for b in batches] == chunks
        d = Dev(lib_path, max_cells=max_cells, max_utts=max_utts, model=model)
        try:
            total, lls = d.em(batches)
            m = d.get_model()
        finally:
            d.close()
        got.append((m.mean.tobytes(), m.var.tobytes(), np.float64(total).tobytes(), lls.tobytes()))
    assert all(g == got[0] for g in got[1:])
    assert got[0][0] != model.mean.tobytes()


# ---- 4. EM ------------------------------------------------------------------------------------------------------------------------------
# Chosen on the CPU with the oracle alone: class means drawn N(0, 6^2) per coordinate against unit-variance frames (6 sigma, the
# separation the issue starts at), seed 3: the oracle's own fit puts 100 % of the frames in their true state (asserted >= 95 % below).
EM_SEED, EM_SEPARATION, EM_ITERS = 3, 6.0, 8


def em_data():
    if "em" not in _cache:
        utts, truth, _ = O.synthetic_corpus(EM_SEED, EM_SEPARATION)
        model = O.flat_start([u[0] for u in utts], 7)          # class 6 is absent from the corpus
        lls = []
        for _ in range(EM_ITERS):
            model, total, _ = O.em_iteration(model, utts)
            lls.append(total)
        durs = [O.align(x, model, c, o) for x, c, o in utts]
        _cache["em"] = (utts, truth, model, lls, durs)
    return _cache["em"]


def model_gates(start, utts):
    """(gate of mean, gate of var) for one iteration from `start` (module docstring)."""
    r0 = 3 * max(ll_gate(x, start, c, o) for x, c, o in utts)
    r = 2 * r0 + (max(len(u[0]) for u in utts) + max(len(u[1]) for u in utts) + len(utts) + 4) * U
    x1 = max(float(np.abs(u[0]).max()) for u in utts)
    return MARGIN * r * x1, MARGIN * 3 * r * x1 * x1


def test_em_precondition_on_the_oracle():
    """The data set is strong enough to show a wrong device: the oracle's own 8-iteration fit puts >= 95 % of the frames in their true
    state, its LL never decreases, and every decision of its final alignment has a margin above 1e-9."""
    utts, truth, model, lls, durs = em_data()
    assert 3 <= min(len(u[1]) for u in utts) and max(len(u[1]) for u in utts) <= 7 and 10 <= min(len(u[0]) for u in utts) and max(len(u[0]) for u in utts) <= 40
    assert any(u[2].any() for u in utts)
    hit = sum(int((np.repeat(np.arange(len(d[0])), d[0]) == t).sum()) for d, t in zip(durs, truth))
    frames = sum(len(t) for t in truth)
    show("oracle frame accuracy", hit / frames, "LL", lls)
    assert hit >= 0.95 * frames
    assert all(b >= a - 1e-9 * abs(a) for a, b in zip(lls, lls[1:]))
    assert min(d[2] for d in durs) > 1e-9


def test_em(lib_path):
    """After flat start (the oracle's, bit for bit) the total LL of each of 8 iterations is >= the previous one's - 1e-9 |LL|; after every
    iteration the device's model is within model_gates() of the oracle's iteration from the device's own previous model, and the total
    LL within the sum of the utterances' G; the absent class 6 keeps its flat-start parameters bit for bit; the final durations are the
    oracle's exactly.  Against drift that stays inside the one-step gate at every step, the final model is also compared with the
    oracle's OWN 8-iteration trajectory from the same flat start.  No rounding analysis bounds that (the EM map may amplify a
    difference from step to step), so the bound is a stated level, not a derived one: 1e-9 max|x| for the means and 1e-9 max x^2 for the
    variances — the relative level at which the issue calls a decision safe and an LL non-decreasing; the one-step gates are about
    1e-12 relative, which leaves the EM map three orders of amplification over 8 iterations, while a systematic error of the
    statistics (a dropped frame, a state folded twice) moves a mean by 1e-3 or more (measured there: emulator 8.7e-16 and 1.7e-16,
    MI355X 1.0e-15 and 1.1e-16).  Measured worst error / gate: emulator 0 (LL), 1.2e-7 (mean), 5.5e-8 (var); MI355X 4.5e-3 (LL), 5.2e-6 (mean), 6.9e-7 (var)."""
    utts, _, own, _, want_durs = em_data()
    d = Dev(lib_path, 8, 7)
    try:
        d.flat_start(utts)
        flat = d.get_model()
        ref = O.flat_start([u[0] for u in utts], 7)
        assert flat.mean.tobytes() == ref.mean.tobytes() and flat.var.tobytes() == ref.var.tobytes() and flat.gvar.tobytes() == ref.gvar.tobytes()
        prev, totals = flat, []
        for it in range(EM_ITERS):
            total, lls = d.em([utts[:5], utts[5:]])
            got = d.get_model()
            want, want_total, want_lls = O.em_iteration(prev, utts)
            gates = [ll_gate(x, prev, c, o) for x, c, o in utts]
            gm, gv = model_gates(prev, utts)
            show("iteration", it, "LL", total, "worst |LL err| / gate", max(abs(a - b) / g for a, b, g in zip(lls, want_lls, gates)),
                 "mean err / gate", np.abs(got.mean - want.mean).max() / gm, "var err / gate", np.abs(got.var - want.var).max() / gv)
            assert all(abs(a - b) <= g for a, b, g in zip(lls, want_lls, gates)) and abs(total - want_total) <= sum(gates)
            assert (np.abs(got.mean - want.mean) <= gm).all() and (np.abs(got.var - want.var) <= gv).all()
            assert got.mean[6].tobytes() == flat.mean[6].tobytes() and got.var[6].tobytes() == flat.var[6].tobytes()
            assert got.gvar.tobytes() == flat.gvar.tobytes()
            totals.append(total)
            prev = got
        assert all(b >= a - 1e-9 * abs(a) for a, b in zip(totals, totals[1:])), totals
        durs, _ = d.align(utts)
    finally:
        d.close()
    assert all(np.array_equal(a, b[0]) for a, b in zip(durs, want_durs))
    x1 = max(float(np.abs(u[0]).max()) for u in utts)
    show("final model against the oracle's own trajectory: mean", np.abs(prev.mean - own.mean).max() / x1, "var", np.abs(prev.var - own.var).max() / (x1 * x1), "bound 1e-9")
    assert np.abs(prev.mean - own.mean).max() <= 1e-9 * x1 and np.abs(prev.var - own.var).max() <= 1e-9 * x1 * x1


def test_em_one_class(lib_path):
    """V = 1: every state of every utterance is the one class, so the fold adds several states of one class per utterance (ascending s,
    from zero) and gamma is spread by exact ties.  One iteration from a random model within model_gates() of the oracle's, LL within G.  Measured error / gate, mean and var: emulator 2.8e-8 and 0,
    MI355X 7.1e-6 and 8.9e-7."""
    model = O.random_model(1, 8, 5)
    utts = [(O.random_features(T, 8, 900 + T), np.zeros(S, np.int32), opt) for T, S, opt in ((9, 4, np.asarray([0, 1, 0, 0], np.uint8)), (12, 3, np.zeros(3, np.uint8)),
                                                                                             (7, 1, np.zeros(1, np.uint8)))]
    d = Dev(lib_path, 8, 1, model=model)
    try:
        total, lls = d.em([utts])
        got = d.get_model()
    finally:
        d.close()
    want, want_total, want_lls = O.em_iteration(model, utts)
    gates = [ll_gate(x, model, c, o) for x, c, o in utts]
    gm, gv = model_gates(model, utts)
    show("one class: mean err / gate", np.abs(got.mean - want.mean).max() / gm, "var err / gate", np.abs(got.var - want.var).max() / gv)
    assert all(abs(a - b) <= g for a, b, g in zip(lls, want_lls, gates)) and abs(total - want_total) <= sum(gates)
    assert (np.abs(got.mean - want.mean) <= gm).all() and (np.abs(got.var - want.var) <= gv).all()
    assert got.mean.tobytes() != model.mean.tobytes()


def test_variance_floor_is_reached(lib_path):
    """A class whose frames are all the same vector: the oracle's fit has every coordinate of its variance on the floor var_floor g_f from
    the fourth iteration on (found on the CPU with the oracle alone); after five, oracle and device both hold the floor bit for bit."""
    r = np.random.default_rng(11)
    utts = []
    for k in range(4):
        state = np.repeat([0, 1, 0], [6 + k, 5, 7])
        x = np.where(state[:, None] == 1, np.asarray([4.0, -3.0]), r.standard_normal((len(state), 2)) - 4.0).astype(np.float32)
        utts.append((x, np.asarray([0, 1, 0], np.int32), np.zeros(3, np.uint8)))
    want = O.flat_start([u[0] for u in utts], 2)
    d = Dev(lib_path, 2, 2)
    try:
        d.flat_start(utts)
        for _ in range(5):
            d.em([utts])
            want = O.em_iteration(want, utts)[0]
        got = d.get_model()
    finally:
        d.close()
    floor = 0.01 * want.gvar
    assert want.var[1].tobytes() == floor.tobytes() and got.var[1].tobytes() == floor.tobytes()
    assert (got.var[0] > floor).all()


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(lib_path):
    """Every refusal names its argument, comes before any launch (the outputs stay untouched) and leaves the handle usable."""
    lib = _lib.load(lib_path)
    model = O.random_model(6, 8, 1)
    good = (O.random_features(10, 8, 1), np.asarray([0, 1, 2], np.int32), np.asarray([0, 1, 0], np.uint8))
    h = C.c_void_p()
    for args, text in (((0, 6, 320, 64, 1000, 4), "n_feat = 0 outside 1 .. 128"), ((8, 513, 320, 64, 1000, 4), "n_classes = 513 outside 1 .. 512"),
                       ((8, 6, 0, 64, 1000, 4), "max_frames = 0 outside"), ((8, 6, 320, 2049, 1000, 4), "max_states = 2049 outside 1 .. 2048"),
                       ((8, 6, 320, 64, 0, 4), "max_cells = 0 outside"), ((8, 6, 320, 64, 1000, 65536), "max_utts = 65536 outside")):
        assert lib.mtts_align_create(*args, 0, C.byref(h)) < 0 and text in lib.mtts_align_last_error(None).decode()
    assert lib.mtts_align_create(8, 6, 320, 64, 1000, 4, 0, None) < 0 and "NULL out" in lib.mtts_align_last_error(None).decode()
    assert lib.mtts_align_em_begin(None) < 0 and "NULL handle" in lib.mtts_align_last_error(None).decode()

    d = Dev(lib_path, 8, 6, max_frames=40, max_states=8, max_cells=200, max_utts=4)
    try:
        with pytest.raises(MttsError, match="no model loaded"):
            d.posteriors([good])
        with pytest.raises(MttsError, match="mtts_align_em_begin: no model loaded"):
            d.em([[good]])
        with pytest.raises(MttsError, match="mtts_align_get_model: no model loaded"):
            d.get_model()
        for field, value, text in (("var", 0.0, r"var holds a value that is not finite and > 0 \(class 2, feature 3\)"), ("var", np.inf, "var holds a value"),
                                   ("mean", np.nan, r"mean holds a non-finite value \(class 2, feature 3\)"), ("gvar", -1.0, r"global_var holds a value .*feature 3")):
            bad = model.copy()
            getattr(bad, field).reshape(-1, 8)[-1 if field == "gvar" else 2, 3] = value
            with pytest.raises(MttsError, match=text):
                d.set_model(bad)
        assert lib.mtts_align_set_model(d.h, None, None, None) < 0 and "NULL mean, var or global_var" in d.error()
        d.set_model(model)
        with pytest.raises(MttsError, match="mtts_align_em_accumulate: no iteration is open"):
            n, T, S, c, o, x = d.pack([good])
            d.check(lib.mtts_align_em_accumulate(d.h, n, _ptr(T), _ptr(S), _ptr(c), _ptr(o), _ptr(x), _ptr(np.empty(1))))
        total = C.c_double(-7.0)
        assert lib.mtts_align_em_finish(d.h, C.byref(total)) < 0 and "mtts_align_em_finish: no iteration is open" in d.error() and total.value == -7.0

        def utt(T=10, cls=(0, 1, 2), opt=(0, 1, 0), x=None):
            return (O.random_features(T, 8, 1) if x is None else x, np.asarray(cls, np.int32), np.asarray(opt, np.uint8))
        nan = O.random_features(10, 8, 1)
        nan[7, 2] = np.nan
        bad_calls = [(utt(T=41), "utterance 1: n_frames = 41 exceeds the handle's max_frames = 40"),
                     (utt(cls=range(6), opt=[0] * 6, T=34), r"utterance 1: 34 x 6 = 204 cells exceed the handle's max_cells = 200"),
                     (utt(T=20, cls=[0] * 9, opt=[0] * 9), "utterance 1: n_states = 9 exceeds the handle's max_states = 8"),
                     (utt(T=2, cls=(0, 1, 2, 3), opt=(0, 1, 0, 0)), "utterance 1: 3 mandatory states exceed n_frames = 2"),
                     (utt(cls=(0, 1, 2, 3), opt=(0, 1, 1, 0)), "utterance 1: states 1 and 2 are adjacent optional states"),
                     (utt(cls=(0, 6, 2)), r"utterance 1: state 1: class 6 outside 0 .. n_classes - 1 = 5"),
                     (utt(cls=(0, -1, 2)), "utterance 1: state 1: class -1 outside"),
                     (utt(x=nan), r"x holds a non-finite value \(row 17\)")]
        for bad, text in bad_calls:
            for call in (d.posteriors, d.align):
                with pytest.raises(MttsError, match=text):
                    call([good, bad])
            d.check(lib.mtts_align_em_begin(d.h))
            with pytest.raises(MttsError, match=text):
                n, T, S, c, o, x = d.pack([good, bad])
                ll = np.full(2, -7.0)
                rc = lib.mtts_align_em_accumulate(d.h, n, _ptr(T), _ptr(S), _ptr(c), _ptr(o), _ptr(x), _ptr(ll))
                assert (ll == -7.0).all()
                d.check(rc)
        n, T, S, c, o, x = d.pack([good])
        ll, g, dur = np.empty(1), np.empty(30), np.empty(3, np.int32)
        for args in ((None, S, c, o, x), (T, None, c, o, x), (T, S, None, o, x), (T, S, c, None, x), (T, S, c, o, None)):
            assert lib.mtts_align_posteriors(d.h, 1, *[_ptr(a) for a in args], _ptr(ll), _ptr(g)) < 0 and "NULL n_frames, n_states, classes, optional or x" in d.error()
        assert lib.mtts_align_posteriors(d.h, 1, _ptr(T), _ptr(S), _ptr(c), _ptr(o), _ptr(x), None, _ptr(g)) < 0 and "NULL ll_out" in d.error()
        assert lib.mtts_align_posteriors(d.h, 1, _ptr(T), _ptr(S), _ptr(c), _ptr(o), _ptr(x), _ptr(ll), None) < 0 and "NULL gamma_out" in d.error()
        assert lib.mtts_align_align(d.h, 1, _ptr(T), _ptr(S), _ptr(c), _ptr(o), _ptr(x), None, _ptr(ll)) < 0 and "NULL durations_out or score_out" in d.error()
        assert lib.mtts_align_posteriors(d.h, 0, _ptr(T), _ptr(S), _ptr(c), _ptr(o), _ptr(x), _ptr(ll), _ptr(g)) < 0 and "n_utts = 0" in d.error()
        assert lib.mtts_align_flat_start(d.h, 1, _ptr(T), None) < 0 and "NULL n_frames or x" in d.error()
        const = np.ones((10, 8), np.float32)
        assert lib.mtts_align_flat_start(d.h, 1, _ptr(T), _ptr(const)) < 0 and "feature 0 is constant" in d.error()
        assert lib.mtts_align_set_floor(d.h, 0.0, 1e-3) < 0 and "var_floor" in d.error()
        assert lib.mtts_align_em_begin(d.h) == 0 and lib.mtts_align_em_finish(d.h, None) < 0 and "NULL total_ll_out" in d.error()
        # the handle still works, and the refused calls changed nothing: the same posteriors as a fresh handle's
        ll, gamma = d.posteriors([good])
        fresh = Dev(lib_path, 8, 6, model=model)
        ll2, gamma2 = fresh.posteriors([good])
        fresh.close()
        assert ll.tobytes() == ll2.tobytes() and gamma[0].tobytes() == gamma2[0].tobytes()
    finally:
        d.close()


# ---- 6. the host layer --------------------------------------------------------------------------------------------------------------------
class _Rates:
    """What Preprocessor.get_alignment reads of its instance."""

    def __init__(self, sampling_rate, hop_length):
        self.sampling_rate, self.hop_length = sampling_rate, hop_length


@pytest.mark.parametrize("rate,hop", [(22050, 256), (16000, 160)])
def test_textgrid_round_trip(tmp_path, rate, hop):
    """write_textgrid -> read_textgrid -> get_alignment gives the durations back exactly (zero-length intervals left out), for random
    durations up to 3000 frames into the file and for every boundary 0 .. 2000."""
    from meta_tts_amd import preprocessor as P
    r = np.random.default_rng(rate)
    seqs = [(["AH"] * 2001, [1] * 2001)]
    for _ in range(20):
        n = int(r.integers(1, 40))
        seqs.append(([f"P{k}" for k in range(n)], [int(v) for v in r.integers(0, 80, n)]))
        seqs[-1][1][0] = max(1, seqs[-1][1][0])
    seqs.append((["A", "sp", "B", 'q"uote'], [3, 0, 5, 2]))
    for k, (phones, durs) in enumerate(seqs):
        path = str(tmp_path / f"{k}.TextGrid")
        A.write_textgrid(path, phones, durs, hop, rate)
        got_p, got_d, start, end = P.Preprocessor.get_alignment(_Rates(rate, hop), P.read_textgrid(path).get_tier_by_name("phones"))
        assert got_p == [p for p, d in zip(phones, durs) if d > 0] and got_d == [d for d in durs if d > 0]
        assert start == 0.0 and round(end * rate / hop) == sum(durs)


def test_state_dict_continues_bit_identically(lib_path):
    utts, _, _, _, _ = em_data()
    names = [f"p{k}" for k in range(7)]
    feats, seqs = [u[0] for u in utts], [[names[c] for c in u[1]] for u in utts]
    kw = dict(n_feat=8, optional=("p0",), max_frames=64, max_states=16, lib_path=lib_path)
    a = A.MonophoneAligner(names, **kw)
    b = A.MonophoneAligner(names, **kw)
    try:
        first = a.fit(feats, seqs, n_iter=2, batch_utterances=5)
        state = a.state_dict()
        rest = a.fit(feats, seqs, n_iter=2, batch_utterances=5, flat_start=False)
        b.load_state_dict({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in state.items()})
        again = b.fit(feats, seqs, n_iter=2, batch_utterances=7, flat_start=False)
        assert rest == again and first[1] >= first[0] - 1e-9 * abs(first[0])
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a.get_model(), b.get_model()))
        da, db = a.align(feats, seqs), b.align(feats, seqs)
        assert all(np.array_equal(x, y) and x.sum() == len(f) for x, y, f in zip(da, db, feats))
        ll, gamma = a.posteriors(feats[:2], seqs[:2])
        assert gamma[0].shape == (len(feats[0]), len(seqs[0])) and np.abs(gamma[1].sum(axis=1) - 1).max() < 1e-9
        with pytest.raises(ValueError, match="not in the phone set"):
            a.align(feats[:1], [["nope"]])
    finally:
        a.close()
        b.close()


def test_align_corpus_feeds_build_from_path(lib_path, tmp_path):
    """A raw tree without TextGrids: build_from_path emits nothing; after align_corpus it emits every utterance, with the aligner's
    durations, and the durations are within 2 frames of the tones' true boundaries (tones are far easier than speech: this is a check of
    the plumbing, not of alignment quality)."""
    from meta_tts_amd import preprocessor as P
    cfg = align_tree.write_raw(str(tmp_path))
    pp = P.Preprocessor(cfg, max_samples=align_tree.SAMPLING_RATE * 2, lib_path=lib_path)
    try:
        f0_fn = lambda wav, sr, hop: np.full(len(wav) // hop + 1, 120.0)   # noqa: E731
        assert pp.build_from_path(f0_fn=f0_fn)["train"] == []
        durs = A.align_corpus(pp, align_tree.phones, n_iter=4, batch_utterances=3, lib_path=lib_path)
        assert sorted(durs) == sorted(align_tree.UTTERANCES)
        lines = pp.build_from_path(f0_fn=f0_fn)["train"]
        assert [ln.split("|")[0] for ln in lines] == [b for _, b in sorted(align_tree.UTTERANCES)]
        for (spk, base), segs in align_tree.UTTERANCES.items():
            d = durs[(spk, base)]
            assert os.path.exists(os.path.join(pp.out_dir, "TextGrid", spk, base + ".TextGrid"))
            on_disk = np.load(os.path.join(pp.out_dir, "duration", f"{spk}-duration-{base}.npy"))
            assert np.array_equal(on_disk, d[d > 0]) and d.sum() == sum(n for _, n in segs)
            assert np.abs(np.cumsum(d) - np.cumsum([n for _, n in segs])).max() <= 2, (base, d, segs)
    finally:
        pp.close()


# ---- 7. the host plan under the sanitizers ----------------------------------------------------------------------------------------------
def test_plan_check_under_sanitizers(tmp_path):
    """tools/align_plan_check.cpp (limits, validation and chunk planner of csrc/alignplan.h, with buffers of exactly the size the
    arguments describe) built with ASan + UBSan as a stand-alone program and run on the CPU: "ok", exit status 0, nothing on stderr."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = ge.HOST_CLANG if os.path.exists(ge.HOST_CLANG) else "clang++"
    exe = str(tmp_path / "align_plan_check")
    subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(root, "meta_tts_amd", "csrc"),
                    os.path.join(root, "tools", "align_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok" and r.stderr == "", (r.returncode, r.stdout, r.stderr)
