"""Constrained decoding without a GPU: bmhrl_amd.decode._apply_rules against the numpy restatement of
tests/constrain_reference.py (bit-equal), and the three re-run paths (greedy_decode, beam_decode, sample_decode on CPU tensors)
on a model that loops and stops early by construction."""
import numpy as np
import pytest
import torch

from bmhrl_amd.decode import _apply_rules, beam_decode, beam_decoder, greedy_decode, sample_decode, sample_decoder
from tests import constrain_reference as ref
from tests.test_beam_cpu import END, PAD, START, _features

AV = "audio_video"
V7, END7 = 7, 6


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def test_apply_rules_is_bit_equal_to_the_restatement():
    g = torch.Generator().manual_seed(3)
    cases = ref.case_table()
    kinds = set()
    for name, hist, t, n, m, theta in cases:
        lp = torch.log_softmax(torch.randn(hist.shape[0], V7, generator=g) * 2, -1)
        lp[0, 5] = float("-inf")                                # an entry that is -inf already
        want = ref.apply_rules(lp.numpy(), hist, t, n, m, theta, END7, PAD)
        before = lp.clone()
        got = _apply_rules(lp, torch.from_numpy(hist).long(), t, n, m, float(np.float32(theta)), END7, PAD)
        assert torch.equal(lp, before), name                     # the input is left alone
        assert got.dtype == torch.float32 and np.array_equal(_bits(got.numpy()), _bits(want)), name
        if n >= 1:
            kinds.add("short" if t + 1 < n else "exact" if t + 1 == n else "long")
            if t + 1 < n and theta == 1.0 and m == 0:
                assert torch.equal(got, before), name            # nothing is banned before the first full n-gram
        if theta != 1.0:
            s = hist[:, :t + 1]
            for r in range(s.shape[0]):
                for v in set(s[r].tolist()):
                    if v != PAD and np.isfinite(want[r, v]):     # one multiply however often the id occurs
                        assert want[r, v] == np.float32(before[r, v].item()) * np.float32(theta), name
                if PAD in s[r].tolist() and np.isfinite(want[r, PAD]):
                    assert want[r, PAD] == before[r, PAD].item(), name
    assert kinds == {"short", "exact", "long"}
    # the cases mean what they say: a repeated bigram with two followers bans both; m bans the end at t = m - 1 only
    h = np.array([[2, 3, 4, 5, 3, 4, 0, 3, 4, 3, 4, 6]])
    lp = np.full((1, V7), -1.0, dtype=np.float32)
    out = ref.apply_rules(lp, h, 10, 3, 0, 1.0, END7, PAD)       # last two: (3, 4); followers so far: 5, 0, 3
    assert sorted(np.flatnonzero(np.isinf(out[0])).tolist()) == [0, 3, 5]
    assert np.isinf(ref.apply_rules(lp, h, 4, 0, 5, 1.0, END7, PAD)[0, END7])
    assert not np.isinf(ref.apply_rules(lp, h, 5, 0, 5, 1.0, END7, PAD)).any()
    out = ref.apply_rules(lp, h, 3, 1, 0, 1.0, END7, PAD)        # n = 1: every token of the sequence
    assert sorted(np.flatnonzero(np.isinf(out[0])).tolist()) == [2, 3, 4, 5]


# ------------------------------------------------------------------------------------------------------- re-run paths
class LoopModel:
    """inference(x, trg, masks) -> (rows, L, V) log-probs that depend on the sample and the last token only.  Sample 0 walks
    the cycle 4 -> 5 -> 4 -> ... for ever, sample 1 goes START -> 6 -> END; everywhere END is the runner-up, and a little
    fixed noise separates the rest.  The sample id is rgb[:, 0, 0], as in tests/test_beam_cpu.py's TableModel."""
    training = False

    def __init__(self, V=8, seed=0):
        g = torch.Generator().manual_seed(seed)
        logits = torch.randn(2, V, V, generator=g) * 0.3
        logits[:, :, END] += 2.0
        for prev, nxt in ((START, 4), (4, 5), (5, 4)):
            logits[0, prev, nxt] += 4.0
        for prev, nxt in ((START, 6), (6, END), (4, 5), (5, 4)):
            logits[1, prev, nxt] += 4.0
        self.table = torch.log_softmax(logits, -1)

    def inference(self, x, trg, masks):
        sid = x[0][0][:, 0, 0].long() - 1
        return self.table[sid.unsqueeze(1), trg]


B, V, L = 2, 8, 10
RULES = dict(no_repeat_ngram=2, min_len=5, repetition_penalty=1.2)


def _hyps(toks):
    """(…, n + 1) tokens -> the list of hypotheses up to their ends"""
    return [ref.upto_end(r, END) for r in toks.reshape(-1, toks.shape[-1]).tolist()]


def _loops_and_stops_early(hyps, n, m):
    """the precondition: some hypothesis repeats an n-gram before its end, some ends before m tokens were generated"""
    return any(ref.repeats_ngram(h, n) for h in hyps), any(h[-1] == END and len(h) - 1 <= m for h in hyps)


def _check_structure(hyps, n, m):
    for h in hyps:
        assert not ref.repeats_ngram(h, n), h
        assert h[-1] != END or len(h) - 1 >= m + 1, h             # the end token is the (m + 1)-th generated one at the earliest


def _greedy_by_hand(model, n, m, theta):
    trg = np.full((B, 1), START, dtype=np.int64)
    done = np.zeros(B, dtype=bool)
    while trg.shape[1] <= L and not done.all():
        lp = model.table[torch.arange(B), torch.from_numpy(trg[:, -1])].numpy()
        lp = ref.apply_rules(lp, trg, trg.shape[1] - 1, n, m, theta, END, PAD)
        nxt = lp.argmax(1)
        trg = np.concatenate([trg, nxt[:, None]], 1)
        done |= nxt == END
    return torch.from_numpy(trg)


def test_greedy_rerun_under_rules():
    model, fs = LoopModel(), _features(B)
    free = greedy_decode(model, fs, L, START, END, PAD, AV)
    assert _loops_and_stops_early(_hyps(free), 2, 5) == (True, True), free
    got, first = greedy_decode(model, fs, L, START, END, PAD, AV, return_first=True, **RULES)
    _check_structure(_hyps(got), 2, 5)
    assert torch.equal(got, _greedy_by_hand(model, 2, 5, 1.2))
    # the first step's log-probs are the adjusted ones: the start token penalised, the end banned
    want = ref.apply_rules(model.table[:, START].numpy(), np.full((B, 1), START), 0, 2, 5, 1.2, END, PAD)
    assert np.array_equal(_bits(first.numpy()), _bits(want))
    for kw in (dict(no_repeat_ngram=3), dict(min_len=L), dict(repetition_penalty=0.7), dict(no_repeat_ngram=1, min_len=2)):
        n, m, theta = kw.get("no_repeat_ngram", 0), kw.get("min_len", 0), kw.get("repetition_penalty", 1.0)
        assert torch.equal(greedy_decode(model, fs, L, START, END, PAD, AV, **kw), _greedy_by_hand(model, n, m, theta)), kw
    from bmhrl_amd.decode import greedy_decoder
    assert torch.equal(greedy_decoder(**RULES)(model, fs, L, START, END, PAD, AV), got)
    assert torch.equal(greedy_decoder()(model, fs, L, START, END, PAD, AV), free)


def test_beam_rerun_under_rules():
    model, fs, K = LoopModel(), _features(B), 3
    free = beam_decode(model, fs, L, START, END, PAD, AV, beam_size=K, return_beams=True)
    assert _loops_and_stops_early(_hyps(free[1]), 2, 5) == (True, True), free[1]
    toks, beams, scores = beam_decode(model, fs, L, START, END, PAD, AV, beam_size=K, return_beams=True, **RULES)
    assert beams.shape[:2] == (B, K) and bool(torch.isfinite(scores).all())
    _check_structure(_hyps(beams), 2, 5)
    _check_structure(_hyps(toks), 2, 5)
    # a beam's score is the sum of the adjusted log-probs of its own tokens
    for b in range(B):
        for k in range(K):
            h = ref.upto_end(beams[b, k].tolist(), END)
            s = torch.zeros((), dtype=torch.float32)
            for t in range(len(h) - 1):
                lp = ref.apply_rules(model.table[b, h[t]].numpy()[None], np.array([h]), t, 2, 5, 1.2, END, PAD)[0]
                s = s + torch.tensor(lp[h[t + 1]])
            assert torch.equal(s, scores[b, k]), (b, k)
    assert torch.equal(beam_decoder(K, **RULES)(model, fs, L, START, END, PAD, AV), toks)
    one = beam_decode(model, fs, L, START, END, PAD, AV, beam_size=1, **RULES)
    greedy = greedy_decode(model, fs, L, START, END, PAD, AV, **RULES)
    for b in range(B):                                            # K = 1 is greedy, padded after the end
        h = ref.upto_end(greedy[b].tolist(), END)
        assert one[b, :len(h)].tolist() == h and bool((one[b, len(h):] == PAD).all())


def test_sample_rerun_under_rules():
    model, fs, n = LoopModel(), _features(B), 3
    seed = 5                                                      # the free draws of this seed loop and stop early
    free = sample_decode(model, fs, L, START, END, PAD, AV, n=n, seed=seed, return_samples=True)
    assert _loops_and_stops_early(_hyps(free[1]), 2, 5) == (True, True), free[1]
    toks, samples, sums, slp, slq = sample_decode(model, fs, L, START, END, PAD, AV, n=n, seed=seed, return_samples=True,
                                                  **RULES)
    assert samples.shape[:2] == (B, n)
    _check_structure(_hyps(samples), 2, 5)
    _check_structure(_hyps(toks), 2, 5)
    # the recorded model log-probs are the adjusted ones
    for b in range(B):
        for i in range(n):
            h = ref.upto_end(samples[b, i].tolist(), END)
            for t in range(len(h) - 1):
                lp = ref.apply_rules(model.table[b, h[t]].numpy()[None], np.array([h]), t, 2, 5, 1.2, END, PAD)[0]
                assert float(slp[b, i, t]) == float(lp[h[t + 1]]) and np.isfinite(lp[h[t + 1]]), (b, i, t)
    assert bool((slq <= 1e-6).all()) and torch.allclose(sums, slp.sum(-1), atol=1e-5)
    assert torch.equal(sample_decoder(n, seed=seed, **RULES)(model, fs, L, START, END, PAD, AV), toks)
    arg = sample_decode(model, fs, L, START, END, PAD, AV, n=1, temperature=0.0, seed=1, **RULES)
    greedy = greedy_decode(model, fs, L, START, END, PAD, AV, **RULES)
    for b in range(B):                                            # T = 0 is greedy, padded after the end
        h = ref.upto_end(greedy[b].tolist(), END)
        assert arg[b, :len(h)].tolist() == h and bool((arg[b, len(h):] == PAD).all())


def test_default_rules_change_nothing():
    model, fs = LoopModel(), _features(B)
    off = dict(no_repeat_ngram=0, min_len=0, repetition_penalty=1.0)
    a = greedy_decode(model, fs, L, START, END, PAD, AV, return_first=True)
    b = greedy_decode(model, fs, L, START, END, PAD, AV, return_first=True, **off)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    a = beam_decode(model, fs, L, START, END, PAD, AV, beam_size=3, return_scores=True, return_beams=True)
    b = beam_decode(model, fs, L, START, END, PAD, AV, beam_size=3, return_scores=True, return_beams=True, **off)
    assert len(a) == len(b) == 4 and all(torch.equal(x, y) for x, y in zip(a, b))
    a = sample_decode(model, fs, L, START, END, PAD, AV, n=3, seed=2, top_p=0.9, return_samples=True)
    b = sample_decode(model, fs, L, START, END, PAD, AV, n=3, seed=2, top_p=0.9, return_samples=True, **off)
    assert len(a) == len(b) == 5 and all(torch.equal(x, y) for x, y in zip(a, b))


def test_invalid_rules_are_refused():
    from bmhrl_amd.decode import greedy_decoder
    model, fs = LoopModel(), _features(B)
    bad = (dict(no_repeat_ngram=-1), dict(min_len=-1), dict(repetition_penalty=0.0), dict(repetition_penalty=-1.5),
           dict(repetition_penalty=float("inf")), dict(repetition_penalty=float("nan")),
           dict(no_repeat_ngram=2.5), dict(min_len=1.5), dict(no_repeat_ngram=float("nan")), dict(min_len=float("inf")))
    for kw in bad + (dict(min_len=L + 1),):
        for fn in (greedy_decode, beam_decode, sample_decode):
            with pytest.raises(ValueError):
                fn(model, fs, L, START, END, PAD, AV, **kw)
    for kw in bad:
        for factory in (greedy_decoder, beam_decoder, sample_decoder):
            with pytest.raises(ValueError):
                factory(**kw)
    greedy_decode(model, fs, L, START, END, PAD, AV, min_len=L)                     # m = max_len is allowed


def test_greedy_decoder_is_not_exported_to_the_reference_loops():
    """the reference has a greedy_decoder with another signature: the factory lives in bmhrl_amd.decode only"""
    from bmhrl_amd import decode
    from bmhrl_amd.epoch_loops import captioning_bmrl_loops as loops
    assert callable(decode.greedy_decoder) and not hasattr(loops, "greedy_decoder")
    assert loops.beam_decoder is decode.beam_decoder and loops.sample_decoder is decode.sample_decoder


def test_ids_outside_the_vocabulary_select_no_entry():
    """a history id outside [0, V) takes part in rule 2's comparisons but selects no entry (as in the kernel): the result is the
    restatement's over the same history with every such id replaced by one in-range id that occurs nowhere else, whose own
    entry is left alone"""
    V = 9
    lp = torch.log_softmax(torch.randn(2, V, generator=torch.Generator().manual_seed(3)), -1)
    hist = np.array([[2, 3, 40, 3, 40, 5, 3, 40], [2, -7, 4, -7, 4, 4, -7, 4]])
    spare = 8
    stand_in = np.where((hist < 0) | (hist >= V), spare, hist)
    for t in (3, 6, 7):
        for n, theta in ((2, 1.3), (3, 0.7), (1, 1.0), (0, 1.3)):
            got = _apply_rules(lp.clone(), torch.from_numpy(hist), t, n, 0, np.float32(theta).item(), END, PAD)
            want = ref.apply_rules(lp.numpy(), stand_in, t, n, 0, theta, END, PAD)
            want[:, spare] = lp.numpy()[:, spare]
            assert np.array_equal(_bits(got.numpy()), _bits(want)), (t, n, theta)


def test_history_capacity_matches_the_header():
    """ops.LOGIT_RULES_MAX_HIST is the header's BMHRL_LOGIT_RULES_MAX_HIST, which the library is compiled with"""
    import os
    import re
    from bmhrl_amd import ops
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bmhrl_hip.h")
    with open(header) as f:
        found = re.findall(r"^#define\s+BMHRL_LOGIT_RULES_MAX_HIST\s+(\d+)\s*$", f.read(), re.M)
    assert found == [str(ops.LOGIT_RULES_MAX_HIST)]
