"""SODA_c on the host: the restatement's double loop against a brute-force enumeration of every
order-preserving matching, bit for bit; what the shared random cases cover; the hand examples; the host half of
bmhrl_amd/evaluate.py (soda_groups, the choice of the best file, the means, the keywords) with the device half replaced by
the restatement.  No GPU."""
import numpy as np
import pytest

from tests import soda_reference as sr

HEAD = {"version": "VERSION 1.0", "external_data": {"used": True, "details": ""}}


@pytest.fixture(scope="module")
def solved():
    """per case: {threshold: (cost matrix, dp, (brute-force sum, matching))} at the first two thresholds"""
    out = []
    for preds, refs, S in sr.random_cases():
        per_t = {}
        for t in sr.CASE_TIOUS[:2]:
            c = sr.cost_matrix(preds, refs, S, t)
            per_t[t] = (c, sr.dp(c), sr.brute_force(c))
        out.append(per_t)
    return out


def test_double_loop_equals_the_enumeration_bit_for_bit(solved):
    assert len(solved) == sr.CASE_COUNT
    for per_t in solved:
        for c, got, (want, _) in per_t.values():
            assert len(c) <= 7 and len(c[0]) <= 5
            assert np.float64(got).tobytes() == np.float64(want).tobytes()
    zeros = cells = not_greedy = 0
    for c in sr.random_matrices():                       # matrices of their own: about 40 % zeros, no threshold
        got = sr.dp(c)
        assert np.float64(got).tobytes() == np.float64(sr.brute_force(c)[0]).tobytes()
        cells += len(c) * len(c[0])
        zeros += sum(v == 0.0 for row in c for v in row)
        not_greedy += got != sr.best_reference_each(c)
    assert 0.35 < zeros / cells < 0.45 and not_greedy * 4 >= sr.CASE_COUNT


def test_what_the_random_cases_cover(solved):
    t0, t1 = sr.CASE_TIOUS[:2]
    zeros = cells = 0
    not_greedy = changes = all_zero = 0
    for per_t in solved:
        c, got, (_, m0) = per_t[t0]
        _, _, (_, m1) = per_t[t1]
        cells += len(c) * len(c[0])
        zeros += sum(v == 0.0 for row in c for v in row)
        not_greedy += got != sr.best_reference_each(c)
        changes += bool(m0) and bool(m1) and [p for p in m0 if p in m1] != m0 and [p for p in m1 if p in m0] != m1
        if not any(v for row in c for v in row):
            all_zero += 1
            assert got == 0.0
    print(not_greedy, changes, all_zero, zeros / cells)
    assert not_greedy * 4 >= len(solved)                 # the order and the one-to-one rule decide in a quarter at least
    assert changes >= 1                                  # a matching that is rearranged, not only cut, by the threshold
    assert all_zero >= 1
    preds, refs, S = sr.random_cases()[13]
    assert not np.any(S) and sr.group_scores(preds, refs, S, sr.CASE_TIOUS) == [[0.0] * 4] * 4
    S_all = [v for _, _, S in sr.random_cases() for row in S for v in row]
    assert 0.3 < sum(v == 0.0 for v in S_all) / len(S_all) < 0.5


def test_hand_examples_of_the_double_loop():
    # the diagonal: both pairs count
    rows = sr.group_scores(sr.HAND_PRED, sr.HAND_REF, sr.HAND_S, [0.5])
    one = 10.0 / (10.0 + 1e-8)
    assert rows[0][0] == one * 0.5 + one * 0.25 and rows[0][1] == rows[0][0] / 2 == rows[0][2] == rows[0][3]
    # the large scores on the anti-diagonal: the order allows one of them, the larger -- not their sum
    c = sr.cost_matrix(sr.HAND_ANTI_PRED, sr.HAND_ANTI_REF, sr.HAND_ANTI_S, 0.3)
    big = 12.0 / (12.0 + 1e-8)
    assert c == [[0.0, big * 0.75], [big * 0.5, 0.0]]
    assert sr.dp(c) == big * 0.75 == sr.brute_force(c)[0]
    print(repr(sr.group_scores(sr.HAND_ANTI_PRED, sr.HAND_ANTI_REF, sr.HAND_ANTI_S, [0.0, 0.3])))
    # below the threshold 0.2 the diagonal's cells (tIoU 4 / 20) come back, and still lose
    c0 = sr.cost_matrix(sr.HAND_ANTI_PRED, sr.HAND_ANTI_REF, sr.HAND_ANTI_S, 0.0)
    assert c0[0][0] == 4.0 / (20.0 + 1e-8) * 0.25 and sr.dp(c0) == big * 0.75
    assert sr.group_scores(sr.HAND_ANTI_PRED, sr.HAND_ANTI_REF, sr.HAND_ANTI_S, [0.3]) == \
        [[0.749999999375, 0.3749999996875, 0.3749999996875, 0.3749999996875]]
    assert sr.prf(0.0, 3, 2) == [0.0, 0.0, 0.0, 0.0] and sr.prf(1.0, 0, 2) == [0.0] * 4 and sr.prf(1.0, 2, 0) == [0.0] * 4
    assert sr.prf(1.0, 2, 4) == [1.0, 0.5, 0.25, 2 * 0.5 * 0.25 / 0.75]


# ---- the host half of bmhrl_amd/evaluate.py, the device half replaced by the restatement
def host_scores(groups, tious, tables, device, tokenizer):
    out = np.zeros((len(groups), len(tious), 4))
    for k, g in enumerate(groups):
        S = sr.meteor_matrix([tokenizer(s) for s in g.pred_sentences], [tokenizer(s) for s in g.ref_sentences])
        out[k] = sr.group_scores(g.pred_segments, g.ref_segments, S, tious)
    return out


def evaluator(monkeypatch, gts, results, tious=(0.3, 0.5), max_proposals=1000, **kw):
    from bmhrl_amd import evaluate as E
    monkeypatch.setattr(E, "soda_scores", host_scores)
    monkeypatch.setattr(E, "score_pairs", lambda hyps, refs, off, device, tables:
                        {m: np.zeros(len(off) - 1) for m in E.METRICS})
    kw.setdefault("soda", True)
    ev = E.DenseCaptionEvaluator(gts, dict(HEAD, results=results), list(tious), max_proposals, device="cpu", stemmer=False,
                                 synonyms=False, **kw)
    ev.evaluate()
    want = sr.evaluate(gts, dict(HEAD, results=results), list(tious), max_proposals, E.tokenize,
                       sort_references=kw.get("sort_references", False))
    return ev, want


def seg(a, b, s):
    return {"timestamp": [a, b], "sentence": s}


GT_A = {"v1": {"duration": 20.0, "timestamps": [[0, 10], [10, 20]], "sentences": ["A dog runs.", "The cat sits."]},
        "v2": {"duration": 20.0, "timestamps": [[0, 20]], "sentences": ["A man plays the guitar."]}}


def test_ties_keep_submission_order(monkeypatch):
    gt = {"v": {"duration": 10.0, "timestamps": [[0, 10], [0, 10]], "sentences": ["A dog runs.", "The cat sits."]}}
    ev, want = evaluator(monkeypatch, [gt], {"v": [seg(0, 10, "a dog runs"), seg(0, 10, "the cat sits")]}, tious=[0.5])
    assert ev.scores["SODA_c"] == want[0]["SODA_c"] and ev.soda_per_video == want[1]
    sentence = 1.0 - 0.5 * (1.0 / 3.0) ** 3                            # METEOR of a three-word sentence against itself
    assert ev.soda_per_video["v"][0][2] == pytest.approx(sentence * 10.0 / (10.0 + 1e-8), rel=1e-12)
    ev2, _ = evaluator(monkeypatch, [gt], {"v": [seg(0, 10, "the cat sits"), seg(0, 10, "a dog runs")]}, tious=[0.5])
    assert ev2.soda_per_video["v"][0][2] == pytest.approx(0.5 * ev.soda_per_video["v"][0][2], rel=1e-12)


def test_prediction_only_videos_are_ignored_and_videos_without_predictions_score_zero(monkeypatch):
    results = {"v1": [seg(0, 10, "a dog runs"), seg(10, 20, "the cat sits")], "only_predicted": [seg(0, 5, "a dog")]}
    ev, want = evaluator(monkeypatch, [GT_A], results)
    assert sorted(ev.soda_per_video) == ["v1", "v2"] and ev.soda_per_video == want[1]
    assert ev.soda_per_video["v2"] == [(0.0, 0.0, 0.0)] * 2 and ev.soda_per_video["v1"][0][2] > 0.9
    for m in sr.METRICS:
        assert ev.scores[m] == want[0][m]
    assert ev.scores["SODA_c"][0] == ev.soda_per_video["v1"][0][2] / 2
    ev3, _ = evaluator(monkeypatch, [GT_A], {"v1": [], "v2": [seg(0, 20, "a man plays the guitar")]})
    assert ev3.soda_per_video["v1"] == [(0.0, 0.0, 0.0)] * 2 and ev3.soda_per_video["v2"][0][2] > 0.9


def test_two_files_take_the_first_best_file(monkeypatch):
    from bmhrl_amd import evaluate as E
    gt_b = {"v1": {"duration": 20.0, "timestamps": [[0, 10]], "sentences": ["A dog runs."]},
            "v3": {"duration": 5.0, "timestamps": [], "sentences": []}}
    results = {"v1": [seg(0, 10, "a dog runs"), seg(10, 20, "the cat sits")]}
    ev, want = evaluator(monkeypatch, [GT_A, gt_b], results, tious=[0.5])
    assert ev.soda_per_video == want[1] and sorted(ev.soda_per_video) == ["v1", "v2", "v3"]
    groups, by_video = E.soda_groups(ev.ground_truths, ev.prediction)
    assert by_video == {"v1": [0, 1], "v2": [], "v3": []} and [g.file for g in groups] == [0, 1]
    per_group = host_scores(groups, [0.5], None, None, E.tokenize)
    assert per_group[0, 0, 3] > per_group[1, 0, 3] > 0                  # file A: both matched; file B: recall 1, precision 1/2
    assert ev.soda_per_video["v1"][0] == tuple(per_group[0, 0, 1:])
    # equal F in both files: the first file's triple, also when the files come the other way round
    same = [GT_A, {"v1": GT_A["v1"]}]
    ev2, want2 = evaluator(monkeypatch, same, results, tious=[0.5])
    assert ev2.soda_per_video == want2[1] and ev2.soda_per_video["v1"] == ev.soda_per_video["v1"]
    triples = E.soda_per_video({"v": [0, 1]}, np.array([[[9, 0.2, 0.4, 0.5]], [[9, 0.4, 0.2, 0.5]]]), 1)
    assert triples == {"v": [(0.2, 0.4, 0.5)]}
    assert E.soda_means({"a": [(0.2, 0.4, 0.5)], "b": [(0.0, 0.0, 0.0)]}, 1) == \
        {"SODA_c": [0.25], "SODA_c_Precision": [0.1], "SODA_c_Recall": [0.2]}


def test_sort_references_changes_a_case_built_for_it(monkeypatch):
    gt = {"v": {"duration": 20.0, "timestamps": [[10, 20], [0, 10]], "sentences": ["The cat sits.", "A dog runs."]}}
    results = {"v": [seg(0, 10, "a dog runs"), seg(10, 20, "the cat sits")]}
    story, want = evaluator(monkeypatch, [gt], results, tious=[0.5])
    by_time, want_t = evaluator(monkeypatch, [gt], results, tious=[0.5], sort_references=True)
    assert story.soda_per_video == want[1] and by_time.soda_per_video == want_t[1]
    assert by_time.scores["SODA_c"][0] == pytest.approx(2 * story.scores["SODA_c"][0], rel=1e-12)


def test_groups_are_ordered_and_cut():
    from bmhrl_amd import evaluate as E
    results = {"v1": [seg(5, 9, "c"), seg(0, 10, "b"), seg(5, 9, "d"), seg(0, 4, "aé"), seg(1, 2, "cut away")]}
    ev = E.DenseCaptionEvaluator([GT_A], dict(HEAD, results=results), [0.5], 4, only_proposals=True, soda=True)
    groups, by_video = E.soda_groups(ev.ground_truths, ev.prediction)
    assert by_video == {"v1": [0], "v2": []} and len(groups) == 1
    g = groups[0]
    assert (g.video, g.file) == ("v1", 0)
    assert g.pred_sentences == ["a ", "b", "c", "d"]                  # (start, end) ascending, the tie in submission order
    assert g.pred_segments == [(0.0, 4.0), (0.0, 10.0), (5.0, 9.0), (5.0, 9.0)]
    assert g.ref_segments == [(0.0, 10.0), (10.0, 20.0)] and g.ref_sentences == ["A dog runs.", "The cat sits."]
    swapped = {"v1": {"timestamps": [[10, 20], [0, 10], [0, 5]], "sentences": ["x", "y", "z"]}}
    assert E.soda_groups([swapped], ev.prediction)[0][0].ref_sentences == ["x", "y", "z"]
    assert E.soda_groups([swapped], ev.prediction, sort_references=True)[0][0].ref_sentences == ["z", "y", "x"]
    ev.evaluate()                                                       # only_proposals: no SODA, no launch
    assert ev.scores == {} and ev.soda_per_video == {}


def test_value_errors_name_the_video():
    from bmhrl_amd import evaluate as E, ops
    from bmhrl_amd.rewards import MeteorTables
    tables = MeteorTables(["a", "b"], False, False)
    many = E.SodaGroup("v_many", 1, [(0.0, 1.0)], ["a"], [(0.0, 1.0)] * (ops.SODA_MAX_REFS + 1), ["b"] * (ops.SODA_MAX_REFS + 1))
    with pytest.raises(ValueError, match="v_many"):
        E.soda_scores([many], [0.5], tables, "cpu")
    long_h = E.SodaGroup("v_long", 0, [(0.0, 1.0)], ["a " * (ops.REWARDS_MAX_L + 1)], [(0.0, 1.0)], ["b"])
    with pytest.raises(ValueError, match="v_long"):
        E.soda_scores([long_h], [0.5], tables, "cpu")
    long_r = E.SodaGroup("v_ref", 0, [(0.0, 1.0)], ["a"], [(0.0, 1.0)], ["b " * (ops.REWARDS_MAX_R + 1)])
    with pytest.raises(ValueError, match="v_ref"):
        E.soda_scores([long_r], [0.5], tables, "cpu")
    with pytest.raises(ValueError):
        E.soda_scores([long_r], [0.5] * (ops.SODA_MAX_T + 1), tables, "cpu")
    assert E.soda_scores([], [0.3, 0.5], tables, "cpu").shape == (0, 2, 4)


def test_without_soda_the_scores_keep_their_keys(monkeypatch):
    from bmhrl_amd import evaluate as E
    results = {"v1": [seg(0, 10, "a dog runs")]}
    ev, _ = evaluator(monkeypatch, [GT_A], results, soda=False, verbose=True)
    assert list(ev.scores) == list(E.METRICS) + ["Recall", "Precision"] and ev.soda_per_video == {}

    def refuse(*a, **k):
        raise AssertionError("soda=False launches nothing new")
    monkeypatch.setattr(E, "soda_scores", refuse)
    ev.evaluate()
    default = E.DenseCaptionEvaluator([GT_A], dict(HEAD, results=results), [0.5], device="cpu", stemmer=False, synonyms=False)
    assert default.soda is False and default.sort_references is False
    default.evaluate()
    assert list(default.scores) == list(E.METRICS)
    ev2, _ = evaluator(monkeypatch, [GT_A], results, soda=True, verbose=True)
    assert list(ev2.scores) == list(E.METRICS) + list(E.SODA_METRICS) + ["Recall", "Precision"]
    assert all(len(v) == 2 for v in ev2.scores.values())
