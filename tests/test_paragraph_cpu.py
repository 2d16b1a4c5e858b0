"""The host half of the paragraph evaluation without a device: the restatement
(tests/paragraph_reference.py) against the hand check, and evaluate.paragraph_groups -- which sentences form a paragraph, in
which order, and what is refused -- against the restatement and against cases written out here."""
import pytest

from tests import paragraph_reference as pr


def seg(start, end, sentence, score=None):
    out = {"timestamp": [start, end], "sentence": sentence}
    if score is not None:
        out["proposal_score"] = score
    return out


def gt_entry(*caps):
    return {"duration": 100.0, "timestamps": [[s, e] for s, e, _ in caps], "sentences": [c for _, _, c in caps]}


@pytest.fixture()
def job():
    """two ground-truth files and a submission: v1 in both files, v2 in file 0 only, v3 without a prediction, v4 whose only
    prediction cleans to nothing, v5 whose reference in file 1 cleans to nothing, zz in the prediction only"""
    gts = [{"v1": gt_entry((10, 20, "A man plays the guitar."), (0, 5, "The crowd waits.")),
            "v2": gt_entry((0, 9, "A dog runs.")),
            "v3": gt_entry((0, 9, "Nothing is predicted here.")),
            "v4": gt_entry((0, 9, "A cat sleeps.")),
            "v5": gt_entry((0, 9, "Two men talk."))},
           {"v1": gt_entry((0, 6, "People wait — for the café concert."), (9, 21, "He plays a guitar on stage !")),
            "v4": gt_entry((0, 8, "The cat is asleep.")),
            "v5": gt_entry((0, 9, "…"), (1, 2, " ?! "))}]
    results = {"v1": [seg(10, 20, "a man plays a guitar", 0.5), seg(0, 5, "the crowd waits", 0.9),
                      seg(10, 20, "he plays the guitar", 0.5), seg(10, 15, "…", 0.99), seg(0, 5, "a crowd claps", 0.1),
                      seg(30, 40, "the man bows", 0.5), seg(21, 25, "a man plays a guitar again", 0.2)],
               "v2": [seg(2, 3, "a dog runs")],
               "v4": [seg(0, 1, " … ", 0.3)],
               "v5": [seg(0, 1, "two men talk", 0.3)],
               "zz": [seg(0, 1, "only predicted", 0.3)]}
    return gts, results


def words(para):
    return [" ".join(s) for s in para]


def test_restatement_reproduces_the_hand_check():
    assert pr.ngram_stats(pr.HAND_PARAGRAPH) == pr.HAND_STATS
    r4, r1, r2 = pr.HAND_STATS[3], pr.HAND_STATS[0], pr.HAND_STATS[1]
    assert (r4[0] - r4[1]) / r4[0] == 0.375 and r4[3] / r4[0] == 0.375
    assert r1[1] / r1[0] == 10 / 17 and r2[1] / r2[0] == 9 / 14


def test_restatement_edge_paragraphs():
    assert pr.ngram_stats([]) == [[0] * 5] * 4 and pr.ngram_stats([[]]) == [[0] * 5] * 4
    assert pr.ngram_stats(["the the the the the".split()])[1] == [4, 1, 4, 0, 4]
    twice = pr.ngram_stats(["a b c".split(), "a b c".split()])
    assert twice == [[6, 3, 6, 3, 2], [4, 2, 4, 2, 2], [2, 1, 2, 1, 2], [0, 0, 0, 0, 0]]
    # "b c" would match only across the boundary of the first two sentences
    assert pr.ngram_stats(["a b".split(), "c d".split(), "b c".split()])[1] == [3, 3, 0, 0, 1]
    assert pr.flatten([[("a", "b"), ()], [], [("c",)]]) == (["a", "b", "c"], [0, 2, 2, 3], [0, 2, 2, 3])


def test_predicted_paragraph_time_order_ties_and_top(job):
    from bmhrl_amd.evaluate import paragraph_groups
    gts, results = job
    g = paragraph_groups(gts, results, str.split)
    assert g.vids == ["v1", "v2", "v3", "v4", "v5"]                       # sorted; zz is not a ground-truth video
    # (start, end) ascending; [0, 5] twice and [10, 20] twice keep list order; "…" is dropped: no token is left
    assert words(g.predicted["v1"]) == ["the crowd waits", "a crowd claps", "a man plays a guitar", "he plays the guitar",
                                        "a man plays a guitar again", "the man bows"]
    assert g.predicted["v3"] == [] and g.predicted["v4"] == [] and "zz" not in g.predicted
    # top 3 by score: 0.99 (cleans to nothing), 0.9, then the first of the three 0.5s in list order
    assert words(paragraph_groups(gts, results, str.split, top=3).predicted["v1"]) == ["the crowd waits", "a man plays a guitar"]
    assert words(paragraph_groups(gts, results, str.split, top=4).predicted["v1"]) == ["the crowd waits", "a man plays a guitar",
                                                                                     "he plays the guitar"]
    assert words(paragraph_groups(gts, results, str.split, top=1).predicted["v1"]) == []
    assert paragraph_groups(gts, results, str.split, top=100).predicted == g.predicted
    for top in (None, 1, 3, 4):
        got = paragraph_groups(gts, results, str.split, top=top)
        for vid in got.vids:
            assert got.predicted[vid] == pr.predicted_paragraph(results.get(vid, []), str.split, top), (vid, top)


def test_reference_paragraphs_files_nonascii_and_sort_references(job):
    from bmhrl_amd.evaluate import paragraph_groups, tokenize
    gts, results = job
    g = paragraph_groups(gts, results, tokenize)
    assert [sorted(r) for r in g.references] == [["v1", "v2", "v3", "v4", "v5"], ["v1", "v4"]]   # v5: no token left in file 1
    assert words(g.references[0]["v1"]) == ["a man plays the guitar", "the crowd waits"]          # file order
    assert words(g.references[1]["v1"]) == ["people wait for the caf concert", "he plays a guitar on stage"]
    s = paragraph_groups(gts, results, tokenize, sort_references=True)
    assert words(s.references[0]["v1"]) == ["the crowd waits", "a man plays the guitar"]
    assert s.predicted == g.predicted
    for sort in (False, True):
        got = paragraph_groups(gts, results, tokenize, sort_references=sort)
        for f, gt in enumerate(gts):
            for vid in got.vids:
                want = pr.reference_paragraph(gt[vid], tokenize, sort) if vid in gt else []
                assert got.references[f].get(vid, []) == want, (f, vid, sort)


def test_restatement_scores_an_empty_prediction_and_averages_the_files(job):
    from bmhrl_amd.evaluate import tokenize
    gts, results = job
    sub = {"results": results, "version": "x", "external_data": {}}
    scores, per_video = pr.evaluate(gts, sub, 2, 1000, tokenize)
    assert sorted(scores) == sorted(["Para_" + m for m in pr.METRICS] + list(pr.STAT_KEYS))
    assert all(len(v) == 2 and v[0] == v[1] for v in scores.values())
    assert 0.0 < scores["Para_METEOR"][0] < 1.0 and 0.0 < scores["Para_CIDEr"][0] <= 10.0
    assert list(per_video) == ["v1", "v2", "v3", "v4", "v5"]
    assert per_video["v3"] == {"stats": [[0] * 5] * 4, "sentences": 0, "tokens": 0}
    assert per_video["v1"]["sentences"] == 6 and per_video["v1"]["tokens"] == 24
    assert per_video["v1"]["stats"] == pr.ngram_stats([s.split() for s in (
        "the crowd waits", "a crowd claps", "a man plays a guitar", "he plays the guitar", "a man plays a guitar again",
        "the man bows")])
    # RE_4: only v1 has a 4-gram -- six, two of them the second "a man plays a guitar"; Div_1: v1, v2 and v5 have a word
    assert scores["Para_RE_4"][0] == (6 - 4) / 6 == scores["Para_XRE_4"][0]
    assert scores["Para_Div_1"][0] == (11 / 24 + 1.0 + 1.0) / 3
    one = pr.evaluate(gts, sub, 1, 1000, tokenize, top=1)[0]
    assert one["Para_Bleu_1"][0] < scores["Para_Bleu_1"][0]               # v1's best-scored proposal cleans to nothing


def test_limits_name_the_video_and_touch_no_device(job):
    from bmhrl_amd import ops
    from bmhrl_amd.evaluate import DenseCaptionEvaluator, paragraph_groups
    gts, results = job
    long_pred = dict(results, v2=[seg(k, k + 1, "w " * 43, 1.0 - 0.01 * k) for k in range(6)])   # 258 > REWARDS_MAX_L
    with pytest.raises(ValueError, match=r"video v2.*258 tokens.*paragraph_top"):
        paragraph_groups(gts, long_pred, str.split)
    assert sum(map(len, paragraph_groups(gts, long_pred, str.split, top=5).predicted["v2"])) == 215
    assert ops.REWARDS_MAX_L == 256 and ops.REWARDS_MAX_R == 512
    long_ref = [gts[0], dict(gts[1], v4=gt_entry(*[(k, k + 1, "w " * 57) for k in range(9)]))]    # 513 > REWARDS_MAX_R
    with pytest.raises(ValueError, match=r"video v4.*513 tokens.*file 1.*paragraph_top"):
        paragraph_groups(long_ref, results, str.split)
    # through the evaluator, on a device no launch accepts: the refusal comes before anything is uploaded
    sub = {"results": long_pred, "version": "x", "external_data": {}}
    ev = DenseCaptionEvaluator(gts, sub, [0.5], device="cpu", tokenizer=str.split, stemmer=False, synonyms=False, paragraph=True)
    with pytest.raises(ValueError, match="video v2"):
        ev.evaluate_paragraph()
    ev = DenseCaptionEvaluator(long_ref, {"results": results, "version": "x", "external_data": {}}, [0.5], device="cpu",
                               tokenizer=str.split, stemmer=False, synonyms=False, paragraph=True, paragraph_top=2)
    with pytest.raises(ValueError, match="video v4"):
        ev.evaluate_paragraph()


def test_constructor_keywords(job):
    from bmhrl_amd.evaluate import DenseCaptionEvaluator
    gts, results = job
    sub = {"results": results, "version": "x", "external_data": {}}
    for bad in (0, -1, 2.0, "3", True):
        with pytest.raises(ValueError, match="paragraph_top"):
            DenseCaptionEvaluator(gts, sub, [0.5], only_proposals=True, paragraph_top=bad)
    ev = DenseCaptionEvaluator(gts, sub, [0.5], only_proposals=True, paragraph=True, paragraph_top=10)
    assert ev.paragraph is True and ev.paragraph_top == 10 and ev.paragraph_per_video == {}
    ev.evaluate()                                                         # only_proposals: no paragraph keys
    assert ev.scores == {}
    ev = DenseCaptionEvaluator(gts, sub, [0.5], only_proposals=True)
    assert ev.paragraph is False and ev.paragraph_top is None


def test_means_of_the_integers():
    import numpy as np
    from bmhrl_amd.evaluate import paragraph_means
    stats = np.zeros((3, 4, 5), dtype=np.int32)
    stats[0] = pr.HAND_STATS
    stats[2, 0] = [3, 3, 0, 0, 1]                                         # a video of three words: no 2-gram counted here
    got = paragraph_means(stats)
    assert got == {"Para_RE_4": 0.375, "Para_XRE_4": 0.375, "Para_Div_1": (10 / 17 + 1.0) / 2, "Para_Div_2": 9 / 14}
    assert paragraph_means(stats[1:2]) == {"Para_RE_4": 0.0, "Para_XRE_4": 0.0, "Para_Div_1": 0.0, "Para_Div_2": 0.0}
