"""The host half of the proposal metrics without a GPU: the plain-Python restatement
(tests/proposal_eval_reference.py) against a hand check, against evaluate.pair_captions / detection_scores on the fixture
(tests/golden/caption_eval.json), segment_tables' layouts there, the proposal_score rules and the argument checks of the ops
that need no device."""
import json
import os

import numpy as np
import pytest
import torch

from tests import proposal_eval_reference as pr
from tests.conftest import GOLDEN

# the hand check: one file, two videos
HAND_GT = {"a": {"timestamps": [[0, 10], [20, 30]], "sentences": ["a0", "a1"]},
           "b": {"timestamps": [[5, 15]], "sentences": ["b0"]}}
HAND_PRED = {"a": [{"sentence": "", "timestamp": [21, 29], "proposal_score": 0.9},
                   {"sentence": "", "timestamp": [0, 4], "proposal_score": 0.8},
                   {"sentence": "", "timestamp": [1, 10], "proposal_score": 0.7},
                   {"sentence": "", "timestamp": [50, 60], "proposal_score": 0.6}],
             "b": [{"sentence": "", "timestamp": [0, 30], "proposal_score": 0.5},
                   {"sentence": "", "timestamp": [6, 15], "proposal_score": [0.95]}]}
HAND_TIOUS = [0.5, 0.75, 0.9]


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLDEN, "caption_eval.json")) as f:
        fx = json.load(f)
    fx["prediction"] = {vid: segs[:fx["max_proposals"]] for vid, segs in fx["submission"]["results"].items()}
    return fx


def test_hand_check_cells_and_curve():
    assert pr.tiou([21, 29], [20, 30]) == 0.7999999992
    assert pr.tiou([1, 10], [0, 10]) == 0.8999999991 and pr.tiou([6, 15], [5, 15]) == 0.8999999991
    assert pr.tiou([0, 30], [5, 15]) == 0.3333333332222222
    out = pr.proposal_recall([HAND_GT], HAND_PRED, HAND_TIOUS, max_avg_nr_proposals=2, points=4)
    assert out["proposals_per_video"] == [0.5, 1.0, 1.5, 2.0]
    third = 1 / 3.0
    assert out["recall_curve"][0] == out["recall_curve"][1] == [0.0, third, 2 / 3.0, 2 / 3.0]
    assert out["recall_curve"][2] == [0.0] * 4
    assert out["AUC"] == [33.33333333333333, 33.33333333333333, 0.0]
    assert out["AR@AN"] == [2 / 3.0, 2 / 3.0, 0.0]


def test_hand_check_with_the_defaults():
    out = pr.proposal_recall([HAND_GT], HAND_PRED, HAND_TIOUS)
    for t in (0, 1):
        assert [out["recall_curve"][t][k - 1] for k in (25, 50, 75, 100)] == [1.0] * 4
        assert out["AUC"][t] == 98.33333333333331 and out["AR@AN"][t] == 1.0
    assert out["AUC"][2] == 0.0 and out["recall_curve"][2] == [0.0] * 100


def test_hand_check_tables():
    # video a in score order: [21,29], [0,4], [1,10], [50,60] against [0,10], [20,30]
    segs = [p["timestamp"] for p in HAND_PRED["a"]]
    hits, first = pr.hit_tables(segs, HAND_GT["a"]["timestamps"], [(0, 4, 0, 2)], HAND_TIOUS, False)
    assert hits == [[1, 0, 1, 0], [1, 0, 1, 0], [0, 0, 0, 0]]
    assert first == [[2, 0], [2, 0], [4, 4]]
    # the threshold that equals a cell's value: >= passes, > does not
    cell = pr.tiou(segs[2], [0, 10])
    assert pr.hit_tables(segs, [[0, 10]], [(0, 4, 0, 1)], [cell], False) == ([[0, 0, 1, 0]], [[2]])
    assert pr.hit_tables(segs, [[0, 10]], [(0, 4, 0, 1)], [cell], True) == ([[0, 0, 0, 0]], [[4]])
    assert pr.pair_list(segs, HAND_GT["a"]["timestamps"], [(0, 4, 0, 2)], 0.5) == [(0, 1), (1, -1), (2, 0), (3, -1)]
    # a group without predictions: every reference's first rank is P = 0
    assert pr.hit_tables([], [[0, 1]], [(0, 0, 0, 1)], [0.5], True) == ([[]], [[0]])


def test_restatement_equals_the_host_functions_on_the_fixture(fixture):
    from bmhrl_amd import evaluate as E
    gts, pred = fixture["ground_truths"], fixture["prediction"]
    for t in fixture["tious"] + [0.0]:
        assert pr.detection(gts, pred, t) == E.detection_scores(gts, pred, t)
        host = E.pair_captions(gts, pred, t)
        mine = pr.pairs_of_job(gts, pred, t)
        assert list(host) == list(mine)
        for vid in host:
            want = [(E.remove_nonascii(pred[vid][pi]["sentence"]),
                     None if r is None else E.remove_nonascii(gts[r[0]][vid]["sentences"][r[1]])) for pi, r in mine[vid]]
            assert host[vid] == want
    for k, t in enumerate(fixture["tious"]):
        p, r = pr.detection(gts, pred, t)
        assert p == fixture["scores"]["Precision"][k] and r == fixture["scores"]["Recall"][k]


def test_segment_tables_layout_on_the_fixture(fixture):
    from bmhrl_amd import evaluate as E
    gts, pred = fixture["ground_truths"], fixture["prediction"]
    tb = E.segment_tables(gts, pred)
    vids = E.ground_truth_video_ids(gts)
    assert tb.vids == vids and tb.n_files == len(gts) and "p99" not in vids
    # the cases the fixture is there for
    assert any(sum(v in g for g in gts) == 1 for v in vids) and any(not pred.get(v) for v in vids)
    assert any(len(fixture["submission"]["results"][v]) > fixture["max_proposals"] for v in vids if v in pred)
    p = r = g = 0
    for v, vid in enumerate(vids):
        mine = pred.get(vid, [])
        assert tb.pred_off[v] == p and tb.ref_off[v] == r and tb.group_off[v] == g
        assert tb.pred_seg[p:p + len(mine)].tolist() == [[float(x) for x in q["timestamp"]] for q in mine]
        assert tb.pred_sentences[p:p + len(mine)] == [q["sentence"] for q in mine]
        assert (tb.pred_video[p:p + len(mine)] == v).all()
        r0 = r
        for f, gt in enumerate(gts):
            if vid not in gt:
                continue
            stamps = gt[vid]["timestamps"]
            assert tb.file_groups[g].tolist() == [p, len(mine), r, len(stamps)]
            assert (tb.group_video[g], tb.group_file[g]) == (v, f)
            assert tb.ref_seg[r:r + len(stamps)].tolist() == [[float(x) for x in s] for s in stamps]
            assert tb.ref_sentences[r:r + len(stamps)] == gt[vid]["sentences"] and (tb.ref_file[r:r + len(stamps)] == f).all()
            r += len(stamps)
            g += 1
        assert tb.video_groups[v].tolist() == [p, len(mine), r0, r - r0]
        p += len(mine)
    assert (p, r, g) == (len(tb.pred_seg), len(tb.ref_seg), len(tb.file_groups)) == (tb.pred_off[-1], tb.ref_off[-1], tb.group_off[-1])
    assert tb.pred_seg.dtype == tb.ref_seg.dtype == np.float64 and tb.file_groups.dtype == tb.video_groups.dtype == np.int32
    # the tables' groups reproduce the host functions through the restatement's tables
    for t in fixture["tious"]:
        pairs = pr.pair_list(tb.pred_seg.tolist(), tb.ref_seg.tolist(), tb.video_groups.tolist(), t)
        host = E.pair_captions(gts, pred, t)
        want = [pair for vid in vids for pair in host[vid]]
        got = [(E.remove_nonascii(tb.pred_sentences[s]), None if r < 0 else E.remove_nonascii(tb.ref_sentences[r]))
               for s, r in pairs]
        assert got == want


def test_proposal_score_rules_and_the_stable_order():
    from bmhrl_amd import evaluate as E
    preds = [{"timestamp": [0, 1], "proposal_score": 0.5}, {"timestamp": [1, 2]}, {"timestamp": [2, 3], "proposal_score": [0.5]},
             {"timestamp": [3, 4], "proposal_score": (0.9,)}, {"timestamp": [4, 5], "proposal_score": 0.0},
             {"timestamp": [5, 6], "proposal_score": 0.5}]
    assert [E.proposal_score_of(p) for p in preds] == [0.5, 0.0, 0.5, 0.9, 0.0, 0.5] == [pr.score_of(p) for p in preds]
    assert E.by_proposal_score(preds) == [3, 0, 2, 5, 1, 4] == pr.score_order(preds)
    gt = {"v": {"timestamps": [[0, 6]], "sentences": ["s"]}}
    tb = E.segment_tables([gt], {"v": preds}, by_score=True)
    assert tb.pred_seg[:, 0].tolist() == [3.0, 0.0, 2.0, 5.0, 1.0, 4.0]
    assert E.segment_tables([gt], {"v": preds}).pred_seg[:, 0].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]
    # the order decides the ranks: the restatement's curve changes when the scores are dropped
    with_scores = pr.proposal_recall([HAND_GT], HAND_PRED, [0.5], 2, 4)
    bare = {v: [{"timestamp": p["timestamp"]} for p in ps] for v, ps in HAND_PRED.items()}
    assert pr.proposal_recall([HAND_GT], bare, [0.5], 2, 4)["recall_curve"] != with_scores["recall_curve"]


def test_keywords_default_to_the_host_routes(fixture):
    from bmhrl_amd import evaluate as E
    ev = E.DenseCaptionEvaluator(fixture["ground_truths"], fixture["submission"], fixture["tious"], fixture["max_proposals"],
                                 verbose=False, only_proposals=True)
    assert ev.tiou_backend == "host" and ev.proposal_recall is False and ev.recall_curve is None
    ev.verbose = True
    ev.evaluate()                                                  # no device is touched
    assert list(ev.scores) == ["Recall", "Precision"] and ev.scores["Recall"] == fixture["scores"]["Recall"]
    with pytest.raises(ValueError, match="tiou_backend"):
        E.DenseCaptionEvaluator(fixture["ground_truths"], fixture["submission"], [0.5], only_proposals=True, tiou_backend="gpu")


def test_ops_checks_that_need_no_device():
    from bmhrl_amd import ops
    seg = torch.zeros(3, 2, dtype=torch.float64)
    tious = torch.tensor([0.5], dtype=torch.float64)
    groups = ops.TiouGroups([[0, 3, 0, 3], [0, 3, 1, 2]], "cpu")
    assert groups.G == 2 and (groups.sum_p, groups.sum_r) == (6, 5) and groups.host.dtype == np.int32
    assert groups.out_off.tolist() == [[0, 3, 6], [0, 3, 5]] and groups.groups.tolist() == groups.host.tolist()
    assert ops.TiouGroups([], "cpu").G == 0
    for bad in ([[0, 1, 0]], [0, 1, 0, 1], [[0, -1, 0, 1]], [[0.0, 1.0, 0.0, 1.0]], [[0, 2**31, 0, 1]]):
        with pytest.raises(ValueError, match="TiouGroups"):
            ops.TiouGroups(bad, "cpu")
    with pytest.raises(ValueError, match="TiouGroups"):
        ops.tiou_hits(seg, seg, [[0, 3, 0, 3]], tious, True)
    for bad_seg in (seg.float(), torch.zeros(3, 3, dtype=torch.float64), torch.zeros(2, 6, dtype=torch.float64)[:, ::3]):
        with pytest.raises(ValueError, match="fp64"):
            ops.tiou_hits(bad_seg, seg, groups, tious, True)
        with pytest.raises(ValueError, match="fp64"):
            ops.tiou_pairs(seg, bad_seg, groups, 0.5, torch.zeros(7, dtype=torch.int64), 6)
    for bad_t in (tious.float(), torch.zeros(0, dtype=torch.float64), torch.zeros(ops.TIOU_MAX_T + 1, dtype=torch.float64),
                  torch.zeros(1, 1, dtype=torch.float64)):
        with pytest.raises(ValueError, match="tious"):
            ops.tiou_hits(seg, seg, groups, bad_t, True)
    for bad_out in ((torch.zeros(1, 5, dtype=torch.int32), torch.zeros(1, 5, dtype=torch.int32)),          # row too short
                    (torch.zeros(1, 6, dtype=torch.int64), torch.zeros(1, 5, dtype=torch.int32)),
                    (torch.zeros(2, 6, dtype=torch.int32), torch.zeros(1, 5, dtype=torch.int32))):
        with pytest.raises(ValueError, match="out"):
            ops.tiou_hits(seg, seg, groups, tious, True, out=bad_out)
    for bad_off in (torch.zeros(6, dtype=torch.int64), torch.zeros(7, dtype=torch.int32)):
        with pytest.raises(ValueError, match="pair_off"):
            ops.tiou_pairs(seg, seg, groups, 0.5, bad_off, 6)
    with pytest.raises(ValueError, match="n_pairs"):
        ops.tiou_pairs(seg, seg, groups, 0.5, torch.zeros(7, dtype=torch.int64), 6, out=torch.zeros(5, dtype=torch.int32))
    # well-formed arguments on the CPU reach the device check, not a kernel
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tiou_hits(seg, seg, groups, tious, True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tiou_pairs(seg, seg, groups, 0.5, torch.zeros(7, dtype=torch.int64), 6)
