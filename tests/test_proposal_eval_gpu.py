"""Proposal metrics on the MI355X (csrc/proposal_eval.hip, bmhrl_amd/evaluate.py) against the
plain-Python restatement (tests/proposal_eval_reference.py) and the host routes of the evaluator.  The kernels compute
evaluate.tiou's fp64 bits, so every integer is compared exactly, and the host floats built from the integers are compared
with ==: they are the same expressions over the same integers."""
import json
import math
import os
import random

import numpy as np
import pytest
import torch

from tests import proposal_eval_reference as pr
from tests.conftest import GOLDEN
from tests.meteor_reference import DictStemmer, dict_synonyms
from tests.test_proposal_eval_cpu import HAND_GT, HAND_PRED, HAND_TIOUS

pytestmark = pytest.mark.gpu

SENTINEL = -7
P_SIZES, R_SIZES, R_LARGE = (0, 1, 63, 64, 65, 130), (1, 3, 64, 65), 300      # no cap on R: one group far past SODA's 256
THRESHOLDS = {1: [0.5], 4: [0.3, 0.5, 0.7, 0.9], 16: [k / 16.0 for k in range(16)]}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bmhrl_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def segments(rng, n):
    """times on a grid of 0.01 inside a short span: equal endpoints, touching and zero-length segments occur"""
    out = []
    for _ in range(n):
        s = round(rng.uniform(0.0, 3.0), 2)
        out.append([s, round(s + rng.choice([0.0, 0.5, 1.0, rng.uniform(0.0, 2.0)]), 2)])
    return out


@pytest.fixture(scope="module")
def job():
    """every (P, R) of the size lists as a group of its own runs, one group with R_LARGE references, one without
    references, and one that shares the predictions of another; the cell values once for all tests"""
    rng = random.Random(5)
    pred_seg, ref_seg, groups = [], [], []
    for P in P_SIZES:
        for R in R_SIZES + ((R_LARGE,) if P == 65 else ()):
            groups.append((len(pred_seg), P, len(ref_seg), R))
            pred_seg += segments(rng, P)
            ref_seg += segments(rng, R)
    groups.append((groups[-1][0], 130, len(ref_seg), 5))               # the last group's predictions, other references
    ref_seg += segments(rng, 5)
    groups.append((3, 7, 0, 0))                                        # no reference
    return {"pred_seg": pred_seg, "ref_seg": ref_seg, "groups": groups, "cells": pr.iou_cells(pred_seg, ref_seg, groups)}


def on_device(job, dev):
    from bmhrl_amd import ops
    f64 = lambda a: torch.tensor(a, dtype=torch.float64, device=dev).reshape(-1, 2)                       # noqa: E731
    return f64(job["pred_seg"]), f64(job["ref_seg"]), ops.TiouGroups(job["groups"], dev)


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("T", [1, 4, 16])
def test_group_shapes(dev, job, T, strict):
    from bmhrl_amd import ops
    pred_seg, ref_seg, groups = on_device(job, dev)
    tious = THRESHOLDS[T]
    hits, first = ops.tiou_hits(pred_seg, ref_seg, groups, torch.tensor(tious, dtype=torch.float64, device=dev), strict)
    want_hits, want_first = pr.hit_tables(job["pred_seg"], job["ref_seg"], job["groups"], tious, strict, job["cells"])
    assert hits.dtype == first.dtype == torch.int32
    assert hits.shape == (T, groups.sum_p) and first.shape == (T, groups.sum_r)
    assert hits.cpu().tolist() == want_hits
    assert first.cpu().tolist() == want_first
    # the job does what it is there for: hits and misses at both ends, equal endpoints
    flat = [c for cell in job["cells"] for row in cell for c in row]
    firsts = [f for row in want_first for f in row]
    assert 0.0 in flat and max(flat) > 0.9 and any(0 < f < 64 for f in firsts) and any(64 <= f < 130 for f in firsts)


def test_threshold_equal_to_a_cell(dev):
    from bmhrl_amd import evaluate as E, ops
    preds, refs = [[0.0, 4.0], [1.0, 10.0], [2.5, 9.75]], [[0.0, 10.0], [2.0, 9.0]]
    cell = E.tiou(preds[1], refs[0])
    assert cell == 0.8999999991
    pred_seg = torch.tensor(preds, dtype=torch.float64, device=dev)
    ref_seg = torch.tensor(refs, dtype=torch.float64, device=dev)
    groups = ops.TiouGroups([[0, 3, 0, 2]], dev)
    tious = torch.tensor([cell, E.tiou(preds[2], refs[1])], dtype=torch.float64, device=dev)
    loose = [x.cpu().tolist() for x in ops.tiou_hits(pred_seg, ref_seg, groups, tious, False)]
    tight = [x.cpu().tolist() for x in ops.tiou_hits(pred_seg, ref_seg, groups, tious, True)]
    assert loose == [list(x) for x in pr.hit_tables(preds, refs, [(0, 3, 0, 2)], tious.tolist(), False)]
    assert tight == [list(x) for x in pr.hit_tables(preds, refs, [(0, 3, 0, 2)], tious.tolist(), True)]
    assert loose[0][0][1] == 1 and loose[1][0][0] == 1                  # the cell itself passes >= ...
    assert tight[0][0][1] == 0 and tight[1][0][0] == 3                  # ... and not >: no prediction is left for the reference
    assert loose[0][1][2] == 1 and tight[0][1][2] == 0                  # the second threshold is the cell (2, 1)


def test_segment_edge_cases(dev):
    from bmhrl_amd import ops
    # zero-length prediction, identical, touching (intersection 0), nested both ways, disjoint; a zero-length reference
    preds = [[5.0, 5.0], [0.0, 10.0], [10.0, 20.0], [2.0, 3.0], [-5.0, 50.0], [30.0, 40.0]]
    refs = [[0.0, 10.0], [5.0, 5.0]]
    tious = [0.0, 1e-9, 0.1, 0.5, 1.0]
    pred_seg = torch.tensor(preds, dtype=torch.float64, device=dev)
    ref_seg = torch.tensor(refs, dtype=torch.float64, device=dev)
    groups = ops.TiouGroups([[0, 6, 0, 2]], dev)
    for strict in (False, True):
        got = [x.cpu().tolist() for x in ops.tiou_hits(pred_seg, ref_seg, groups,
                                                       torch.tensor(tious, dtype=torch.float64, device=dev), strict)]
        assert got == [list(x) for x in pr.hit_tables(preds, refs, [(0, 6, 0, 2)], tious, strict)]
        if strict:
            assert got[0][0] == [0, 1, 0, 1, 1, 0]                      # > 0: only a real intersection
            assert got[0][4] == [0] * 6 and got[1][4] == [6, 6]         # identical segments stay under 1: the + 1e-8
        else:
            assert got[0][0] == [2] * 6 and got[1][0] == [0, 0]         # >= 0: everything, the first prediction first


def test_sentinels_and_repeatability(dev, job):
    from bmhrl_amd import ops
    pred_seg, ref_seg, groups = on_device(job, dev)
    tious = torch.tensor(THRESHOLDS[4], dtype=torch.float64, device=dev)
    runs = []
    for _ in range(2):
        out = (torch.full((4, groups.sum_p + 9), SENTINEL, dtype=torch.int32, device=dev),
               torch.full((4, groups.sum_r + 5), SENTINEL, dtype=torch.int32, device=dev))
        hits, first = ops.tiou_hits(pred_seg, ref_seg, groups, tious, False, out=out)
        assert hits.data_ptr() == out[0].data_ptr() and hits.shape[1] == groups.sum_p
        assert (out[0][:, groups.sum_p:] == SENTINEL).all() and (out[1][:, groups.sum_r:] == SENTINEL).all()
        assert (hits >= 0).all() and (first >= 0).all()
        off = torch.zeros(groups.sum_p + 1, dtype=torch.int64, device=dev)
        torch.cumsum(hits[1].clamp(min=1), 0, out=off[1:])
        n = int(off[-1])
        rows = torch.full((n + 11,), SENTINEL, dtype=torch.int32, device=dev)
        pairs = ops.tiou_pairs(pred_seg, ref_seg, groups, THRESHOLDS[4][1], off, n, out=rows)
        assert pairs.shape == (n,) and (rows[n:] == SENTINEL).all() and (pairs != SENTINEL).all()
        runs.append((out[0].cpu(), out[1].cpu(), rows.cpu()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    # without predictions nothing is written on that side; G = 0 launches nothing
    empty = ops.TiouGroups([], dev)
    out = (torch.full((4, 3), SENTINEL, dtype=torch.int32, device=dev), torch.full((4, 3), SENTINEL, dtype=torch.int32, device=dev))
    hits, first = ops.tiou_hits(pred_seg, ref_seg, empty, tious, True, out=out)
    assert hits.shape == (4, 0) and first.shape == (4, 0) and (out[0] == SENTINEL).all() and (out[1] == SENTINEL).all()


@pytest.mark.parametrize("threshold", THRESHOLDS[4])
def test_pairs(dev, job, threshold):
    from bmhrl_amd import ops
    pred_seg, ref_seg, groups = on_device(job, dev)
    hits, _ = ops.tiou_hits(pred_seg, ref_seg, groups, torch.tensor([threshold], dtype=torch.float64, device=dev), False)
    counts = hits[0].clamp(min=1).to(torch.int64)
    off = torch.zeros(groups.sum_p + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=off[1:])
    pairs = ops.tiou_pairs(pred_seg, ref_seg, groups, threshold, off, int(off[-1])).cpu().tolist()
    slots = np.repeat(np.arange(groups.sum_p), counts.cpu().numpy()).tolist()
    want = pr.pair_list(job["pred_seg"], job["ref_seg"], job["groups"], threshold, job["cells"])
    assert list(zip(slots, pairs)) == want
    assert -1 in pairs and any(c > 1 for c in counts.cpu().tolist())


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLDEN, "caption_eval.json")) as f:
        return json.load(f)


def test_fixture_end_to_end(dev, fixture):
    from bmhrl_amd.evaluate import DenseCaptionEvaluator
    fx = fixture
    make = lambda backend: DenseCaptionEvaluator(fx["ground_truths"], fx["submission"], fx["tious"], fx["max_proposals"],  # noqa: E731
                                                 verbose=True, device=dev, stemmer=DictStemmer(), synonyms=dict_synonyms,
                                                 tiou_backend=backend)
    host, device = make("host"), make("device")
    for t in fx["tious"]:
        assert device.tokenized_pairs(t) == host.tokenized_pairs(t)
        assert device.evaluate_detection(t) == host.evaluate_detection(t)
    assert device.evaluate_detection(0.42) == host.evaluate_detection(0.42)       # a threshold outside the evaluator's own
    host.evaluate()
    device.evaluate()
    assert list(device.scores) == list(host.scores) and device.scores == host.scores
    assert device.scores["Recall"] == fx["scores"]["Recall"] and device.scores["Precision"] == fx["scores"]["Precision"]


def random_recall_job(seed=11, videos=40):
    rng = random.Random(seed)
    gts, pred = [{}, {}], {}
    for v in range(videos):
        vid = f"v{v:03d}"
        files = [0, 1] if v % 5 else [v % 2]                            # some videos in one file only
        for f in files:
            stamps = segments(rng, rng.randint(1, 5))
            gts[f][vid] = {"timestamps": stamps, "sentences": ["s"] * len(stamps)}
        n = rng.choice([0, 1, 2, 7, 30, rng.randint(0, 30)])
        pred[vid] = [{"sentence": "", "timestamp": s, "proposal_score": [round(rng.random(), 1)]} for s in segments(rng, n)]
        if v % 7 == 0:
            del pred[vid]                                               # no entry at all
    pred["only_predicted"] = [{"sentence": "", "timestamp": [0.0, 1.0], "proposal_score": [0.5]}]
    return gts, pred


def check_recall(got, want):
    assert got["AUC"] == want["AUC"] and got["AR@AN"] == want["AR@AN"]
    assert got["recall_curve"].tolist() == want["recall_curve"]
    assert got["proposals_per_video"].tolist() == want["proposals_per_video"]


def test_proposal_recall(dev):
    from bmhrl_amd import evaluate as E
    from bmhrl_amd.epoch_loops.validation_loops import calculate_metrics
    got = E.proposal_recall([HAND_GT], HAND_PRED, HAND_TIOUS, max_avg_nr_proposals=2, points=4, device=dev)
    check_recall(got, pr.proposal_recall([HAND_GT], HAND_PRED, HAND_TIOUS, 2, 4))
    assert got["AUC"] == [33.33333333333333, 33.33333333333333, 0.0] and got["proposals_per_video"].tolist() == [0.5, 1.0, 1.5, 2.0]
    assert E.proposal_recall([HAND_GT], HAND_PRED, HAND_TIOUS, device=dev)["AUC"] == [98.33333333333331, 98.33333333333331, 0.0]
    gts, pred = random_recall_job()
    tious = [0.5 + 0.05 * k for k in range(10)]
    want = pr.proposal_recall(gts, pred, tious)
    check_recall(E.proposal_recall(gts, pred, tious, device=dev), want)
    assert 0.0 < want["AUC"][0] < 100.0 and want["AUC"][0] > want["AUC"][-1]
    for one in ([gts[0]], [gts[1]]):                                    # a single file, other budgets
        check_recall(E.proposal_recall(one, pred, tious[:3], max_avg_nr_proposals=10, points=7, device=dev),
                     pr.proposal_recall(one, pred, tious[:3], 10, 7))
    nothing = E.proposal_recall(gts, {}, tious[:2], device=dev)
    assert nothing["AUC"] == [0.0, 0.0] and not nothing["recall_curve"].any()
    # through the evaluator and calculate_metrics: max_proposals cuts the lists first
    sub = {"version": "x", "external_data": {}, "results": pred}
    cut = {vid: segs[:12] for vid, segs in pred.items()}
    metrics = calculate_metrics(gts, sub, tious, 12, verbose=False, only_proposals=True, evaluator="device",
                                evaluator_options={"device": dev, "proposal_recall": True, "tiou_backend": "device"})
    want = pr.proposal_recall(gts, cut, tious)
    assert [metrics[t]["AUC"] for t in tious] == want["AUC"] and [metrics[t]["AR@AN"] for t in tious] == want["AR@AN"]
    assert metrics["Average across tIoUs"]["AUC"] == sum(want["AUC"]) / float(len(tious))
    assert set(metrics[tious[0]]) == {"AUC", "AR@AN"}


def test_validation_loop_reports_the_new_scalars(dev, tmp_path):
    from bmhrl_amd.epoch_loops.proposal_epoch_loops import validation_loop
    from bmhrl_amd.epoch_loops.validation_loops import calculate_metrics
    from tests.test_proposal_generator_gpu import B, TARGETS, Board, Loader, make_cfg, make_model
    tious = [0.3, 0.5, 0.7, 0.9]
    gt = {f"v_{i}_{b}": {"duration": [22.0, 20.5][b], "timestamps": [[t[1] - t[2] / 2, t[1] + t[2] / 2] for t in TARGETS if t[0] == b],
                         "sentences": ["a segment ." for t in TARGETS if t[0] == b]} for i in range(2) for b in range(B)}
    paths = []
    for n, drop in (("val_1.json", None), ("val_2.json", "v_1_1")):
        paths.append(str(tmp_path / n))
        with open(paths[-1], "w") as f:
            json.dump({k: v for k, v in gt.items() if k != drop}, f)
    boards = []
    for options in (None, {"tiou_backend": "device", "proposal_recall": True}):
        cfg = make_cfg(modality="audio_video", grad_clip=1.0, max_prop_per_vid=10, nms_tiou_thresh=0.4,
                       log_path=str(tmp_path / f"log{len(boards)}"), reference_paths=paths, tIoUs=tious, caption_evaluator="device",
                       device=str(dev))
        if options is not None:
            cfg.proposal_evaluator_options = options
        model = make_model(dev, cfg)
        boards.append(Board())
        best = validation_loop(cfg, model, torch.optim.Adam(model.parameters(), lr=1e-3), None, Loader(dev, "val_1"), 0, -1.0,
                               boards[-1])
        assert math.isfinite(best)
        # the scalars are the host loops' values for the submission this pass wrote
        sub = os.path.join(cfg.log_path, "submissions", "prop_results_val_1_e0_maxprop10.json")
        host = calculate_metrics(paths, sub, tious, 10, verbose=True, only_proposals=True, evaluator="device")
        for t in tious:
            assert boards[-1].scalars[f"densevid_eval_k/precision_{t}"] == host[t]["Precision"]
            assert boards[-1].scalars[f"densevid_eval_k/recall_{t}"] == host[t]["Recall"]
        assert boards[-1].scalars["metrics/avg_recall_at_k"] == host["Average across tIoUs"]["Recall"]
        if options is not None:
            with open(sub) as f:
                want = pr.proposal_recall([json.load(open(q)) for q in paths], json.load(f)["results"], tious)
            assert boards[-1].scalars["metrics/AUC"] == sum(want["AUC"]) / 4.0
            assert boards[-1].scalars["metrics/AR_at_AN"] == sum(want["AR@AN"]) / 4.0
    old, new = (b.scalars for b in boards)
    assert set(new) - set(old) == {"metrics/AUC", "metrics/AR_at_AN"} and set(old) <= set(new)
    assert set(old) == {f"densevid_eval_k/{m}_{t}" for m in ("precision", "recall", "F1") for t in tious} | \
        {"metrics/avg_precision_at_k", "metrics/avg_recall_at_k", "metrics/avg_F1_at_k"}
    assert 0.0 <= new["metrics/AUC"] <= 100.0 and 0.0 <= new["metrics/AR_at_AN"] <= 1.0


def test_refusals(dev):
    from bmhrl_amd import _lib, ops
    lib = _lib.load()
    seg = torch.zeros(4, 2, dtype=torch.float64, device=dev)
    tious = torch.tensor([0.5], dtype=torch.float64, device=dev)
    groups = ops.TiouGroups([[0, 4, 0, 4], [2, 2, 1, 3]], dev)
    hits = torch.full((1, 6), SENTINEL, dtype=torch.int32, device=dev)
    first = torch.full((1, 7), SENTINEL, dtype=torch.int32, device=dev)
    off = torch.arange(7, dtype=torch.int64, device=dev)
    rows = torch.full((6,), SENTINEL, dtype=torch.int32, device=dev)

    def hits_args(**over):
        a = dict(pred_seg=seg.data_ptr(), n_pred=4, ref_seg=seg.data_ptr(), n_ref=4, host=groups.host.ctypes.data,
                 groups=groups.groups.data_ptr(), out_off=groups.out_off.data_ptr(), G=2, tious=tious.data_ptr(), T=1, strict=1,
                 pred_hits=hits.data_ptr(), ld_pred=6, ref_first=first.data_ptr(), ld_ref=7, stream=ops.stream())
        a.update(over)
        return list(a.values())

    def pairs_args(**over):
        a = dict(pred_seg=seg.data_ptr(), n_pred=4, ref_seg=seg.data_ptr(), n_ref=4, host=groups.host.ctypes.data,
                 groups=groups.groups.data_ptr(), out_off=groups.out_off.data_ptr(), G=2, tiou=0.5, pair_off=off.data_ptr(),
                 n_slots=6, pair_ref=rows.data_ptr(), n_pairs=6, stream=ops.stream())
        a.update(over)
        return list(a.values())

    def table(rows_):
        return np.ascontiguousarray(rows_, dtype=np.int32)
    bad_tables = [table([[0, 4, 0, 4], [3, 2, 1, 3]]), table([[0, 4, 0, 4], [2, 2, 2, 3]]), table([[0, -1, 0, 4], [2, 2, 1, 3]]),
                  table([[-1, 2, 0, 4], [2, 2, 1, 3]]), table([[0, 4, 0, 4], [2, 2, 1, -3]]), table([[0, 4, -1, 4], [2, 2, 1, 3]]),
                  table([[2**31 - 1, 2, 0, 4], [2, 2, 1, 3]])]
    refused = [dict(pred_seg=None), dict(ref_seg=None), dict(host=None), dict(groups=None), dict(out_off=None), dict(G=-1),
               dict(n_pred=-1), dict(n_ref=-1), dict(n_pred=3), dict(n_ref=3)] + [dict(host=t.ctypes.data) for t in bad_tables]
    for over in refused + [dict(tious=None), dict(T=0), dict(T=ops.TIOU_MAX_T + 1), dict(strict=2), dict(strict=-1),
                           dict(pred_hits=None), dict(ref_first=None), dict(ld_pred=5), dict(ld_ref=6)]:
        assert lib.bmhrl_tiou_hits(*hits_args(**over)) == -22, over
    for over in refused + [dict(pair_off=None), dict(pair_ref=None), dict(n_slots=5), dict(n_slots=7), dict(n_pairs=-1)]:
        assert lib.bmhrl_tiou_pairs(*pairs_args(**over)) == -22, over
    assert lib.bmhrl_tiou_hits(*hits_args(G=0, host=None, groups=None, out_off=None)) == 0
    assert lib.bmhrl_tiou_pairs(*pairs_args(G=0, host=None, groups=None, out_off=None)) == 0
    torch.cuda.synchronize()
    assert (hits == SENTINEL).all() and (first == SENTINEL).all() and (rows == SENTINEL).all()     # nothing was launched
    # the same arguments without a fault are accepted
    assert lib.bmhrl_tiou_hits(*hits_args()) == 0 and lib.bmhrl_tiou_pairs(*pairs_args()) == 0
    torch.cuda.synchronize()
    assert (hits >= 0).all() and (first >= 0).all()
    # a pair_off that leaves a prediction no room, or points outside pair_ref, writes nothing there
    rows.fill_(SENTINEL)
    wild = torch.tensor([0, 1, 2, 6, 9, 12, -5], dtype=torch.int64, device=dev)
    assert lib.bmhrl_tiou_pairs(*pairs_args(pair_off=wild.data_ptr())) == 0
    torch.cuda.synchronize()
    assert rows.cpu().tolist() == [-1, -1, -1, SENTINEL, SENTINEL, SENTINEL]
