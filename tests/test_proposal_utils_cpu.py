"""bmhrl_amd.proposal_utils on CPU tensors against what the reference's utilities/proposal_utils.py returned
(tests/golden/proposals.json + proposals.npz, written by tests/golden/make_proposal_golden.py): exact, bit for bit."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from bmhrl_amd import proposal_utils as pu
from tests.proposal_reference import load_golden


def from_bits(hexed, *shape):
    a = np.array([int(hexed[i:i + 8], 16) for i in range(0, len(hexed), 8)], dtype=np.uint32).view(np.float32)
    return torch.from_numpy(a.reshape(shape).copy())


def same_bits(a, b):
    b = torch.from_numpy(b) if isinstance(b, np.ndarray) else b
    return a.shape == b.shape and np.array_equal(a.contiguous().numpy().view(np.uint32), b.contiguous().numpy().view(np.uint32))


@pytest.fixture(scope="module")
def golden():
    return load_golden()


def test_tiou_vectorized_reproduces_the_recorded_values(golden):
    assert len(golden["tiou"]) == 9
    for rec in golden["tiou"]:
        cols = 1 if rec["mode"] == "lengths" else 2
        a, b = from_bits(rec["a"], rec["M"], cols), from_bits(rec["b"], rec["N"], cols)
        kw = {"center_length": {}, "start_end": {"center_length": False}, "lengths": {"without_center_coords": True}}[rec["mode"]]
        assert same_bits(pu.tiou_vectorized(a, b, **kw), from_bits(rec["tiou"], rec["M"], rec["N"])), rec["mode"]


def test_postprocess_and_nms_reproduce_every_recorded_case(golden):
    batch = {"duration_in_secs": golden["durations"], "video_ids": golden["video_ids"]}
    assert len(golden["cases"]) == 30
    for case in golden["cases"]:
        N, k, thr = case["N"], case["k"], case["nms_tiou"]
        pred = torch.from_numpy(golden["inputs"][N])
        cfg = SimpleNamespace(max_prop_per_vid=k, nms_tiou_thresh=thr)
        post = pu.postprocess_preds(pred.clone(), cfg, batch)
        assert case["postprocessed"].shape == (3, case["k_eff"], 3) and same_bits(post, case["postprocessed"]), (N, k)
        if thr is not None:
            for v, rec in zip(post, case["nms"]):
                assert same_bits(pu.non_max_suppresion(v.clone(), thr), rec), (N, k, thr)


def test_anet_predictions_reproduce_every_recorded_case(golden):
    batch = {"duration_in_secs": golden["durations"], "video_ids": golden["video_ids"]}
    for case in golden["cases"]:
        pred = torch.from_numpy(golden["inputs"][case["N"]])
        cfg = SimpleNamespace(max_prop_per_vid=case["k"], nms_tiou_thresh=case["nms_tiou"])
        anet = pu.AnetPredictions(cfg, "val_1", 0)
        assert anet.add_new_predictions(pred.clone(), batch) == case["returned"]
        results = anet.predictions["results"]
        assert all(type(seg["proposal_score"]) is tuple and len(seg["proposal_score"]) == 1 for v in results.values() for seg in v)
        assert json.loads(json.dumps(results)) == case["results"]
        assert (anet.segments_used, anet.segments_total, anet.num_vid_w_no_props) == \
            (case["segments_used"], case["segments_total"], case["num_vid_w_no_props"])
    assert any(c["num_vid_w_no_props"] for c in golden["cases"])


def test_submission_file_has_the_reference_layout(golden, tmp_path):
    batch = {"duration_in_secs": golden["durations"], "video_ids": golden["video_ids"]}
    cfg = SimpleNamespace(max_prop_per_vid=5, nms_tiou_thresh=0.4, log_path=str(tmp_path))
    anet = pu.AnetPredictions(cfg, "val_1", 3)
    anet.add_new_predictions(torch.from_numpy(golden["inputs"][100]), batch)
    anet.write_anet_predictions_to_json()
    assert anet.submission_path == os.path.join(str(tmp_path), "submissions", "prop_results_val_1_e3_maxprop5.json")
    with open(anet.submission_path) as f:
        written = json.load(f)
    assert set(written) == {"version", "external_data", "results"} and written["version"] == "VERSION 1.0"
    seg = next(iter(written["results"].values()))[0]
    assert set(seg) == {"sentence", "proposal_score", "timestamp"} and seg["sentence"] == "" and len(seg["proposal_score"]) == 1
    with pytest.raises(NotImplementedError):
        pu.AnetPredictions(cfg, "val_2", 3).write_anet_predictions_to_json()


def test_equal_confidences_keep_their_row_order():
    pred = torch.tensor([[[5.0, 2.0, 0.5], [9.0, 2.0, 0.7], [1.0, 2.0, 0.5], [3.0, 2.0, 0.5]]])
    assert pu.select_topk_predictions(pred, 3)[0, :, 0].tolist() == [9.0, 5.0, 1.0]


def test_calculate_f1():
    assert pu.calculate_f1(0.5, 0.5) == pytest.approx(0.5, abs=1e-12)
    assert pu.calculate_f1(0.0, 0.0) == 0.0
    assert pu.calculate_f1(0.25, 0.75) == 2 * 0.25 * 0.75 / (0.25 + 0.75 + 1e-16)
    assert pu.add_dict_to_another_dict({"a": 1.0, "b": 2.0}, {"a": 0.5}) == {"a": 1.5, "b": 2.0}


def test_anchors_from_segments_is_deterministic_sorted_and_finds_separated_clusters():
    rng = np.random.default_rng(5)
    clusters = [rng.uniform(1.0, 2.0, 40), rng.uniform(20.0, 22.0, 25), rng.uniform(100.0, 105.0, 10)]
    lengths = np.concatenate(clusters)
    rng.shuffle(lengths)
    anchors = pu.anchors_from_segments(lengths, 3)
    assert anchors == pu.anchors_from_segments(list(lengths), 3) == sorted(anchors)
    assert anchors == pytest.approx([c.mean() for c in clusters], rel=1e-12)
    many = pu.anchors_from_segments(rng.uniform(0.5, 200.0, 500), 48)
    assert len(many) == 48 and many == sorted(many) and all(np.isfinite(many))
    with pytest.raises(ValueError):
        pu.anchors_from_segments([1.0, 2.0], 3)
