"""Soft-NMS without a GPU: proposal_utils.soft_nms against the numpy restatement of
tests/soft_nms_reference.py bit for bit, its hard mode against non_max_suppresion, a case worked by hand, the routing of
select_rows (a cfg without the new fields calls exactly what it called before) and the condition under which the Gaussian
cases may be compared bit for bit at all."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from bmhrl_amd import proposal_utils as pu
from tests import soft_nms_reference as R

CASES = R.cases()


def bits(a):
    a = a.detach().cpu().contiguous().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return np.atleast_1d(a).view(np.uint32)


def pool_rows(pred, durations, m):
    """what the piecewise route hands soft_nms: (B, m, 4) rows (start, end, conf, row index), confidence descending"""
    B, N, _ = pred.shape
    idx = np.broadcast_to(np.arange(N, dtype=np.float32).reshape(1, N, 1), (B, N, 1))
    t = torch.from_numpy(np.concatenate([pred, idx], axis=2))
    return pu.postprocess_preds(t, SimpleNamespace(max_prop_per_vid=min(m, N)), {"duration_in_secs": durations})


@pytest.mark.parametrize("name", list(CASES))
def test_soft_nms_equals_the_restatement_bit_for_bit(name):
    c = CASES[name]
    props, rows, count, well = R.expected(name)
    assert well
    pool = pool_rows(c["pred"], c["durations"], c["m"])
    for b, video in enumerate(pool):
        got = pu.soft_nms(video, c["method"], c["tiou_thresh"], c["sigma"], c["min_score"], k=c["k"])
        n = int(count[b])
        assert got.shape == (n, 4), (name, b)
        assert np.array_equal(bits(got[:, :3]), bits(props[b, :n])), (name, b)
        assert got[:, 3].tolist() == rows[b, :n].tolist(), (name, b)
        assert not bits(props[b, n:]).any() and (rows[b, n:] == -1).all()


def test_every_case_is_well_conditioned():
    """the condition of tests/soft_nms_reference.py holds for every shared case, so the GPU tests may demand equal bits"""
    assert len(CASES) >= 25
    assert all(R.expected(name)[3] for name in CASES)
    # and the condition can fail: a weight that lies on a rounding boundary of fp32 is reported
    boundary = float(np.float32(0.75)) + 2.0 ** -25         # exactly between two fp32 neighbours
    t = math.sqrt(-0.5 * math.log(boundary))
    near = np.nextafter(t, np.inf) - t                        # one step of t moves the weight by about a twentieth of the window
    assert any(not R.gaussian_weight(float(t + j * near), 0.5)[1] for j in range(-64, 65))


@pytest.mark.parametrize("thr", [0.0, 0.3, 0.5, 0.9])
def test_hard_equals_non_max_suppresion(thr):
    rng = np.random.default_rng(5)
    pred = R.random_pred(rng, 3, 400)
    pool = pool_rows(pred, R.D3, 150)
    for video in pool:
        want = pu.non_max_suppresion(video, thr)
        got = pu.soft_nms(video, "hard", thr, min_score=None)
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want))
        few = pu.soft_nms(video, "hard", thr, min_score=None, k=7)
        assert np.array_equal(bits(few), bits(want[:7]))


HAND = np.array([[[5, 10, .9], [5, 10, .8], [25, 10, .5]]], dtype=np.float32)       # [centre, length, confidence]


def hand(method, thr, min_score):
    video = pool_rows(HAND, [100.0], 3)[0]
    got = pu.soft_nms(video, method, thr, 0.5, min_score)
    want = R.soft_select(HAND, [100.0], 3, 3, method, thr, 0.5, min_score)
    n = int(want[2][0])
    assert np.array_equal(bits(got[:, :3]), bits(want[0][0, :n])) and got[:, 3].tolist() == want[1][0, :n].tolist()
    return got


def test_the_case_worked_by_hand():
    got = hand("hard", 0.5, None)
    assert got[:, 3].tolist() == [0, 2] and got[:, :3].tolist() == [[0.0, 10.0, HAND[0, 0, 2]], [20.0, 30.0, 0.5]]
    got = hand("linear", 0.5, 1e-3)                           # row 1: tIoU 1 with row 0, score 0.8 * (1 - 1) = 0 < 1e-3
    assert got[:, 3].tolist() == [0, 2]
    got = hand("gaussian", 0.0, 1e-3)                         # row 1: 0.8 * exp(-1 / 0.5), now behind row 2's 0.5
    assert got[:, 3].tolist() == [0, 2, 1]
    assert np.array_equal(bits(got[2, 2]), bits(np.float32(0.8) * np.float32(math.exp(-2.0))))
    assert np.array_equal(bits(got[1, 2]), bits(np.float32(0.5)))          # disjoint from the pick: the factor is exactly 1


@pytest.mark.parametrize("name", [n for n in CASES if "negative" not in n])
def test_emitted_scores_never_increase(name):
    props, rows, count, _ = R.expected(name)
    for b in range(props.shape[0]):
        s = props[b, :count[b], 2]
        assert (s[1:] <= s[:-1]).all(), (name, b)
        floor = CASES[name]["min_score"]
        assert floor is None or (s >= np.float32(floor)).all()


def test_duplicates_and_floor():
    props, rows, count, _ = R.expected("exact duplicates linear")
    # at most one of each four copies (the first: ties go to the smaller row): the others fell to exactly 0, below the floor
    assert ((count > 20) & (count <= 40)).all()
    for b in range(2):
        picked = rows[b, :count[b]].tolist()
        assert len({r // 4 for r in picked}) == len(picked) and all(r % 4 == 0 for r in picked)
    assert (R.expected("all below the floor")[2] == 0).all()
    assert (R.expected("no floor")[2] == 100).all()
    assert (R.expected("k < count")[2] == 10).all() and (R.expected("k > survivors")[2] < 200).all()


# ------------------------------------------------------------------------------------------------ select_rows
class Recorder:
    def __init__(self, result):
        self.calls, self.result = [], result

    def __call__(self, *args, **kwargs):
        self.calls.append((args, kwargs))
        return self.result


@pytest.mark.parametrize("extra", [{}, {"nms_method": None}, {"nms_method": "hard"}, {"nms_method": "hard", "nms_candidates": 100},
                                   {"nms_candidates": 50, "soft_nms_sigma": 0.1, "soft_nms_min_score": 0.5}])
def test_a_cfg_without_the_new_fields_takes_the_calls_it_took_before(monkeypatch, extra):
    cfg = SimpleNamespace(max_prop_per_vid=100, nms_tiou_thresh=0.4, **extra)
    assert pu.soft_nms_settings(cfg) is None
    batch = {"duration_in_secs": [50.0, 31.7]}
    host = torch.from_numpy(R.random_pred(np.random.default_rng(1), 2, 300))
    # host input: postprocess_preds(model_output, cfg, batch), then non_max_suppresion(video, threshold) per video
    post = pu.postprocess_preds(host.clone(), cfg, batch)
    rec_post, rec_nms, rec_soft = Recorder(post), Recorder(post[0, :2]), Recorder(None)
    monkeypatch.setattr(pu, "postprocess_preds", rec_post)
    monkeypatch.setattr(pu, "non_max_suppresion", rec_nms)
    monkeypatch.setattr(pu, "soft_nms", rec_soft)
    monkeypatch.setattr(pu, "soft_select_rows", rec_soft)
    rows, k = pu.select_rows(host, cfg, batch)
    assert k == 100 and rows == [post[0, :2].tolist()] * 2 and not rec_soft.calls
    assert len(rec_post.calls) == 1 and rec_post.calls[0][0][0] is host and rec_post.calls[0][0][1] is cfg \
        and rec_post.calls[0][0][2] is batch and not rec_post.calls[0][1]
    assert [(c[0][0].data_ptr(), c[0][1], c[1]) for c in rec_nms.calls] == [(post[b].data_ptr(), 0.4, {}) for b in range(2)]

    # device input: device_proposal_rows(model_output, durations, max_prop_per_vid, nms_tiou_thresh) and nothing else
    class OnDevice:
        is_cuda, shape = True, (2, 300, 3)
    rec_dev = Recorder(([[[0.0, 1.0, 0.5]]] * 2, 100))
    monkeypatch.setattr(pu, "device_proposal_rows", rec_dev)
    dev_input = OnDevice()
    assert pu.select_rows(dev_input, cfg, batch) == rec_dev.result and not rec_soft.calls and len(rec_post.calls) == 1
    assert rec_dev.calls == [((dev_input, batch["duration_in_secs"], 100, 0.4), {})]


def test_settings():
    base = dict(max_prop_per_vid=100, nms_tiou_thresh=None)
    s = pu.soft_nms_settings
    assert s(SimpleNamespace(**base, nms_method="gaussian")) == (100, 100, "gaussian", 0.0, 0.5, 1e-3)
    assert s(SimpleNamespace(**base, nms_method="linear", nms_candidates=400, soft_nms_sigma=0.3, soft_nms_min_score=0.01)) == \
        (100, 400, "linear", 0.0, 0.3, 0.01)
    assert s(SimpleNamespace(**base, nms_candidates=400)) == (100, 400, "hard", float("inf"), 0.5, None)
    assert s(SimpleNamespace(max_prop_per_vid=100, nms_tiou_thresh=0.4, nms_candidates=400, soft_nms_min_score=0.3)) == \
        (100, 400, "hard", 0.4, 0.5, None)
    with pytest.raises(ValueError):
        s(SimpleNamespace(**base, nms_method="median"))
    with pytest.raises(ValueError):
        s(SimpleNamespace(**base, nms_method="linear", nms_candidates=50))


@pytest.mark.parametrize("method,thr,m", [("gaussian", None, 256), ("linear", 0.5, 100), ("hard", 0.4, 256), ("hard", None, 256)])
def test_the_soft_route_for_host_input(method, thr, m):
    pred = R.random_pred(np.random.default_rng(3), 3, 600)
    cfg = SimpleNamespace(max_prop_per_vid=100, nms_tiou_thresh=thr, nms_method=method, nms_candidates=m)
    rows, k = pu.select_rows(torch.from_numpy(pred.copy()), cfg, {"duration_in_secs": R.D3})
    assert k == 100
    floor = None if method == "hard" else 1e-3
    eff = (float("inf") if method == "hard" else 0.0) if thr is None else thr
    props, _, count, well = R.soft_select(pred, R.D3, m, 100, method, eff, 0.5, floor)
    assert well
    for b in range(3):
        assert len(rows[b]) == count[b]
        assert np.array_equal(bits(np.array(rows[b], dtype=np.float32).reshape(-1, 3)), bits(props[b, :count[b]]))
    # N below the pool and below k: both are clipped, the second return value is min(k, N)
    small, k = pu.select_rows(torch.from_numpy(pred[:, :40].copy()), cfg, {"duration_in_secs": R.D3})
    assert k == 40 and all(len(v) <= 40 for v in small)


def test_anet_predictions_through_the_soft_route():
    pred = R.random_pred(np.random.default_rng(4), 2, 600)
    cfg = SimpleNamespace(max_prop_per_vid=100, nms_tiou_thresh=None, nms_method="gaussian", nms_candidates=256)
    anet = pu.AnetPredictions(cfg, "val_1", 0)
    anet.add_new_predictions(torch.from_numpy(pred.copy()), {"duration_in_secs": [50.0, 31.7], "video_ids": ["a", "b"]})
    props, _, count, _ = R.soft_select(pred, [50.0, 31.7], 256, 100, "gaussian", 0.0, 0.5, 1e-3)
    for b, vid in enumerate(("a", "b")):
        want = [(round(float(s), 5), round(float(e), 5), round(float(c), 5)) for s, e, c in props[b, :count[b]]]
        want = [w for w in want if w[1] - w[0] > 0.2]
        got = [(p["timestamp"][0], p["timestamp"][1], p["proposal_score"][0]) for p in anet.predictions["results"][vid]]
        assert got == want and len(got) > 0
    assert anet.segments_total == 200
