"""bmhrl_proposal_select_soft (bmhrl_amd/csrc/proposal.hip) on the MI355X: props, rows and count against
the numpy restatement of tests/soft_nms_reference.py, bit for bit.  The cases are that module's: N = 1 and 3; N = 64 / 65 (the
wave edge of the pool); N = 4096 / 4097 (the chunk edge, the first case with a pass); N = 2 * 4096 + 5 with m = 1024 (passes
that keep more than 128 keys per chunk); m = 513 / 1023 (a ragged second row per thread); k below the count and above the
survivors; three durations, one so short that trimmed segments are empty; equal confidences, exact duplicates, everything
below the floor, no floor, thresholds 0 and 0.5.  Equal bits may be demanded of the Gaussian cases because every one of
them is well conditioned (tests/test_soft_nms_cpu.py asserts it)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import soft_nms_reference as R

pytestmark = pytest.mark.gpu

CASES = R.cases()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bmhrl_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def bits(t):
    return (t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)).view(np.uint32)


def run(dev, c):
    from bmhrl_amd import ops
    props, rows, count = ops.proposal_select_soft(torch.from_numpy(c["pred"]).to(dev),
                                                  torch.tensor(c["durations"], dtype=torch.float32, device=dev), c["m"], c["k"],
                                                  c["method"], c["tiou_thresh"], c["sigma"], c["min_score"])
    assert props.shape == (c["pred"].shape[0], c["k"], 3) and rows.dtype == count.dtype == torch.int32
    return props.cpu().numpy(), rows.cpu().numpy(), count.cpu().numpy()


@pytest.mark.parametrize("name", list(CASES))
def test_equals_the_restatement_bit_for_bit(dev, name):
    c = CASES[name]
    want_props, want_rows, want_count, well = R.expected(name)
    assert well
    props, rows, count = run(dev, c)
    assert np.array_equal(count, want_count), (count, want_count)
    assert np.array_equal(rows, want_rows)
    assert np.array_equal(bits(props), bits(want_props))
    # the corners are the trimmed corners of pred[rows], zeros and -1 stand behind the picks
    for b in range(props.shape[0]):
        n, dur = int(count[b]), np.float32(c["durations"][b])
        picked = c["pred"][b, rows[b, :n]]
        start, end = picked[:, 0] - picked[:, 1] / np.float32(2), picked[:, 0] + picked[:, 1] / np.float32(2)
        assert np.array_equal(bits(props[b, :n, 0]), bits(np.minimum(np.maximum(start, np.float32(0)), dur)))
        assert np.array_equal(bits(props[b, :n, 1]), bits(np.minimum(end, dur)))
        assert len(set(rows[b, :n].tolist())) == n
        assert not bits(props[b, n:]).any() and (rows[b, n:] == -1).all()
    again = run(dev, c)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip((props, rows, count), again))          # two runs, equal bits


@pytest.mark.parametrize("N,k,thr", [(300, 100, 0.4), (8197, 128, 0.5), (65, 64, 0.0), (4097, 1, 0.7)])
def test_hard_with_the_pool_equal_to_k_is_proposal_select(dev, N, k, thr):
    from bmhrl_amd import ops
    pred = torch.from_numpy(R.random_pred(np.random.default_rng(N), 3, N)).to(dev)
    dur = torch.tensor(R.D3, dtype=torch.float32, device=dev)
    want_props, want_count = ops.proposal_select(pred, dur, k, thr)
    props, rows, count = ops.proposal_select_soft(pred, dur, k, k, "hard", thr)
    assert torch.equal(count, want_count) and np.array_equal(bits(props), bits(want_props))
    by_number = ops.proposal_select_soft(pred, dur, k, k, 0, thr)
    assert all(torch.equal(a, b) for a, b in zip((props, rows, count), by_number))


def test_one_captured_call_replays_to_the_eager_result(dev):
    """as tests/bench_proposals.py::timed captures: on a side stream, after one eager call there"""
    from bmhrl_amd import ops
    pred = torch.from_numpy(R.random_pred(np.random.default_rng(8), 2, 4097)).to(dev)
    dur = torch.tensor(R.D3[:2], dtype=torch.float32, device=dev)
    call = lambda: ops.proposal_select_soft(pred, dur, 256, 100, "gaussian", 0.0, 0.5, 1e-3)
    eager = [t.clone() for t in call()]
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
        with torch.cuda.graph(g):
            out = call()
    torch.cuda.current_stream().wait_stream(s)
    for t in out:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert int(eager[2].min()) > 0
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(eager, out))
    want = R.soft_select(pred.cpu().numpy(), R.D3[:2], 256, 100, "gaussian", 0.0, 0.5, 1e-3)
    assert want[3] and np.array_equal(bits(out[0]), bits(want[0])) and np.array_equal(out[1].cpu().numpy(), want[1])


def test_refusals_and_the_optional_rows(dev):
    from bmhrl_amd import _lib, ops
    lib = _lib.load()
    pred = torch.rand(2, 16, 3, device=dev)
    dur = torch.full((2,), 10.0, device=dev)
    props = torch.zeros(2, 8, 3, device=dev)
    rows = torch.zeros(2, 8, dtype=torch.int32, device=dev)
    count = torch.zeros(2, dtype=torch.int32, device=dev)
    nan, inf = float("nan"), float("inf")
    st = ops.stream()

    def call(pred_p=pred.data_ptr(), B=2, N=16, dur_p=dur.data_ptr(), m=8, k=8, method=2, thr=0.5, sigma=0.5, floor=-inf,
             props_p=props.data_ptr(), rows_p=rows.data_ptr(), count_p=count.data_ptr(), ws_p=None, ws_n=0):
        return lib.bmhrl_proposal_select_soft(pred_p, B, N, dur_p, m, k, method, thr, sigma, floor, props_p, rows_p, count_p,
                                              ws_p, ws_n, st)

    assert call() == 0
    with_rows = (props.clone(), count.clone())
    props.zero_(), count.zero_()
    assert call(rows_p=None) == 0                               # rows is optional
    assert np.array_equal(bits(props), bits(with_rows[0])) and torch.equal(count, with_rows[1]) and int(count.min()) > 0
    assert call(pred_p=None) == -22 and call(dur_p=None) == -22 and call(props_p=None) == -22 and call(count_p=None) == -22
    assert call(B=0) == -22 and call(B=65536) == -22 and call(N=0) == -22 and call(N=(1 << 24) + 1) == -22
    assert call(m=0, k=1) == -22 and call(m=1025, k=8) == -22 and call(k=0) == -22 and call(k=9) == -22
    assert call(method=3) == -22 and call(method=-1) == -22
    assert call(thr=nan) == -22 and call(floor=nan) == -22
    assert call(sigma=0.0) == -22 and call(sigma=-1.0) == -22 and call(sigma=nan) == -22
    assert call(method=1, sigma=0.0) == 0 and call(method=0, sigma=nan) == 0       # sigma belongs to the Gaussian method only
    assert call(thr=inf) == 0 and call(floor=-inf) == 0
    # more than one chunk needs the workspace: 2 chunks of 5000 rows keep m = 8 keys each, for B = 2 videos
    big = torch.rand(2, 5000, 3, device=dev)
    ws = torch.zeros(2 * ops.proposal_select_workspace(5000, 8), dtype=torch.int64, device=dev)
    assert ws.numel() >= 2 * 2 * 8
    assert call(N=5000, pred_p=big.data_ptr()) == -22
    assert call(N=5000, pred_p=big.data_ptr(), ws_p=ws.data_ptr(), ws_n=2 * 2 * 8 - 1) == -22
    assert call(N=5000, pred_p=big.data_ptr(), ws_p=ws.data_ptr(), ws_n=ws.numel()) == 0
    torch.cuda.synchronize()
    # and through ops: the checked call path reports the library's refusal
    for kwargs in (dict(m=0, k=1), dict(m=1025, k=8), dict(k=0), dict(k=9), dict(method=3), dict(tiou_thresh=nan),
                   dict(method="gaussian", sigma=0.0), dict(min_score=nan)):
        args = dict(m=8, k=8, method="linear", tiou_thresh=0.5, sigma=0.5, min_score=None)
        args.update(kwargs)
        with pytest.raises(_lib.HipError, match="bmhrl_proposal_select_soft failed: invalid argument -22"):
            ops.proposal_select_soft(pred, dur, **args)
    with pytest.raises(ValueError):
        ops.proposal_select_soft(pred, dur, 8, 8, "median")
    torch.cuda.synchronize()


def test_anet_predictions_device_route_equals_the_piecewise_route(dev):
    from bmhrl_amd import proposal_utils as pu
    cfg = SimpleNamespace(max_prop_per_vid=100, nms_tiou_thresh=None, nms_method="gaussian", nms_candidates=256)
    output = torch.from_numpy(R.random_pred(np.random.default_rng(21), 2, 600)).to(dev)
    batch = {"duration_in_secs": [50.0, 31.7], "video_ids": ["v_a", "v_b"]}
    on_device, on_host = pu.AnetPredictions(cfg, "val_1", 0), pu.AnetPredictions(cfg, "val_1", 0)
    calls = []
    from bmhrl_amd import ops
    real = ops.proposal_select_soft
    try:
        ops.proposal_select_soft = lambda *a, **kw: calls.append(1) or real(*a, **kw)
        w_dev = on_device.add_new_predictions(output, batch)
        w_host = on_host.add_new_predictions(output.cpu(), batch)
    finally:
        ops.proposal_select_soft = real
    assert len(calls) == 1                                      # the device input took the kernel, the host copy did not
    assert on_device.predictions == on_host.predictions and w_dev == w_host
    props, _, count, _ = R.soft_select(output.cpu().numpy(), batch["duration_in_secs"], 256, 100, "gaussian", 0.0, 0.5, 1e-3)
    for b, v in enumerate(batch["video_ids"]):                  # and both are the restatement's picks, rounded and filtered
        want = [[round(float(s), 5), round(float(e), 5)] for s, e, _ in props[b, :count[b]]]
        want = [w for w in want if w[1] - w[0] > 0.2]
        assert [p["timestamp"] for p in on_device.predictions["results"][v]] == want and len(want) > 0
    assert (on_device.segments_total, on_device.segments_used) == (on_host.segments_total, on_host.segments_used)
