"""bmhrl_proposal_chain (bmhrl_amd/csrc/event_chain.hip) on the MI355X: events, chain, length and value
against the numpy restatement of tests/event_chain_reference.py, bit for bit, twice.  The cases are that module's: P = 1, 2,
3; 64 / 65 (the wave edge); 512 / 513 (a thread's second row); 1023 / 1024; count 0, below P with garbage and NaN rows behind
it, NULL, outside [0, P]; three videos with different counts, one with nothing eligible; L = 1, 32 and above the eligible
rows; equal scores, exact duplicates, equal starts with different ends; tau 0 with touching segments; tau 0.5 with lambda
0.3; nested segments; a cost above every score, NaN scores, every row shorter than min_length."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import event_chain_reference as R
from tests import soft_nms_reference as S

pytestmark = pytest.mark.gpu

CASES = R.cases()
CHAIN = dict(chain_max_events=6, chain_max_tiou=0.1, chain_overlap_weight=0.5, chain_event_cost=0.05)


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
    count = None if c["count"] is None else torch.from_numpy(c["count"]).to(dev)
    out = ops.proposal_chain(torch.from_numpy(c["props"]).to(dev), count, c["L"], c["max_tiou"], c["overlap_weight"],
                             c["event_cost"], c["min_length"])
    B = c["props"].shape[0]
    assert out[0].shape == (B, c["L"], 3) and out[1].shape == (B, c["L"]) and out[2].shape == out[3].shape == (B,)
    assert out[1].dtype == out[2].dtype == torch.int32 and out[0].dtype == out[3].dtype == torch.float32
    return [t.cpu().numpy() for t in out]


@pytest.mark.parametrize("name", list(CASES))
def test_equals_the_restatement_bit_for_bit(dev, name):
    want = R.expected(name)
    got = run(dev, CASES[name])
    assert np.array_equal(got[2], want[2]), (got[2], want[2])
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[3]), bits(want[3]))
    again = run(dev, CASES[name])
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, again))             # two runs, equal bits


def test_select_soft_and_chain_captured_together_replay_to_the_eager_result(dev):
    """as tests/test_soft_nms_gpu.py captures: on a side stream, after one eager call there; the chain reads the select
    call's device output with nothing between them"""
    from bmhrl_amd import ops
    pred_np = S.random_pred(np.random.default_rng(8), 2, 4097)
    pred = torch.from_numpy(pred_np).to(dev)
    dur = torch.tensor(S.D3[:2], dtype=torch.float32, device=dev)

    def call():
        props, _, count = ops.proposal_select_soft(pred, dur, 256, 100, "gaussian", 0.0, 0.5, 1e-3)
        return ops.proposal_chain(props, count, 10, 0.1, 0.5, 0.05)

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
    assert int(eager[2].min()) > 1
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(eager, out))
    props, _, count, well = S.soft_select(pred_np, S.D3[:2], 256, 100, "gaussian", 0.0, 0.5, 1e-3)
    want = R.chain_select(props, count, 10, 0.1, 0.5, 0.05)
    assert well and all(np.array_equal(bits(a), bits(b)) for a, b in zip(out, want))


def test_refusals_and_the_optional_pointers(dev):
    from bmhrl_amd import _lib, ops
    lib = _lib.load()
    B, P, L = 2, 16, 8
    props = torch.from_numpy(R.random_props(np.random.default_rng(5), B, P)).to(dev)
    count = torch.full((B,), 12, dtype=torch.int32, device=dev)
    events = torch.zeros(B, L, 3, device=dev)
    chain = torch.zeros(B, L, dtype=torch.int32, device=dev)
    length = torch.zeros(B, dtype=torch.int32, device=dev)
    value = torch.zeros(B, device=dev)
    nan, inf = float("nan"), float("inf")
    st = ops.stream()

    def call(props_p=props.data_ptr(), count_p=count.data_ptr(), B=B, P=P, L=L, tau=0.1, lam=0.5, cost=0.05, shortest=0.2,
             events_p=events.data_ptr(), chain_p=chain.data_ptr(), length_p=length.data_ptr(), value_p=value.data_ptr()):
        return lib.bmhrl_proposal_chain(props_p, count_p, B, P, L, tau, lam, cost, shortest, events_p, chain_p, length_p, value_p,
                                        st)

    assert call() == 0
    torch.cuda.synchronize()
    full = (events.clone(), chain.clone(), length.clone())
    want = R.chain_select(props.cpu().numpy(), count.cpu().numpy(), L, 0.1, 0.5, 0.05)
    assert np.array_equal(bits(events), bits(want[0])) and np.array_equal(bits(value), bits(want[3])) and int(length.min()) > 0
    events.zero_(), chain.zero_(), length.zero_()
    assert call(value_p=None) == 0                              # value is optional
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((events, chain, length), full))
    assert call(count_p=None) == 0                              # count NULL: all P rows
    torch.cuda.synchronize()
    assert np.array_equal(chain.cpu().numpy(), R.chain_select(props.cpu().numpy(), None, L, 0.1, 0.5, 0.05)[1])
    assert call(props_p=None) == -22 and call(events_p=None) == -22 and call(chain_p=None) == -22 and call(length_p=None) == -22
    assert call(B=0) == -22 and call(B=65536) == -22 and call(B=-1) == -22
    assert call(P=0) == -22 and call(P=1025) == -22 and call(P=-1) == -22
    assert call(L=0) == -22 and call(L=33) == -22 and call(L=-1) == -22
    for name in ("tau", "lam", "cost", "shortest"):
        assert call(**{name: nan}) == -22 and call(**{name: -1e-6}) == -22 and call(**{name: -inf}) == -22, name
    assert call(tau=0.0, lam=0.0, cost=0.0, shortest=0.0) == 0 and call(tau=inf) == 0
    torch.cuda.synchronize()
    # and through ops: the checked call path reports the library's refusal
    for kwargs in (dict(max_events=0), dict(max_events=33), dict(max_tiou=nan), dict(max_tiou=-0.5), dict(overlap_weight=nan),
                   dict(overlap_weight=-1.0), dict(event_cost=nan), dict(event_cost=-1.0), dict(min_length=nan),
                   dict(min_length=-0.2)):
        args = dict(max_events=8)
        args.update(kwargs)
        with pytest.raises(_lib.HipError, match="bmhrl_proposal_chain failed: invalid argument -22"):
            ops.proposal_chain(props, count, **args)
    with pytest.raises(_lib.HipError):
        ops.proposal_chain(torch.zeros(1, 1025, 3, device=dev), None, 4)
    for bad in (lambda: ops.proposal_chain(props[:, :, :2], count, 4), lambda: ops.proposal_chain(props.double(), count, 4),
                lambda: ops.proposal_chain(props, count.long(), 4), lambda: ops.proposal_chain(props, count[:1], 4),
                lambda: ops.proposal_chain(props.transpose(0, 1), count, 4)):
        with pytest.raises(ValueError):
            bad()
    assert ops.PROPOSAL_CHAIN_MAX_P == 1024 and ops.PROPOSAL_CHAIN_MAX_L == 32
    torch.cuda.synchronize()


@pytest.mark.parametrize("extra", [dict(nms_tiou_thresh=0.4), dict(nms_tiou_thresh=None, nms_method="gaussian", nms_candidates=256)])
def test_select_rows_with_a_chain_on_device_input_equals_the_host_copy(dev, extra):
    from bmhrl_amd import ops, proposal_utils as pu
    cfg = SimpleNamespace(max_prop_per_vid=100, **extra, **CHAIN)
    output = torch.from_numpy(S.random_pred(np.random.default_rng(21), 2, 600)).to(dev)
    batch = {"duration_in_secs": [50.0, 31.7], "video_ids": ["v_a", "v_b"]}
    calls = []
    real = ops.proposal_chain
    try:
        ops.proposal_chain = lambda *a, **kw: calls.append(1) or real(*a, **kw)
        on_device, k_dev = pu.select_rows(output, cfg, batch)
        on_host, k_host = pu.select_rows(output.cpu(), cfg, batch)
    finally:
        ops.proposal_chain = real
    assert len(calls) == 1                                      # the device input took the kernel, the host copy did not
    assert k_dev == k_host == 100
    assert [bits(np.array(v, dtype=np.float32)).tolist() for v in on_device] == \
        [bits(np.array(v, dtype=np.float32)).tolist() for v in on_host]
    assert all(1 <= len(v) <= 6 and v == sorted(v) for v in on_device)
    a, b = pu.AnetPredictions(cfg, "val_1", 0), pu.AnetPredictions(cfg, "val_1", 0)
    assert a.add_new_predictions(output, batch) == b.add_new_predictions(output.cpu(), batch) and a.predictions == b.predictions


def test_chain_predictions_on_the_device_equals_the_host_route(dev):
    from bmhrl_amd import proposal_utils as pu
    props = R.random_props(np.random.default_rng(9), 3, 40)
    props[1, :, 2] = 0.01                                       # ends with no events
    sub = {"results": {f"v_{b}": [{"sentence": "", "proposal_score": (float(c),), "timestamp": [float(s), float(e)]}
                                  for s, e, c in props[b, :40 - 9 * b]] for b in range(3)}}
    cfg = SimpleNamespace(**CHAIN)
    out = pu.chain_predictions(sub, cfg, device=dev)
    assert out == pu.chain_predictions(sub, cfg) and list(out["results"]) == ["v_0", "v_2"]
