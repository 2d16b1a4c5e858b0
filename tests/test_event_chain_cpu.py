"""Event-chain selection without a GPU: proposal_utils.event_chain against the numpy restatement of
tests/event_chain_reference.py bit for bit, the restatement against the enumeration of every chain of small tables, a case
worked by hand, the properties of a chain, chain_settings, the routing of select_rows (a cfg without the new fields calls
exactly what it called before) and chain_predictions."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from bmhrl_amd import proposal_utils as pu
from tests import event_chain_reference as R
from tests import soft_nms_reference as S

CASES = R.cases()
f = np.float32


def bits(a):
    a = a.detach().cpu().contiguous().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return np.atleast_1d(a).view(np.uint32)


def settings(c):
    return c["L"], c["max_tiou"], c["overlap_weight"], c["event_cost"], c["min_length"]


@pytest.mark.parametrize("name", list(CASES))
def test_event_chain_equals_the_restatement_bit_for_bit(name):
    c = CASES[name]
    events, chain, length, value = R.expected(name)
    P = c["props"].shape[1]
    for b in range(c["props"].shape[0]):
        cnt = P if c["count"] is None else min(max(int(c["count"][b]), 0), P)
        rows, index, v = pu.event_chain(torch.from_numpy(c["props"][b, :cnt]), *settings(c))
        n = int(length[b])
        assert index == chain[b, :n].tolist(), (name, b)
        assert rows.shape == (n, 3) and np.array_equal(bits(rows), bits(events[b, :n])), (name, b)
        assert np.array_equal(bits(f(v)), bits(value[b])) and f(v) == v, (name, b)
        assert not bits(events[b, n:]).any() and (chain[b, n:] == -1).all()


# ------------------------------------------------------------------------------------------------ every chain of a small table
def enumerate_chains(g, t, allowed, lam, L):
    """(optimum, its chain) over every chain of positions that obeys the links, in float64 on the fp32 tables"""
    n = len(g)
    best = (-np.inf, [])

    def grow(chain, total):
        nonlocal best
        if total > best[0]:
            best = (total, list(chain))
        if len(chain) == L:
            return
        last = chain[-1]
        for j in range(last + 1, n):
            if allowed[last, j]:
                chain.append(j)
                grow(chain, total - lam * float(t[last, j]) + float(g[j]))
                chain.pop()

    for j in range(n):
        grow([j], float(g[j]))
    return best


def in_float64(rows, picked, lam, cost):
    total = 0.0
    for a, i in enumerate(picked):
        total += float(rows[i, 2] - f(cost))
        if a:
            p = rows[picked[a - 1]]
            total -= float(f(lam)) * float(R.tiou_with(p[0], p[1], rows[i, 0], rows[i, 1]))
    return total


def test_the_restatement_finds_the_optimum_of_small_tables():
    """300 random tables of at most 10 rows.  overlap_weight 0 with scores and cost on a grid of 1/64: every sum is exact
    and the value IS the enumerated optimum.  Otherwise three roundings per level on magnitudes of at most L * max score
    (+ overlap_weight for the penalty): |value - optimum| <= 3 L 2^-24 (L max score + overlap_weight)."""
    rng = np.random.default_rng(36)
    exact = 0
    for trial in range(300):
        n, L = int(rng.integers(1, 11)), int(rng.integers(1, 6))
        rows = R.random_props(rng, 1, n, dur=25.0, longest=8.0, grid=0.25 if trial % 2 else None)[0]
        tau = float(rng.choice([0.0, 0.1, 0.3, 0.6, 1.0]))
        on_grid = trial % 3 == 0
        lam = 0.0 if on_grid else float(rng.choice([0.1, 0.5, 1.0, 2.0]))
        cost = float(rng.choice([0.0, 0.125, 0.25]))
        if on_grid:
            exact += 1
            rows[:, 2] = rng.integers(1, 65, n) / 64.0
        picked, value = R.chain_of(rows, n, L, tau, lam, cost, 0.2)
        idx, g = R.eligible_in_order(rows, n, cost, 0.2)
        if len(idx) == 0:
            assert picked == [] and value == 0
            continue
        t, allowed = R.link_tables(rows, idx, tau)
        optimum, chain = enumerate_chains(g, t, allowed, float(f(lam)), L)
        bound = 3 * L * 2.0 ** -24 * (L * float(rows[:, 2].max()) + lam)
        if on_grid:
            assert float(value) == optimum, (trial, value, optimum)
            assert picked == [int(idx[j]) for j in chain] or in_float64(rows, picked, lam, cost) == optimum
        else:
            assert abs(float(value) - optimum) <= bound, (trial, value, optimum, bound)
        assert abs(in_float64(rows, picked, lam, cost) - float(value)) <= bound, (trial, picked)
        assert 1 <= len(picked) <= L
    assert exact == 100


# ------------------------------------------------------------------------------------------------ by hand
#                  A             B              C               D (inside A: starts later, ends earlier -- never linked to A)
HAND = np.array([[0, 10, .9], [5, 15, .8], [10, 20, .7], [2, 8, .95]], dtype=np.float32)


def hand(L, tau, lam, cost):
    rows, index, value = pu.event_chain(torch.from_numpy(HAND), L, tau, lam, cost)
    want, want_value = R.chain_of(HAND, 4, L, tau, lam, cost, 0.2)
    assert index == want and np.array_equal(bits(f(value)), bits(want_value)) and np.array_equal(bits(rows), bits(HAND[index]))
    return index, f(value)


def test_the_case_worked_by_hand():
    # order A D B C; gains .8 .85 .7 .6; tIoU: A-B 5/15, D-B 3/13, B-C 5/15, A-C = D-C = 0
    gA, gB, gC, gD = (f(x) - f(.1) for x in (f(.9), f(.8), f(.7), f(.95)))
    tDB, tBC = f(3) / (f(13) + f(1e-8)), f(5) / (f(15) + f(1e-8))
    index, value = hand(3, 0.4, 0.5, 0.1)                   # D B C 1.868 beats A B C 1.767 and D C 1.45
    assert index == [3, 1, 2]
    assert np.array_equal(bits(value), bits(((((gD - f(.5) * tDB) + gB) - f(.5) * tBC) + gC)))
    assert abs(float(value) - (.85 - .5 * 3 / 13 + .7 - .5 / 3 + .6)) < 1e-6
    index, value = hand(3, 0.3, 0.5, 0.1)                   # 1/3 > 0.3 bars A-B and B-C: D C 1.45 beats D B 1.435 and A C 1.4
    assert index == [3, 2] and np.array_equal(bits(value), bits(gD + gC))
    index, value = hand(2, 0.4, 0.5, 0.1)                   # two events: D C again
    assert index == [3, 2]
    index, value = hand(1, 0.4, 0.5, 0.1)
    assert index == [3] and np.array_equal(bits(value), bits(gD))
    index, value = hand(3, 0.4, 0.5, 0.9)                   # .9f - .9f is no gain: D alone is eligible
    assert index == [3] and np.array_equal(bits(value), bits(f(.95) - f(.9)))
    index, value = hand(3, 0.4, 0.5, 0.95)
    assert index == [] and value == 0
    index, value = hand(3, 0.4, 5.0, 0.1)                   # a heavy penalty: the disjoint pair
    assert index == [3, 2]


# ------------------------------------------------------------------------------------------------ properties
@pytest.mark.parametrize("name", list(CASES))
def test_a_chain_has_the_properties_of_the_definition(name):
    c = CASES[name]
    events, chain, length, value = R.expected(name)
    P = c["props"].shape[1]
    for b in range(events.shape[0]):
        n = int(length[b])
        cnt = P if c["count"] is None else min(max(int(c["count"][b]), 0), P)
        e, idx = events[b, :n], chain[b, :n].tolist()
        assert n <= c["L"] and len(set(idx)) == n and all(0 <= i < cnt for i in idx)
        assert np.array_equal(bits(e), bits(c["props"][b, idx]))
        assert (e[1:, 0] >= e[:-1, 0]).all() and (e[1:, 1] >= e[:-1, 1]).all()
        assert (R.tiou_with(e[:-1, 0], e[:-1, 1], e[1:, 0], e[1:, 1]) <= f(c["max_tiou"])).all()
        assert (e[:, 2] > f(c["event_cost"])).all() and ((e[:, 1] - e[:, 0]) > f(c["min_length"])).all()
        assert (n == 0) == (len(R.eligible_in_order(c["props"][b], cnt, c["event_cost"], c["min_length"])[0]) == 0)
        assert value[b] > 0 if n else value[b] == 0


def test_what_the_cases_are_there_for():
    length = {name: R.expected(name)[2] for name in CASES}
    assert len(CASES) >= 25
    for name in ("count 0", "cost above every score", "every row shorter than min_length"):
        assert (length[name] == 0).all(), name
    assert length["per-video counts"][1] == 0 and (length["per-video counts"][[0, 2]] > 0).all()
    assert length["counts outside [0, P]"][0] == 0 and (length["counts outside [0, P]"][1:] > 0).all()
    assert (length["nested segments never link"] == 1).all()
    assert (length["tau 0, touching segments"] == 20).all()
    assert (length["P=1024 L=1"] == 1).all() and (length["P=1024 L=32"] > 16).all()
    assert (length["L above the eligible rows"] <= 6).all() and (length["L above the eligible rows"] > 1).all()
    assert (length["garbage and NaN behind count"] > 0).all()
    for b in range(2):                                      # of three copies of a row the first is the one a chain holds
        picked = R.expected("exact duplicates")[1][b, :length["exact duplicates"][b]]
        assert (picked % 3 == 0).all() and len(picked) > 1
    chain = R.expected("exact duplicates tau 1")[1]
    assert any(a // 3 == b // 3 for a, b in zip(chain[0, :-1], chain[0, 1:]) if b >= 0)     # with tau 1 copies do link


# ------------------------------------------------------------------------------------------------ settings and routing
def test_chain_settings():
    s = pu.chain_settings
    base = dict(max_prop_per_vid=100, nms_tiou_thresh=0.4)
    assert s(SimpleNamespace(**base)) is None and s(SimpleNamespace(**base, chain_max_events=None)) is None
    assert s(SimpleNamespace(**base, chain_max_tiou=0.3, chain_event_cost=0.1)) is None       # chain_max_events switches it on
    assert s(SimpleNamespace(**base, chain_max_events=10)) == (10, 0.0, 0.0, 0.0, 0.2)
    assert s(SimpleNamespace(**base, chain_max_events=32, chain_max_tiou=0.1, chain_overlap_weight=0.5, chain_event_cost=0.05,
                             chain_min_length=0.0)) == (32, 0.1, 0.5, 0.05, 0.0)
    for bad in (dict(chain_max_events=0), dict(chain_max_events=33), dict(chain_max_events=-1), dict(chain_max_events=2.5),
                dict(chain_max_events=5, chain_max_tiou=-0.1), dict(chain_max_events=5, chain_overlap_weight=float("nan")),
                dict(chain_max_events=5, chain_event_cost=-1.0), dict(chain_max_events=5, chain_min_length=float("nan"))):
        with pytest.raises(ValueError):
            s(SimpleNamespace(**base, **bad))
    with pytest.raises(ValueError):
        pu.event_chain(torch.zeros(3, 3), 0)
    with pytest.raises(ValueError):
        pu.event_chain(torch.zeros(3, 3), 5, max_tiou=-1.0)


class Recorder:
    def __init__(self, result):
        self.calls, self.result = [], result

    def __call__(self, *args, **kwargs):
        self.calls.append((args, kwargs))
        return self.result


class OnDevice:
    is_cuda, shape = True, (2, 300, 3)


CHAIN = dict(chain_max_events=6, chain_max_tiou=0.1, chain_overlap_weight=0.5, chain_event_cost=0.05)


@pytest.mark.parametrize("chain", [{}, CHAIN])
def test_a_cfg_without_the_chain_fields_takes_the_calls_it_took_before(monkeypatch, chain):
    """with them the same calls carry one more keyword, `chain`"""
    batch = {"duration_in_secs": [50.0, 31.7]}
    extra = {"chain": pu.chain_settings(SimpleNamespace(**chain))} if chain else {}
    rec_dev, rec_soft = Recorder(([[[0.0, 1.0, 0.5]]] * 2, 100)), Recorder(([[[0.0, 2.0, 0.25]]] * 2, 100))
    rec_chain = Recorder(None)
    monkeypatch.setattr(pu, "device_proposal_rows", rec_dev)
    monkeypatch.setattr(pu, "soft_select_rows", rec_soft)
    dev_input = OnDevice()
    hard = SimpleNamespace(max_prop_per_vid=100, nms_tiou_thresh=0.4, **chain)
    assert pu.select_rows(dev_input, hard, batch) == rec_dev.result
    assert rec_dev.calls == [((dev_input, batch["duration_in_secs"], 100, 0.4), extra)] and not rec_soft.calls
    soft = SimpleNamespace(max_prop_per_vid=100, nms_tiou_thresh=None, nms_method="gaussian", nms_candidates=256, **chain)
    assert pu.select_rows(dev_input, soft, batch) == rec_soft.result
    assert rec_soft.calls == [((dev_input, batch["duration_in_secs"], 100, 256, "gaussian", 0.0, 0.5, 1e-3), extra)]
    assert len(rec_dev.calls) == 1
    if not chain:                                           # and on host input event_chain is not called at all
        monkeypatch.undo()
        monkeypatch.setattr(pu, "event_chain", rec_chain)
        host = torch.from_numpy(S.random_pred(np.random.default_rng(1), 2, 300))
        pu.select_rows(host.clone(), hard, batch)
        pu.select_rows(host.clone(), soft, batch)
        assert not rec_chain.calls


@pytest.mark.parametrize("extra", [dict(nms_tiou_thresh=0.4), dict(nms_tiou_thresh=None),
                                   dict(nms_tiou_thresh=None, nms_method="gaussian", nms_candidates=256),
                                   dict(nms_tiou_thresh=0.5, nms_method="linear"),
                                   dict(nms_tiou_thresh=0.4, nms_candidates=256)])
def test_the_chain_on_host_input_is_event_chain_of_the_old_result(extra):
    pred = S.random_pred(np.random.default_rng(3), 3, 600)
    batch = {"duration_in_secs": S.D3}
    old, k_old = pu.select_rows(torch.from_numpy(pred.copy()), SimpleNamespace(max_prop_per_vid=100, **extra), batch)
    new, k_new = pu.select_rows(torch.from_numpy(pred.copy()), SimpleNamespace(max_prop_per_vid=100, **extra, **CHAIN), batch)
    assert k_new == k_old == 100
    for b in range(3):
        rows = np.array(old[b], dtype=np.float32).reshape(-1, 3)
        want, _ = R.chain_of(rows, len(rows), 6, 0.1, 0.5, 0.05, 0.2)
        assert np.array_equal(bits(np.array(new[b], dtype=np.float32).reshape(-1, 3)), bits(rows[want]))
        assert new[b] == pu.event_chain(torch.tensor(old[b], dtype=torch.float32).reshape(-1, 3), 6, 0.1, 0.5, 0.05)[0].tolist()
    assert 1 <= len(new[0]) <= 6 and len(new[1]) >= 1
    small, k = pu.select_rows(torch.from_numpy(pred[:, :40].copy()), SimpleNamespace(max_prop_per_vid=100, **extra, **CHAIN), batch)
    assert k == 40                                          # the second return value stays min(k, N)


def test_anet_predictions_with_a_chain():
    pred = S.random_pred(np.random.default_rng(4), 2, 600)
    cfg = SimpleNamespace(max_prop_per_vid=100, nms_tiou_thresh=None, nms_method="gaussian", nms_candidates=256, **CHAIN)
    anet = pu.AnetPredictions(cfg, "val_1", 0)
    anet.add_new_predictions(torch.from_numpy(pred.copy()), {"duration_in_secs": [50.0, 31.7], "video_ids": ["a", "b"]})
    props, _, count, _ = S.soft_select(pred, [50.0, 31.7], 256, 100, "gaussian", 0.0, 0.5, 1e-3)
    for b, vid in enumerate(("a", "b")):
        picked, _ = R.chain_of(props[b], count[b], 6, 0.1, 0.5, 0.05, 0.2)
        want = [[round(float(s), 5), round(float(e), 5)] for s, e, _ in props[b, picked]]
        got = [p["timestamp"] for p in anet.predictions["results"][vid]]
        assert got == want and 1 <= len(got) <= 6 and got == sorted(got)
    assert anet.segments_total == 200


# ------------------------------------------------------------------------------------------------ chain_predictions
def submission_of(props, names):
    results = {}
    for b, vid in enumerate(names):
        results[vid] = [{"sentence": f"{vid} {i}", "proposal_score": (float(c),) if i % 2 else [float(c)], "timestamp": [float(s), float(e)]}
                        for i, (s, e, c) in enumerate(props[b])]
    return {"version": "VERSION 1.0", "external_data": {"used": True, "details": ""}, "results": results}


def test_chain_predictions():
    rng = np.random.default_rng(9)
    props = R.random_props(rng, 4, 40)
    props[2, :, 2] = 0.01                                   # every score of v_c below the cost: it ends with no events
    sub = submission_of(props, ["v_a", "v_b", "v_c", "v_d"])
    sub["results"]["v_d"] = sub["results"]["v_d"][:7]       # a ragged table
    sub["results"]["v_e"] = []
    before = copy.deepcopy(sub)
    cfg = SimpleNamespace(**CHAIN)
    out = pu.chain_predictions(sub, cfg)
    assert sub == before and out is not sub                 # the input is not touched
    assert {k: v for k, v in out.items() if k != "results"} == {k: v for k, v in sub.items() if k != "results"}
    assert list(out["results"]) == ["v_a", "v_b", "v_d"]
    for b, vid in ((0, "v_a"), (1, "v_b"), (3, "v_d")):
        n = len(sub["results"][vid])
        picked, _ = R.chain_of(props[b, :n], n, 6, 0.1, 0.5, 0.05, 0.2)
        assert out["results"][vid] == [sub["results"][vid][i] for i in picked] and 1 <= len(picked) <= 6
        assert all(x is y for x, y in zip(out["results"][vid], (sub["results"][vid][i] for i in picked)))
    assert pu.chain_predictions(sub, pu.chain_settings(cfg)) == out                     # the settings themselves
    assert pu.chain_predictions(sub, cfg, device="cpu") == out
    assert pu.chain_predictions({"results": {}}, cfg) == {"results": {}}
    with pytest.raises(ValueError):
        pu.chain_predictions(sub, SimpleNamespace(max_prop_per_vid=100))
