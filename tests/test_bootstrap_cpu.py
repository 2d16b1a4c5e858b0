"""The bootstrap over videos on the host: evaluate.bootstrap_ratios_host against the plain-loop
restatement (tests/bootstrap_reference.py) bit for bit, the exact properties of the counts, row 0 against np.mean, the
soundness of the draw, summarize's indices worked by hand, bootstrap / compare on stand-in evaluators whose device is the CPU, and a real
DenseCaptionEvaluator with device="cpu" behind tests/test_soda_cpu.py's stand-ins for the device score calls: .scores with
and without bootstrap=, .per_video against .scores, .intervals.  The paragraph family needs the device
(tests/test_bootstrap_gpu.py)."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

from tests import bootstrap_reference as br


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name", list(br.CASES))
def test_host_equals_the_restatement_bit_for_bit(name):
    from bmhrl_amd.evaluate import bootstrap_ratios_host
    c = br.CASES[name]
    got = bootstrap_ratios_host(c["values"], c["weights"], c["R"], c["seed"])
    want = br.expected(name)
    assert got.dtype == np.float64 and got.shape == (c["R"] + 1, c["values"].shape[0])
    assert np.array_equal(bits(got), bits(want))


def test_host_does_not_depend_on_its_chunking(monkeypatch):
    from bmhrl_amd import evaluate
    c = br.CASES["N65_M3_R300_zeroseed_some"]
    whole = evaluate.bootstrap_ratios_host(c["values"], c["weights"], c["R"], c["seed"])
    monkeypatch.setattr(evaluate, "_BOOT_CHUNK", 1)                        # one row per pass
    assert np.array_equal(bits(evaluate.bootstrap_ratios_host(c["values"], c["weights"], c["R"], c["seed"])), bits(whole))


@pytest.mark.parametrize("N,seed", [(1, 0), (2, br.BIG_SEED), (65, 0), (400, 7), (16384, br.BIG_SEED)])
def test_counts_are_the_restatements_and_sum_to_n(N, seed):
    from bmhrl_amd.evaluate import bootstrap_counts
    rows = [0, 1, 2, 3, 1000, (1 << 20)]
    got = bootstrap_counts(N, rows, seed)
    assert got.shape == (len(rows), N) and (got >= 0).all()
    assert (got.sum(axis=1) == N).all()                                    # every resample makes N draws
    assert (got[0] == 1).all()
    for k, r in enumerate(rows[:4] if N > 400 else rows):
        assert got[k].tolist() == br.counts(N, r, seed), r
    assert not np.array_equal(got[1], got[2]) or N == 1


@pytest.mark.parametrize("name", [n for n, c in br.CASES.items() if c["weights"] is None])
def test_row_zero_agrees_with_the_mean(name):
    """both are N-term fp64 sums (the division by N is one more rounding each, inside the bound's slack for N >= 2; N = 1
    is exact): |row 0 - np.mean| <= 2 (N - 1) 2^-53 sum|x| / N"""
    from bmhrl_amd.evaluate import bootstrap_ratios_host
    c = br.CASES[name]
    x = c["values"]
    N = x.shape[1]
    row0 = bootstrap_ratios_host(x, None, c["R"], c["seed"])[0]
    bound = 2.0 * max(N - 1, 0) * 2.0 ** -53 * np.abs(x).sum(axis=1) / N
    err = np.abs(row0 - np.mean(x, axis=1))
    print(name, err.max(), bound.min())
    assert (err <= bound).all()


def test_a_column_of_zero_weights_gives_zero():
    from bmhrl_amd.evaluate import bootstrap_ratios_host
    for name, c in br.CASES.items():
        if not name.endswith("zero_column"):
            continue
        M = c["values"].shape[0]
        got = bootstrap_ratios_host(c["values"], c["weights"], c["R"], c["seed"])
        assert np.array_equal(bits(got[:, M // 2]), bits(np.zeros(c["R"] + 1))), name      # +0.0, every row
        if M > 1:
            assert np.count_nonzero(got[:, :M // 2]) > 0


def test_refusals():
    from bmhrl_amd.evaluate import bootstrap_ratios_host
    x = np.ones((2, 5))
    for bad in (dict(values=np.ones(5)), dict(weights=np.ones((2, 4))), dict(resamples=0), dict(resamples=(1 << 20) + 1),
                dict(values=np.ones((2, 16385))), dict(values=np.ones((4097, 2))), dict(values=np.ones((0, 5))),
                dict(values=np.ones((2, 0))), dict(seed=-1), dict(seed=1 << 64),
                dict(values=np.array([[1.0, np.nan]])), dict(values=np.array([[1.0, np.inf]])),
                dict(weights=np.array([[1.0, 1.0, -np.inf, 1.0, 1.0]] * 2))):
        args = dict(values=x, weights=None, resamples=3, seed=0)
        args.update(bad)
        with pytest.raises(ValueError):
            bootstrap_ratios_host(**args)
    assert bootstrap_ratios_host(x, None, 3, (1 << 64) - 1).tolist() == [[1.0, 1.0]] * 4


DRAW_N, DRAW_R, DRAW_SEED = 400, 4000, 2024


def test_the_draw_is_sound():
    """seeded, N = 400, R = 4000.  A video's total over all resamples is a sum of R counts of mean 1 and variance 1 - 1/N:
    within 6 sqrt(R) of R.  The standard error of the mean of a column of normal values is s sqrt((N - 1) / N) / sqrt(N)
    under the bootstrap; the R resampled means estimate it with relative sampling error 1 / sqrt(2 R) = 1.1 %: within 6 %."""
    from bmhrl_amd.evaluate import bootstrap_counts, bootstrap_ratios_host, summarize
    N, R = DRAW_N, DRAW_R
    c = bootstrap_counts(N, np.arange(1, R + 1), DRAW_SEED)
    total = c.sum(axis=0)
    print("totals", total.min(), total.max(), 6 * math.sqrt(R))
    assert (np.abs(total - R) <= 6 * math.sqrt(R)).all()
    x = np.random.RandomState(5).standard_normal((1, N))
    stats = bootstrap_ratios_host(x, None, R, DRAW_SEED)
    _, _, se = summarize(stats)
    want = x.std(ddof=1) * math.sqrt((N - 1) / N) / math.sqrt(N)
    print("se", se[0], want, se[0] / want - 1)
    assert abs(se[0] / want - 1) <= 0.06
    assert abs(stats[1:].mean() - stats[0, 0]) <= 6 * want / math.sqrt(R)       # the resampled means centre on the observed


@pytest.mark.parametrize("R,alpha,lo,hi", [(1, 0.05, 0, 0), (1, 0.5, 0, 0), (2, 0.05, 0, 1), (2, 0.5, 0, 1), (40, 0.05, 1, 38),
                                           (40, 0.5, 10, 29), (1000, 0.05, 25, 974), (1000, 0.5, 250, 749)])
def test_summarize_indices_worked_by_hand(R, alpha, lo, hi):
    """the resampled rows are a shuffle of 0 .. R - 1 (second column: their negatives), so sorted[k] = k:
    lo = floor(alpha / 2 * R), hi = ceil((1 - alpha / 2) * R) - 1, clamped to [0, R - 1] -- e.g. R = 40, alpha = 0.05:
    floor(1.0) = 1 and ceil(39.0) - 1 = 38; R = 2: floor(0.05) = 0 and ceil(1.95) - 1 = 1; R = 1: both 0"""
    import torch
    from bmhrl_amd.evaluate import summarize
    perm = np.random.RandomState(R).permutation(R).astype(np.float64)
    stats = np.concatenate([[[123.0, 456.0]], np.stack([perm, -perm], axis=1)])           # row 0 is not read
    got_lo, got_hi, se = summarize(stats, alpha)
    assert got_lo.tolist() == [float(lo), float(-(R - 1 - lo))] and got_hi.tolist() == [float(hi), float(-(R - 1 - hi))]
    want_se = math.sqrt(R * (R + 1) / 12.0) if R > 1 else 0.0                             # of 0 .. R - 1, unbiased
    assert np.allclose(se, want_se, rtol=1e-12, atol=0)
    t_lo, t_hi, t_se = summarize(torch.from_numpy(stats), alpha)                          # the torch route: the same picks
    assert t_lo.tolist() == got_lo.tolist() and t_hi.tolist() == got_hi.tolist()
    assert np.allclose(t_se.numpy(), want_se, rtol=1e-12, atol=0)


def test_summarize_refusals():
    from bmhrl_amd.evaluate import summarize
    for alpha in (0.0, 1.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            summarize(np.zeros((3, 1)), alpha)
    with pytest.raises(ValueError):
        summarize(np.zeros((1, 1)))


def stand_in(values, vids=None, weights=None, T=2):
    """what bootstrap / compare read of an evaluated DenseCaptionEvaluator: .per_video, .scores, .device"""
    values = np.asarray(values, dtype=np.float64)
    N = values.shape[-1]
    vids = [f"v{k}" for k in range(N)] if vids is None else vids
    per_video = {"tiou": (vids, {"METEOR": [values[t] for t in range(T)], "CIDEr": [values[t] * 2.0 for t in range(T)]})}
    scores = {"METEOR": [float(np.mean(values[t])) for t in range(T)], "CIDEr": [float(np.mean(values[t] * 2.0)) for t in range(T)]}
    if weights is not None:
        ratio = np.where(weights > 0, values[0], 0.0)
        per_video["paragraph"] = (vids, {"Para_Div_1": [np.stack([ratio, weights])] * T})
        scores["Para_Div_1"] = [float(ratio.sum() / weights.sum())] * T
    return SimpleNamespace(per_video=per_video, scores=scores, device="cpu")


def grid(seed, T=2, N=64):
    return np.random.RandomState(seed).randint(0, 64, (T, N)) / 64.0


def test_bootstrap_on_a_stand_in():
    from bmhrl_amd.evaluate import bootstrap, bootstrap_ratios_host, summarize
    x = grid(1)
    w = (np.arange(64) % 3 > 0).astype(np.float64)
    ev = stand_in(x, weights=w)
    ev.scores["METEOR"][1] = 0.123                                         # `value` is .scores' entry, not row 0
    out = bootstrap(ev, resamples=200, seed=3, alpha=0.1)
    assert sorted(out) == ["CIDEr", "METEOR", "Para_Div_1"] and all(len(v) == 2 for v in out.values())
    assert out["METEOR"][1]["value"] == 0.123
    lo, hi, se = summarize(bootstrap_ratios_host(np.stack([x[0], x[1], 2 * x[0], 2 * x[1]]), None, 200, 3), 0.1)
    assert [out["METEOR"][0][k] for k in ("lo", "hi", "se")] == [lo[0], hi[0], se[0]]
    assert [out["CIDEr"][1][k] for k in ("lo", "hi", "se")] == [lo[3], hi[3], se[3]]
    plo, phi, _ = summarize(bootstrap_ratios_host(np.where(w > 0, x[0], 0.0)[None], w[None], 200, 3), 0.1)
    assert (out["Para_Div_1"][0]["lo"], out["Para_Div_1"][1]["hi"]) == (plo[0], phi[0])
    for m, rows in out.items():
        for t, d in enumerate(rows):
            assert sorted(d) == ["hi", "lo", "se", "value"] and d["lo"] <= d["hi"] and d["se"] > 0
            if (m, t) != ("METEOR", 1):
                assert d["lo"] <= d["value"] <= d["hi"]
    with pytest.raises(ValueError):
        bootstrap(SimpleNamespace(per_video={}, scores={}, device="cpu"))


def test_compare_a_run_with_itself_and_with_a_shifted_copy():
    from bmhrl_amd.evaluate import compare
    b = grid(2)
    same = compare(stand_in(b), stand_in(b.copy()), resamples=100, seed=1)
    for rows in same.values():
        for d in rows:
            assert sorted(d) == ["a", "b", "delta", "hi", "lo", "losses", "wins"]
            assert d["delta"] == d["lo"] == d["hi"] == 0.0 and d["wins"] == d["losses"] == 0.0 and d["a"] == d["b"]
    # A = B + 0.25 on a grid of 1/64 with N = 64: every sum and the division by N are exact
    shifted = compare(stand_in(b + 0.25), stand_in(b), resamples=100, seed=1)
    for t in range(2):
        d = shifted["METEOR"][t]
        assert d["wins"] == 1.0 and d["losses"] == 0.0 and d["lo"] == d["hi"] == d["delta"] == 0.25
        assert shifted["CIDEr"][t]["lo"] == shifted["CIDEr"][t]["hi"] == 0.5
    back = compare(stand_in(b), stand_in(b + 0.25), resamples=100, seed=1)
    assert back["METEOR"][0]["losses"] == 1.0 and back["METEOR"][0]["wins"] == 0.0 and back["METEOR"][0]["hi"] == -0.25


def test_compare_sees_one_resample_for_both_runs(monkeypatch):
    from bmhrl_amd import evaluate
    calls = []
    real = evaluate.bootstrap_ratios_host
    monkeypatch.setattr(evaluate, "bootstrap_ratios_host", lambda v, w, r, s: (calls.append(v.shape), real(v, w, r, s))[1])
    a, b = grid(3), grid(4)
    w = np.ones(64)
    out = evaluate.compare(stand_in(a, weights=w), stand_in(b, weights=w), resamples=50, seed=9)
    assert calls == [(8, 64), (4, 64)]                                     # one (2 M, N) call per family
    stats = real(np.concatenate([a, 2 * a, b, 2 * b]), None, 50, 9)
    delta = np.sort(stats[1:, 0] - stats[1:, 4])
    d = out["METEOR"][0]
    assert (d["lo"], d["hi"]) == (delta[1], delta[48])                     # floor(0.025 * 50) = 1, ceil(0.975 * 50) - 1 = 48
    assert d["wins"] == (delta > 0).mean() and d["losses"] == (delta < 0).mean() and 0 < d["wins"] < 1


def test_compare_refuses_different_videos():
    from bmhrl_amd.evaluate import compare
    b = grid(5)
    vids = [f"v{k}" for k in range(64)]
    other = list(vids)
    other[17] = "v_other"
    with pytest.raises(ValueError, match="position 17: 'v17' and 'v_other'"):
        compare(stand_in(b, vids), stand_in(b, other))
    with pytest.raises(ValueError, match="position 63: 'v63' and None"):
        compare(stand_in(b, vids), stand_in(b[:, :63], vids[:63]))
    with pytest.raises(ValueError, match="position 63: None and 'v63'"):                   # the mirrored case: A is B's prefix
        compare(stand_in(b[:, :63], vids[:63]), stand_in(b, vids))
    with pytest.raises(ValueError):
        compare(stand_in(b, vids), stand_in(b, vids, weights=np.ones(64)))                 # another family
    with pytest.raises(ValueError):
        compare(stand_in(b, vids), SimpleNamespace(per_video={}, scores={}, device="cpu"))  # not evaluated


def test_the_evaluator_takes_and_checks_the_keywords():
    from bmhrl_amd.evaluate import DenseCaptionEvaluator
    gt = {"v1": {"duration": 10.0, "timestamps": [[0.0, 5.0]], "sentences": ["a man"]}}
    sub = {"results": {"v1": [{"sentence": "a man", "timestamp": [0.0, 5.0]}]}, "version": "x", "external_data": {}}
    for bad in (dict(bootstrap=0), dict(bootstrap=-3), dict(bootstrap=2.5), dict(bootstrap=True), dict(bootstrap_alpha=0.0),
                dict(bootstrap_alpha=1.0)):
        with pytest.raises(ValueError):
            DenseCaptionEvaluator(gt, sub, [0.5], only_proposals=True, **bad)
    ev = DenseCaptionEvaluator(gt, sub, [0.5], only_proposals=True, bootstrap=100, bootstrap_seed=4, bootstrap_alpha=0.1)
    assert (ev.bootstrap, ev.bootstrap_seed, ev.bootstrap_alpha) == (100, 4, 0.1)
    ev.evaluate()                                                          # proposals only: nothing is a mean over videos
    assert ev.per_video == {} and ev.intervals == {}
    plain = DenseCaptionEvaluator(gt, sub, [0.5], only_proposals=True)
    assert plain.bootstrap is None and plain.per_video == {} and plain.intervals == {}


# ---- a real DenseCaptionEvaluator on the CPU, its device score calls behind tests/test_soda_cpu.py's stand-ins
# (soda_scores is the host restatement, score_pairs gives zeros): .evaluate() -> bootstrap -> bootstrap_ratios_host
def soda_job():
    from tests.test_soda_cpu import GT_A, seg
    gt = dict(GT_A)
    gt["v3"] = {"duration": 30.0, "timestamps": [[0, 12], [12, 30]], "sentences": ["A woman sings.", "The crowd claps loudly."]}
    gt["v4"] = {"duration": 10.0, "timestamps": [[0, 10]], "sentences": ["Two men talk."]}
    gt["v5"] = {"duration": 10.0, "timestamps": [[0, 10]], "sentences": ["Nothing is predicted here."]}
    results = {"v1": [seg(0, 10, "a dog runs"), seg(10, 20, "the cat sits")], "v2": [seg(0, 18, "a man plays a guitar")],
               "v3": [seg(0, 11, "a woman sings a song"), seg(14, 30, "the crowd claps")], "v4": [seg(2, 9, "two women talk")]}
    return [gt], results


def test_a_real_evaluator_on_the_cpu_keeps_its_scores_and_fills_per_video_and_intervals(monkeypatch):
    from bmhrl_amd import evaluate as E
    from tests.test_soda_cpu import evaluator
    gts, results = soda_job()
    calls = []
    real = E.bootstrap_ratios_host
    monkeypatch.setattr(E, "bootstrap_ratios_host", lambda v, w, r, s: (calls.append((v.shape, w, r, s)), real(v, w, r, s))[1])
    plain, _ = evaluator(monkeypatch, gts, results)
    assert calls == [] and plain.intervals == {} and plain.bootstrap is None
    boot, _ = evaluator(monkeypatch, gts, results, bootstrap=200, bootstrap_seed=6, bootstrap_alpha=0.1)
    assert calls == [((14, 5), None, 200, 6), ((6, 5), None, 200, 6)]       # one call per family: tiou, soda; two tIoUs
    # .scores is unchanged with and without bootstrap=
    assert list(plain.scores) == list(boot.scores)
    for k in plain.scores:
        assert np.asarray(plain.scores[k]).tobytes() == np.asarray(boot.scores[k]).tobytes(), k
    # .per_video means reproduce .scores, with and without the keyword
    for ev in (plain, boot):
        assert list(ev.per_video) == ["tiou", "soda"]
        vids, kept = ev.per_video["tiou"]
        assert vids == ["v1", "v2", "v3", "v4", "v5"] and list(kept) == list(E.METRICS)
        for m in E.METRICS:
            assert [float(np.mean(col)) for col in kept[m]] == ev.scores[m] and all(col.shape == (5,) for col in kept[m])
        vids, kept = ev.per_video["soda"]
        assert vids == list(ev.soda_per_video) == ["v1", "v2", "v3", "v4", "v5"] and list(kept) == list(E.SODA_METRICS)
        for m in E.SODA_METRICS:
            assert [sum(col.tolist(), 0.0) / len(col) for col in kept[m]] == ev.scores[m]
        assert ev.scores["SODA_c"][0] > 0.2 and len(set(ev.per_video["soda"][1]["SODA_c"][0].tolist())) >= 4
    # .intervals: lo <= hi for every metric and tIoU, value from .scores, the figures of the host route
    assert sorted(boot.intervals) == sorted(E.METRICS + E.SODA_METRICS)
    for m, rows in boot.intervals.items():
        assert len(rows) == 2
        for t, d in enumerate(rows):
            assert sorted(d) == ["hi", "lo", "se", "value"] and d["value"] == boot.scores[m][t] and d["lo"] <= d["hi"]
    assert all(d == dict(value=0.0, lo=0.0, hi=0.0, se=0.0) for d in boot.intervals["METEOR"])    # the stand-in's zeros
    d = boot.intervals["SODA_c"][0]
    assert d["lo"] < d["value"] < d["hi"] and d["se"] > 0
    lo, hi, se = E.summarize(real(np.stack(boot.per_video["soda"][1]["SODA_c"]), None, 200, 6), 0.1)
    assert (d["lo"], d["hi"], d["se"]) == (lo[0], hi[0], se[0])
    assert E.bootstrap(boot, 200, 6, 0.1) == boot.intervals
    # and compare on two real evaluators over the same videos
    other = dict(results, v2=[{"timestamp": [0, 18], "sentence": "a man plays the guitar"}])
    second, _ = evaluator(monkeypatch, gts, other)
    out = E.compare(second, plain, resamples=100, seed=1)
    assert out["SODA_c"][0]["a"] > out["SODA_c"][0]["b"] and out["SODA_c"][0]["wins"] > 0 and out["SODA_c"][0]["losses"] == 0


def test_rows_per_workgroup_query():
    from bmhrl_amd import _lib, ops
    assert [ops.bootstrap_rows(n, 10) for n in (1, 2560, 2561, 4917, 5120, 5121, 16384)] == [4, 4, 2, 2, 2, 1, 1]
    assert [ops.bootstrap_rows(64, r) for r in (1, 2, 3)] == [2, 2, 4]
    for n, r in ((0, 5), (16385, 5), (5, 0), (5, (1 << 20) + 1)):
        with pytest.raises(_lib.HipError):
            ops.bootstrap_rows(n, r)


def test_limits_are_the_headers():
    import re
    from bmhrl_amd import evaluate, ops
    from tests.conftest import ROOT
    with open(f"{ROOT}/include/bmhrl_hip.h") as f:
        header = f.read()
    macro = lambda name: int(re.search(rf"#define {name} (\d+)", header).group(1))                          # noqa: E731
    limits = (macro("BMHRL_BOOTSTRAP_MAX_N"), macro("BMHRL_BOOTSTRAP_MAX_M"), macro("BMHRL_BOOTSTRAP_MAX_R"))
    assert limits == (16384, 4096, 1048576) == evaluate.BOOTSTRAP_LIMITS
    assert limits == (ops.BOOTSTRAP_MAX_N, ops.BOOTSTRAP_MAX_M, ops.BOOTSTRAP_MAX_R)
    with open(f"{ROOT}/bmhrl_amd/csrc/bootstrap.hip") as f:
        assert f"kColBlock = {br.COLUMN_BLOCK};" in f.read()
