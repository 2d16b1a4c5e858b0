"""bmhrl_bootstrap_ratios (bmhrl_amd/csrc/bootstrap.hip) on the MI355X: the statistics against the
plain-loop restatement of tests/bootstrap_reference.py, bit for bit, twice, over that module's cases (N = 1, 2, 63, 64, 65,
255, 256, 257, 4097, 16384 and both sides of the thresholds at which a workgroup carries 4, 2 or 1 rows; M = 1, 3, 4, 5 and
one above the column block; R = 1, 2, 5 and 300; weights absent, present, with an all-zero column; seed 0 and one above
2^32; values of mixed sign); every refusal; the evaluator's .per_video and .intervals; bootstrap and compare on device
evaluators against the host route."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import bootstrap_reference as br
from tests.meteor_reference import DictStemmer, dict_synonyms
from tests.test_paragraph_cpu import job  # noqa: F401  (two invented ground-truth files and a submission)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TIOUS = [0.3, 0.5, 0.7]


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def run(c):
    from bmhrl_amd import ops
    dev = lambda a: None if a is None else torch.from_numpy(a).to(DEV)                                      # noqa: E731
    out = ops.bootstrap_ratios(dev(c["values"]), dev(c["weights"]), c["R"], c["seed"])
    assert out.dtype == torch.float64 and tuple(out.shape) == (c["R"] + 1, c["values"].shape[0]) and out.device == DEV
    return out.cpu().numpy()


@pytest.mark.parametrize("name", list(br.CASES))
def test_equals_the_restatement_bit_for_bit(name):
    want = br.expected(name)
    got = run(br.CASES[name])
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(run(br.CASES[name])), bits(got))            # two runs, equal bits


def test_refusals_leave_the_output_untouched():
    from bmhrl_amd import _lib, ops
    lib = _lib.load()
    N, M, R = 70, 3, 4
    values = torch.from_numpy(br.CASES["N65_M3_R300_zeroseed_some"]["values"]).to(DEV)
    values = torch.cat([values, values[:, :5]], dim=1).contiguous()
    weights = torch.ones(M, N, dtype=torch.float64, device=DEV)
    stats = torch.full((R + 1, M), -7.0, dtype=torch.float64, device=DEV)
    st = ops.stream()

    def call(values_p=values.data_ptr(), weights_p=weights.data_ptr(), N=N, M=M, R=R, seed=0, stats_p=stats.data_ptr()):
        return lib.bmhrl_bootstrap_ratios(values_p, weights_p, N, M, R, seed, stats_p, st)

    assert call(values_p=None) == -22 and call(stats_p=None) == -22
    assert call(N=0) == -22 and call(N=-1) == -22 and call(N=16385) == -22          # before any launch
    assert call(M=0) == -22 and call(M=-1) == -22 and call(M=4097) == -22
    assert call(R=0) == -22 and call(R=-1) == -22 and call(R=(1 << 20) + 1) == -22
    torch.cuda.synchronize()
    assert bool((stats == -7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    with_ones = stats.clone()
    assert call(weights_p=None) == 0                                        # weights are optional: sum / N
    torch.cuda.synchronize()
    want = br.bootstrap_ratios(values.cpu().numpy(), None, R, 0)
    assert np.array_equal(bits(stats), bits(want))
    # unit weights: the denominator is N, summed exactly -- the same quotient
    assert np.array_equal(bits(with_ones), bits(want))
    # and through ops: the checked call path reports the library's refusal, the wrapper the malformed tensors
    for kwargs in (dict(resamples=0), dict(resamples=(1 << 20) + 1)):
        with pytest.raises(_lib.HipError, match="bmhrl_bootstrap_ratios failed: invalid argument -22"):
            ops.bootstrap_ratios(values, None, **kwargs)
    with pytest.raises(_lib.HipError):
        ops.bootstrap_ratios(torch.zeros(1, 16385, dtype=torch.float64, device=DEV), None, 2)
    with pytest.raises(_lib.HipError):
        ops.bootstrap_ratios(torch.zeros(4097, 2, dtype=torch.float64, device=DEV), None, 2)
    for bad in (lambda: ops.bootstrap_ratios(values.float(), None, 2), lambda: ops.bootstrap_ratios(values[0], None, 2),
                lambda: ops.bootstrap_ratios(values, weights[:, :5], 2), lambda: ops.bootstrap_ratios(values, weights.float(), 2),
                lambda: ops.bootstrap_ratios(values.t(), None, 2), lambda: ops.bootstrap_ratios(values, weights.cpu(), 2),
                lambda: ops.bootstrap_ratios(values, None, 2, seed=-1), lambda: ops.bootstrap_ratios(values, None, 2, seed=1 << 64)):
        with pytest.raises(ValueError):
            bad()
    assert (ops.BOOTSTRAP_MAX_N, ops.BOOTSTRAP_MAX_M, ops.BOOTSTRAP_MAX_R) == (16384, 4096, 1 << 20)
    torch.cuda.synchronize()


def test_bootstrap_ratios_is_one_launch(monkeypatch):
    from bmhrl_amd import ops
    calls = []
    real = ops._launch
    monkeypatch.setattr(ops, "_launch", lambda name, *a: (calls.append(name), real(name, *a))[1])
    run(br.CASES["N65_M130_R2_bigseed_zero_column"])
    assert calls == ["bmhrl_bootstrap_ratios"]


def evaluator(gts, results, launches=None, **kw):
    from bmhrl_amd import ops
    from bmhrl_amd.evaluate import DenseCaptionEvaluator
    sub = {"results": results, "version": "x", "external_data": {}}
    real = ops._launch
    if launches is not None:
        ops._launch = lambda name, *a: (launches.append(name), real(name, *a))[1]
    try:
        ev = DenseCaptionEvaluator(gts, sub, TIOUS, 1000, device=DEV, stemmer=DictStemmer(), synonyms=dict_synonyms, **kw)
        ev.evaluate()
    finally:
        ops._launch = real
    return ev


_RUNS = []


@pytest.fixture()
def runs(job):  # noqa: F811
    """(plain, with bootstrap, another submission with bootstrap) and the launches of the first two, soda and paragraph
    on; evaluated once for the module"""
    if not _RUNS:
        _RUNS.append(make_runs(*job))
    return _RUNS[0]


def make_runs(gts, results):
    other = copy.deepcopy(results)
    other["v1"][0]["sentence"] = "a man sings"
    other["v2"][0]["sentence"] = "the dog runs away"
    other["v5"][0]["sentence"] = "two women talk"
    la, lb = [], []
    plain = evaluator(gts, results, la, soda=True, paragraph=True, verbose=True)
    boot = evaluator(gts, results, lb, soda=True, paragraph=True, verbose=True, bootstrap=200, bootstrap_seed=5,
                     bootstrap_alpha=0.1)
    second = evaluator(gts, other, None, soda=True, paragraph=True, verbose=True, bootstrap=200, bootstrap_seed=5)
    return plain, boot, second, la, lb


def test_scores_do_not_move_and_the_launches_are_the_old_ones_plus_one_per_family(runs):
    plain, boot, _, la, lb = runs
    assert list(plain.scores) == list(boot.scores)
    for k in plain.scores:
        assert np.asarray(plain.scores[k]).tobytes() == np.asarray(boot.scores[k]).tobytes(), k
    assert "bmhrl_bootstrap_ratios" not in la and plain.intervals == {}
    assert lb.count("bmhrl_bootstrap_ratios") == 3                         # tiou, soda, paragraph
    assert [n for n in lb if n != "bmhrl_bootstrap_ratios"] == la          # without the keyword: exactly the calls it made


def test_per_video_means_reproduce_the_scores(runs):
    from bmhrl_amd.evaluate import METRICS, PARAGRAPH_STAT_KEYS, SODA_METRICS
    plain = runs[0]
    assert list(plain.per_video) == ["tiou", "soda", "paragraph"]
    vids, kept = plain.per_video["tiou"]
    assert vids == ["v1", "v2", "v3", "v4", "v5"] and list(kept) == list(METRICS)
    for m in METRICS:
        assert len(kept[m]) == len(TIOUS)
        for t, col in enumerate(kept[m]):
            assert col.dtype == np.float64 and col.shape == (5,)
            assert float(np.mean(col)) == plain.scores[m][t], (m, t)
    assert plain.scores["METEOR"][0] > 0
    vids, kept = plain.per_video["soda"]
    assert vids == list(plain.soda_per_video) and list(kept) == list(SODA_METRICS)
    for m in SODA_METRICS:
        for t, col in enumerate(kept[m]):
            assert sum(col.tolist(), 0.0) / len(col) == plain.scores[m][t], (m, t)
    vids, kept = plain.per_video["paragraph"]
    assert vids == list(plain.paragraph_per_video) and list(kept) == list(PARAGRAPH_STAT_KEYS)
    for m in PARAGRAPH_STAT_KEYS:
        for t, col in enumerate(kept[m]):
            assert col.shape == (2, 5) and set(col[1].tolist()) <= {0.0, 1.0} and not col[0][col[1] == 0].any()
            vals = col[0][col[1] > 0].tolist()
            assert (sum(vals) / len(vals) if vals else 0.0) == plain.scores[m][t], (m, t)
    assert 0 < kept["Para_Div_1"][0][1].sum() < 5                          # v3 and v4 hold no token: weight 0


def test_intervals(runs):
    from bmhrl_amd.evaluate import METRICS, PARAGRAPH_STAT_KEYS, SODA_METRICS, bootstrap
    _, boot, _, _, _ = runs
    assert sorted(boot.intervals) == sorted(METRICS + SODA_METRICS + PARAGRAPH_STAT_KEYS)
    for m, rows in boot.intervals.items():
        assert len(rows) == len(TIOUS)
        for t, d in enumerate(rows):
            assert sorted(d) == ["hi", "lo", "se", "value"]
            assert d["value"] == boot.scores[m][t] and d["lo"] <= d["hi"] and d["se"] >= 0.0
    assert boot.intervals["METEOR"][0]["lo"] < boot.intervals["METEOR"][0]["hi"]
    again = bootstrap(boot, 200, 5, 0.1)                                   # the keyword is this call
    assert again == boot.intervals


def on_host(ev):
    return SimpleNamespace(per_video=ev.per_video, scores=ev.scores, device="cpu")


def same_but_se(got, want):
    assert list(got) == list(want)
    for m in got:
        assert len(got[m]) == len(want[m])
        for g, w in zip(got[m], want[m]):
            assert list(g) == list(w)
            for k in g:
                if k == "se":                                              # torch's reduction order is not defined here
                    assert abs(g[k] - w[k]) <= 1e-12 * abs(w[k]), (m, k, g[k], w[k])
                else:
                    assert np.float64(g[k]).tobytes() == np.float64(w[k]).tobytes(), (m, k, g[k], w[k])


def test_device_and_host_routes_agree(runs):
    from bmhrl_amd.evaluate import bootstrap, compare
    _, boot, second, _, _ = runs
    same_but_se(bootstrap(boot, 300, 11, 0.05), bootstrap(on_host(boot), 300, 11, 0.05))
    got = compare(boot, second, 300, 11, 0.05)
    same_but_se(got, compare(on_host(boot), on_host(second), 300, 11, 0.05))
    assert got["METEOR"][0]["a"] == boot.scores["METEOR"][0] and got["METEOR"][0]["b"] == second.scores["METEOR"][0]
    assert any(d["wins"] > 0 for rows in got.values() for d in rows)       # the two submissions differ
    assert all(0.0 <= d["wins"] + d["losses"] <= 1.0 and d["lo"] <= d["hi"] for rows in got.values() for d in rows)
    own = compare(boot, boot, 50, 0)
    assert all(d["lo"] == d["hi"] == d["wins"] == d["losses"] == 0.0 for rows in own.values() for d in rows)


def test_the_option_reaches_the_loops_metrics(runs):
    from bmhrl_amd.epoch_loops.validation_loops import calculate_metrics
    _, boot, _, _, _ = runs
    base = dict(device=DEV, stemmer=DictStemmer(), synonyms=dict_synonyms, soda=True, paragraph=True)
    sub = {"results": boot.prediction, "version": "x", "external_data": {}}
    plain = calculate_metrics(boot.ground_truths, sub, TIOUS, 1000, evaluator="device", evaluator_options=base)
    assert list(plain) == TIOUS + ["Average across tIoUs"]
    with_opt = calculate_metrics(boot.ground_truths, sub, TIOUS, 1000, evaluator="device",
                                 evaluator_options=dict(base, bootstrap=200, bootstrap_seed=5, bootstrap_alpha=0.1))
    assert list(with_opt) == TIOUS + ["Average across tIoUs", "Bootstrap intervals"]
    assert all(with_opt[k] == plain[k] for k in plain)
    same_but_se(with_opt["Bootstrap intervals"], boot.intervals)
