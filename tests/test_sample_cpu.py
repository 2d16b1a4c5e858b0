"""Sampled decoding, the re-run path (bmhrl_amd.decode.sample_decode with incremental=False; on CPU tensors the only path):
the rules of the module's sampling section pinned on the table model of tests/test_beam_cpu.py, whose log-probs come from a
fixed table indexed by (sample, previous token, position)."""
import math

import numpy as np
import pytest
import torch

from bmhrl_amd.decode import greedy_decode, sample_decode, sample_decoder, uniform01
from tests.test_beam_cpu import END, PAD, START, TableModel, _features, _pad_after_end

AV = "audio_video"


def _kept_set(lp, T, k, p):
    """the kept tokens of rule 3 for one fp32 log-prob row, in float64"""
    V = lp.numel()
    q = torch.exp((lp.double() - lp.max()) / T)
    order = torch.sort(-lp, stable=True).indices
    cum = q[order].cumsum(0)
    c = V if k == 0 or k >= V else k
    if p < 1:
        c = min(c, int((cum < float(np.float32(p)) * cum[-1]).sum()) + 1)
    return set(order[:c].tolist()), q


def test_uniform01_mirrors_the_device_generator():
    """splitmix64 finaliser, upper 32 bits, then 24 bits of mantissa: pinned values, uint64 wraparound of seed + index"""
    u = uniform01(0, [0, 1, 2, 2 ** 40])
    assert u[0] == 0.0 and all(0 <= x < 1 for x in u)
    assert np.array_equal(u * 16777216.0, np.floor(u * 16777216.0))             # multiples of 2^-24
    assert uniform01(2 ** 64 + 5, [7]) == uniform01(5, [7])
    assert uniform01(2 ** 64 - 1, [1]) == uniform01(-1, [1])

    def ref(seed, idx):                                                         # the C code with Python ints
        m = 2 ** 64 - 1
        z = (idx * 0x9E3779B97F4A7C15 + seed) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        z ^= z >> 31
        return ((z >> 32) >> 8) / 16777216.0
    for seed, idx in ((1, 3), (12345, (7 << 16) + 29), (2 ** 63 + 11, 2 ** 48 + 1), (2 ** 64 - 1, 2 ** 64 - 1)):
        assert uniform01(seed, [idx])[0] == ref(seed, idx)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("kw", [dict(temperature=0.0), dict(top_k=1), dict(top_p=1e-9)])
def test_degenerate_sampling_is_greedy(kw, n):
    B, V, L = 5, 12, 9
    model = TableModel(B, V, L + 1, seed=1)
    fs = _features(B)
    greedy = greedy_decode(model, fs, L, START, END, PAD, AV, memoise=False)
    assert (greedy[:, 1:] == END).any()
    got = sample_decode(model, fs, L, START, END, PAD, AV, n=n, seed=9, incremental=False, **kw)
    assert got.dtype == torch.int64
    assert torch.equal(got, _pad_after_end(greedy))
    _, samples, sums, slp, slq = sample_decode(model, fs, L, START, END, PAD, AV, n=n, seed=9, return_samples=True, **kw)
    assert bool((slq == 0).all())                                              # a point mass: log 1
    for i in range(n):
        assert torch.equal(samples[:, i, :got.shape[1]], got)


@pytest.mark.parametrize("T,k,p", [(1.0, 3, 1.0), (0.7, 0, 0.6), (1.5, 4, 0.8), (1.0, 0, 1.0)])
def test_every_token_lies_in_its_truncated_set(T, k, p):
    B, V, L, n = 4, 10, 7, 5
    model = TableModel(B, V, L + 1, seed=2, scale=2.0)
    fs = _features(B)
    _, samples, sums, slp, slq = sample_decode(model, fs, L, START, END, PAD, AV, n=n, temperature=T, top_k=k, top_p=p,
                                               seed=3, return_samples=True)
    checked = 0
    for b in range(B):
        for i in range(n):
            row = samples[b, i].tolist()
            s = torch.zeros((), dtype=torch.float64)
            for t in range(1, len(row)):
                lp = model.table[b, row[t - 1], t - 1]
                kept, q = _kept_set(lp, T, k, p)
                assert row[t] in kept, (b, i, t)
                assert float(slp[b, i, t - 1]) == float(lp[row[t]])               # the model's log-prob, T-free
                mass = sum(float(q[v]) for v in kept)
                assert math.isclose(float(slq[b, i, t - 1]), math.log(float(q[row[t]]) / mass), abs_tol=1e-5)
                s += float(lp[row[t]])
                checked += 1
                if row[t] == END:
                    assert all(v == PAD for v in row[t + 1:]) and bool((slp[b, i, t:] == 0).all())
                    break
            assert math.isclose(float(sums[b, i]), float(s), abs_tol=1e-4)
    assert checked > B * n


def test_seeds_rows_and_repeats():
    B, V, L, n = 3, 40, 6, 4
    model = TableModel(B, V, L + 1, seed=4, scale=0.3)                      # high entropy: draws of one table differ
    fs = _features(B)
    run = lambda seed: sample_decode(model, fs, L, START, -1, PAD, AV, n=n, seed=seed, return_samples=True)[1]
    a, b, c = run(11), run(11), run(12)
    assert torch.equal(a, b)
    assert not torch.equal(a, c)
    for clip in range(B):
        assert len({tuple(r.tolist()) for r in a[clip]}) == n                # the n rows of one clip differ
    assert a.shape == (B, n, L + 1)                                         # end_idx -1: max_len steps


def test_first_token_frequencies_follow_the_tempered_truncated_softmax():
    """2^14 rows of one clip, one step: chi-square of the first-token counts at a fixed seed (deterministic)"""
    V, rows = 30, 2 ** 14
    model = TableModel(1, V, 2, seed=6, scale=1.5)
    fs = _features(1)
    for T, k, p in ((1.0, 0, 1.0), (0.6, 8, 1.0), (1.4, 0, 0.7)):
        _, samples, _, _, _ = sample_decode(model, fs, 1, START, -1, PAD, AV, n=rows, temperature=T, top_k=k, top_p=p, seed=8,
                                            return_samples=True)
        counts = torch.bincount(samples[0, :, 1], minlength=V).double()
        kept, q = _kept_set(model.table[0, START, 0], T, k, p)
        mask = torch.zeros(V, dtype=torch.bool)
        mask[list(kept)] = True
        assert int(counts[~mask].sum()) == 0
        expect = rows * q[mask] / q[mask].sum()
        chi2 = float(((counts[mask] - expect) ** 2 / expect).sum())
        dof = int(mask.sum()) - 1
        assert chi2 < dof + 6 * math.sqrt(2 * dof) + 10, (T, k, p, chi2, dof)


@pytest.mark.parametrize("length_penalty", [0.0, 1.5])
def test_shapes_padding_and_best_of_n(length_penalty):
    B, V, L, n = 4, 9, 8, 6
    model = TableModel(B, V, L + 1, seed=5)
    fs = _features(B)
    toks, samples, sums, slp, slq = sample_decode(model, fs, L, START, END, PAD, AV, n=n, seed=21,
                                                  length_penalty=length_penalty, return_samples=True)
    m = samples.shape[-1] - 1
    assert samples.shape == (B, n, m + 1) and sums.shape == (B, n) and slp.shape == slq.shape == (B, n, m)
    assert sums.dtype == slp.dtype == slq.dtype == torch.float32 and samples.dtype == torch.int64
    assert bool((samples[..., 0] == START).all())
    is_end = samples[..., 1:] == END
    assert m == L or bool(is_end.any(-1).all())
    n_k = torch.where(is_end.any(-1), (is_end.cumsum(-1) == 0).sum(-1) + 1, torch.full((B, n), m))
    if m < L:
        assert int(n_k.max()) == m                                          # stops after the step all rows finished
    final = sums / ((5.0 + n_k.float()) / 6.0) ** length_penalty
    for b in range(B):
        best = max(range(n), key=lambda i: (float(final[b, i]), -i))
        want = samples[b, best, :int(n_k[b, best]) + 1]
        got = toks[b]
        assert torch.equal(got[:want.shape[0]], want) and bool((got[want.shape[0]:] == PAD).all())
    assert toks.shape[1] == int(max(n_k[b, int(torch.sort(-final[b], stable=True).indices[0])] for b in range(B))) + 1
    one = sample_decode(model, fs, L, START, END, PAD, AV, n=1, seed=21)
    s1 = sample_decode(model, fs, L, START, END, PAD, AV, n=1, seed=21, return_samples=True)[1]
    assert torch.equal(one, s1[:, 0, :one.shape[1]])                       # n = 1: the sample itself


def test_length_penalty_changes_only_the_choice():
    B, V, L, n = 3, 8, 7, 8
    model = TableModel(B, V, L + 1, seed=7)
    fs = _features(B)
    a = sample_decode(model, fs, L, START, END, PAD, AV, n=n, seed=2, return_samples=True)
    b = sample_decode(model, fs, L, START, END, PAD, AV, n=n, seed=2, length_penalty=3.0, return_samples=True)
    for x, y in zip(a[1:], b[1:]):
        assert torch.equal(x, y)


def test_invalid_arguments_are_refused():
    model = TableModel(1, 5, 4)
    fs = _features(1)
    for kw in (dict(n=0), dict(temperature=-0.1), dict(temperature=float("inf")), dict(top_k=-1), dict(top_p=0.0),
               dict(top_p=1.01)):
        with pytest.raises(ValueError):
            sample_decode(model, fs, 3, START, END, PAD, AV, **kw)
        with pytest.raises(ValueError):
            sample_decoder(**kw)


def test_sample_decoder_is_exported_for_the_reference_loops():
    import bmhrl_amd.install  # noqa: F401
    from epoch_loops.captioning_bmrl_loops import sample_decoder as exported
    from bmhrl_amd.epoch_loops.validation_loops import predict_1by1
    from types import SimpleNamespace
    assert exported is sample_decoder
    B, V, L = 3, 10, 6
    model = TableModel(B, V, L + 1, seed=4)
    fs = _features(B)
    itos = [f"w{i}" for i in range(V)]
    itos[START], itos[END], itos[PAD] = "<s>", "</s>", "<blank>"
    ds = SimpleNamespace(start_idx=START, end_idx=END, pad_idx=PAD, train_vocab=SimpleNamespace(itos=itos))
    batch = {"feature_stacks": fs, "video_ids": ["v0", "v1", "v0"], "starts": torch.tensor([0.0, 1.0, 2.0]),
             "ends": torch.tensor([1.0, 2.0, 3.0])}

    class Loader(list):
        dataset = ds
    pred = predict_1by1(SimpleNamespace(max_len=L, modality=AV), model, Loader([batch]), exported(n=4, top_p=0.9, seed=1))
    got = [seg["sentence"] for vid in ("v0", "v1") for seg in pred["results"][vid]]
    assert len(got) == B and all(isinstance(s, str) for s in got)
