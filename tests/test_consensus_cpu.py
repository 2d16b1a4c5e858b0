"""Consensus (minimum-Bayes-risk) choice among a clip's hypotheses, the host path (bmhrl_amd.decode.consensus_host and
select="consensus" on the re-run decoders; on CPU tensors the only path): hand-made cases whose answers are written here, the
restatement of tests/consensus_reference.py, and the decoders on the table model of tests/test_beam_cpu.py."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from bmhrl_amd import decode
from bmhrl_amd.decode import beam_decode, beam_decoder, consensus_host, idf_weights, sample_decode, sample_decoder
from tests import consensus_reference as ref
from tests.test_beam_cpu import END, PAD, START, TableModel, _features

AV = "audio_video"


def _hyps(*rows):
    """one clip (1, K, m + 1): [start] + words + [end] + padding for every list of words"""
    m = max(len(r) for r in rows) + 1
    return torch.tensor([[[START] + list(r) + [END] + [PAD] * (m - len(r) - 1) for r in rows]], dtype=torch.int64)


def _both(toks, N, w=None):
    """U and u of the host path, checked against the restatement (equality of every entry)"""
    U, u = consensus_host(toks, END, N, w, pair=True)
    assert U.dtype == torch.float64 and u.dtype == torch.float64
    t = ref.terms(toks.numpy(), END, None if w is None else w.numpy())
    U_ref, u_ref = ref.utilities(t, N)
    assert np.array_equal(U.numpy(), U_ref) and np.array_equal(u.numpy(), u_ref)
    assert torch.equal(consensus_host(toks, END, N, w), U)
    return U[0].tolist(), u[0].tolist()


def test_two_identical_hypotheses_and_one_different():
    U, u = _both(_hyps([5, 6, 7], [5, 6, 7], [5, 8, 9]), 2)
    third = 1.0 / 3.0
    assert u[0][1] == 1.0 and u[1][0] == 1.0                    # unigrams 3 / 3, bigrams 2 / 2
    assert u[0][2] == (third + 0.0) / 2.0 == u[2][0] == u[1][2]  # one unigram of three, no bigram
    assert U[0] == (1.0 + (third + 0.0) / 2.0) / 2.0 == U[1]
    assert U[2] == ((third + 0.0) / 2.0 + (third + 0.0) / 2.0) / 2.0
    assert [row[i] for i, row in enumerate(u)] == [0.0, 0.0, 0.0]


def test_an_empty_hypothesis_scores_nothing():
    U, u = _both(_hyps([], [5, 6], []), 2)                      # rows 0 and 2 end at column 1
    assert U == [0.0, 0.0, 0.0]                                 # max(W) = 0 between the two empty ones: t = 0, not 0 / 0
    assert all(v == 0.0 for row in u for v in row)


def test_a_hypothesis_shorter_than_the_gram():
    U, u = _both(_hyps([5], [5, 6]), 2)
    assert u[0][1] == (1.0 / 2.0 + 0.0) / 2.0                   # unigram 1 / max(1, 2); row 0 has no bigram
    assert u[1][0] == (1.0 / 2.0 + 0.0) / 2.0
    assert U == [0.25, 0.25]
    U4, _ = _both(_hyps([5], [5, 6]), 4)                        # g = 3, 4: neither row has a gram
    assert U4 == [(0.5 + 0.0 + 0.0 + 0.0) / 4.0] * 2


def test_a_repeated_gram_on_one_side_is_clipped():
    U, u = _both(_hyps([5, 5, 5, 6], [5, 6, 7]), 1)
    assert u[0][1] == 2.0 / 4.0                                 # min(3, 1) + min(1, 1) over max(4, 3); unclipped: 4 / 4
    assert u[1][0] == 2.0 / 4.0
    assert U == [0.5, 0.5]


def test_tokens_after_the_end_and_pad_before_it():
    a = torch.tensor([[[START, 5, PAD, 6, END, 7, 7], [START, 5, PAD, 7, 7, 7, 7]]])
    U, u = _both(a, 1)
    assert ref.words(a[0, 0].tolist(), END) == [5, PAD, 6] and ref.words(a[0, 1].tolist(), END) == [5, PAD, 7, 7, 7, 7]
    assert u[0][1] == 2.0 / 6.0 and U == [2.0 / 6.0, 2.0 / 6.0]  # 5 and the pad word match; the 7s behind row 0's end do not


def test_one_hypothesis_has_utility_zero():
    U, u = _both(_hyps([5, 6, 7]), 4)
    assert U == [0.0] and u == [[0.0]]


def test_a_weight_changes_the_winner():
    toks = _hyps([5, 4, 6], [5, 4, 7], [8, 9, 10], [11, 9, 12])
    order = torch.tensor([[0, 1, 2, 3]])
    n_k = torch.full((1, 4), 4)
    U, _ = _both(toks, 1)
    assert U == [(2.0 / 3.0 + 0.0 + 0.0) / 3.0] * 2 + [(0.0 + 0.0 + 1.0 / 3.0) / 3.0] * 2
    assert int(decode._consensus_choice(toks, n_k, order, torch.tensor([U], dtype=torch.float64))[0]) == 0
    w = torch.ones(13)
    w[5] = w[4] = 0.25                                          # the shared pair of rows 0 / 1 weighs little,
    w[9] = 4.0                                                  # the shared word of rows 2 / 3 much
    Uw, _ = _both(toks, 1, w)
    assert Uw[0] == (0.5 / 1.5 + 0.0 + 0.0) / 3.0 == Uw[1]      # W = 0.25 + 0.25 + 1, M = 0.25 + 0.25
    assert Uw[2] == (0.0 + 0.0 + 4.0 / 6.0) / 3.0 == Uw[3]      # W = 1 + 4 + 1, M = 4
    pick, best = decode._consensus_choice(toks, n_k, order, torch.tensor([Uw], dtype=torch.float64))
    assert int(pick) == 2 and best.tolist() == [[START, 8, 9, 10, END]]
    assert ref.choose(Uw, [0, 1, 2, 3]) == 2 and ref.choose(U, [0, 1, 2, 3]) == 0


def test_weights_of_ids_outside_the_table_and_bigram_means():
    toks = _hyps([5, 6], [5, 6, 20], [-4, 6])                   # V = 8: 20 and -4 weigh 0 and compare by their ids
    w = torch.tensor([1.0, 1.0, 1.0, 1.0, 1.0, 0.5, 3.0, 1.0])
    U, u = _both(toks, 2, w)
    # row 0 against row 1: unigrams (0.5 + 3) / max(3.5, 3.5 + 0), bigrams w(5 6) = (0.5 + 3) / 2 over max(1.75, 1.75 + 1.5)
    assert u[0][1] == ((0.5 * 1.0 + 3.0 * 1.0) / 3.5 + 1.75 / (1.75 + (3.0 + 0.0) / 2.0)) / 2.0
    assert u[0][2] == (3.0 / 3.5 + 0.0 / 1.75) / 2.0            # -4 is not 5; the bigram (-4 6) weighs 1.5


def test_the_tie_rule_follows_the_arranged_order():
    toks = _hyps([5, 6], [7, 8], [7, 8])
    util = torch.tensor([[0.5, 0.7, 0.7]], dtype=torch.float64)
    n_k = torch.tensor([[3, 3, 3]])
    for order, want in (([0, 1, 2], 1), ([2, 0, 1], 2), ([0, 2, 1], 2), ([1, 2, 0], 1)):
        pick, _ = decode._consensus_choice(toks, n_k, torch.tensor([order]), util)
        assert int(pick) == want == ref.choose(util[0].tolist(), order), order
    same = torch.zeros(1, 3, dtype=torch.float64)
    assert int(decode._consensus_choice(toks, n_k, torch.tensor([[2, 1, 0]]), same)[0]) == 2


def test_random_hypotheses_match_the_restatement():
    rng = np.random.RandomState(3)
    toks = rng.randint(0, 7, size=(3, 5, 13))
    toks[:, :, 0] = START
    toks[0, 1] = toks[0, 0]
    w = torch.from_numpy(rng.uniform(0.25, 4.0, size=7).astype(np.float32))
    for N in (1, 2, 3, 4):
        _both(torch.from_numpy(toks), N)
        _both(torch.from_numpy(toks), N, w)
    U1 = consensus_host(torch.from_numpy(toks), END, 4, torch.ones(7))
    assert torch.equal(U1, consensus_host(torch.from_numpy(toks), END, 4))          # all-ones weights: the same bits


# ----------------------------------------------------------------------------------------------------------- decoders
def _expected(hyps, scores, util, end=END):
    """the caption tensor R7 returns for hypotheses (B, K, m + 1) with primary scores (B, K) and utilities (B, K)"""
    picks = [ref.choose(util[b].tolist(), ref.logp_order(scores[b].tolist())) for b in range(hyps.shape[0])]
    caps = [ref.caption(hyps[b, k].tolist(), end) for b, k in enumerate(picks)]
    n = max(len(c) for c in caps)
    return torch.tensor([c + [PAD] * (n - len(c)) for c in caps]), picks


def test_sample_decode_with_consensus():
    B, V, L, n = 4, 9, 8, 6
    model = TableModel(B, V, L + 1, seed=7, scale=2.0)
    fs = _features(B)
    kw = dict(n=n, seed=5, top_k=4)
    base = sample_decode(model, fs, L, START, END, PAD, AV, return_samples=True, **kw)
    same = sample_decode(model, fs, L, START, END, PAD, AV, return_samples=True, select="logp", consensus_n=2, **kw)
    assert len(base) == len(same) == 5 and all(torch.equal(a, b) for a, b in zip(base, same))
    got = sample_decode(model, fs, L, START, END, PAD, AV, return_samples=True, select="consensus", **kw)
    assert len(got) == 6 and all(torch.equal(a, b) for a, b in zip(base[1:], got[1:5]))
    out, samples, sums, util = got[0], got[1], got[2], got[5]
    assert util.shape == (B, n) and util.dtype == torch.float64
    U_ref, _ = ref.utilities(ref.terms(samples.numpy(), END), 4)
    assert np.array_equal(util.numpy(), U_ref)
    want, picks = _expected(samples, sums, util)
    assert torch.equal(out, want)
    assert picks != [ref.logp_order(sums[b].tolist())[0] for b in range(B)]         # the choice differs from rule 7's somewhere
    assert torch.equal(sample_decode(model, fs, L, START, END, PAD, AV, select="consensus", **kw), out)
    # N and the weights reach the utilities
    w = torch.linspace(0.25, 4.0, V)
    for N, cw in ((1, None), (2, w), (4, w.double())):
        g = sample_decode(model, fs, L, START, END, PAD, AV, return_samples=True, select="consensus", consensus_n=N,
                          consensus_weight=cw, **kw)
        U_ref, _ = ref.utilities(ref.terms(samples.numpy(), END, None if cw is None else w.numpy()), N)
        assert np.array_equal(g[5].numpy(), U_ref) and torch.equal(g[0], _expected(samples, sums, g[5])[0])
    one = sample_decode(model, fs, L, START, END, PAD, AV, n=1, seed=5, return_samples=True, select="consensus")
    assert torch.equal(one[5], torch.zeros(B, 1, dtype=torch.float64))
    assert torch.equal(one[0], sample_decode(model, fs, L, START, END, PAD, AV, n=1, seed=5))


def test_beam_decode_with_consensus():
    B, V, L, K = 4, 9, 7, 5
    model = TableModel(B, V, L + 1, seed=3)
    fs = _features(B)
    base = beam_decode(model, fs, L, START, END, PAD, AV, beam_size=K, return_scores=True, return_beams=True)
    same = beam_decode(model, fs, L, START, END, PAD, AV, beam_size=K, return_scores=True, return_beams=True, select="logp")
    assert len(base) == len(same) == 4 and all(torch.equal(a, b) for a, b in zip(base, same))
    got = beam_decode(model, fs, L, START, END, PAD, AV, beam_size=K, return_scores=True, return_beams=True, select="consensus",
                      consensus_n=2)
    assert len(got) == 5 and torch.equal(got[2], base[2]) and torch.equal(got[3], base[3])   # the beams, best first, as ever
    out, score, beams, scores, util = got
    U_ref, _ = ref.utilities(ref.terms(beams.numpy(), END), 2)
    assert np.array_equal(util.numpy(), U_ref)
    picks = [ref.choose(util[b].tolist(), list(range(K))) for b in range(B)]           # the beams arrive in rule 5's order
    caps = [ref.caption(beams[b, k].tolist(), END) for b, k in enumerate(picks)]
    n = max(len(c) for c in caps)
    assert out.tolist() == [c + [PAD] * (n - len(c)) for c in caps]
    assert torch.equal(score, scores[torch.arange(B), torch.tensor(picks)])
    assert any(p != 0 for p in picks)
    assert torch.equal(beam_decode(model, fs, L, START, END, PAD, AV, beam_size=K, select="consensus", consensus_n=2), out)
    # a beam wider than the candidates: the beams that never came alive are hypotheses of pad words (R6)
    wide = beam_decode(TableModel(2, 4, 3, seed=2, scale=2.0), _features(2), 2, START, END, PAD, AV, beam_size=16,
                       return_beams=True, select="consensus")
    assert bool(torch.isinf(wide[2]).any())
    assert np.array_equal(wide[3].numpy(), ref.utilities(ref.terms(wide[1].numpy(), END), 4)[0])


def test_invalid_arguments_are_refused():
    model = TableModel(1, 5, 4)
    fs = _features(1)
    bad = (dict(select="best"), dict(select=None), dict(consensus_n=0), dict(consensus_n=5), dict(consensus_n=1.5),
           dict(consensus_n=True), dict(consensus_n="2"), dict(consensus_weight=[1.0, 2.0]), dict(consensus_weight=torch.ones(2, 3)),
           dict(consensus_weight=torch.ones(5, dtype=torch.int64)), dict(consensus_weight=torch.ones(0)))
    for kw in bad:
        for sel in ({}, dict(select="consensus")):                  # the arguments are checked whatever select says
            kw2 = {**sel, **kw}
            with pytest.raises(ValueError):
                sample_decode(model, fs, 3, START, END, PAD, AV, n=2, **kw2)
            with pytest.raises(ValueError):
                beam_decode(model, fs, 3, START, END, PAD, AV, beam_size=2, **kw2)
            with pytest.raises(ValueError):
                sample_decoder(2, **kw2)
            with pytest.raises(ValueError):
                beam_decoder(2, **kw2)


def test_the_op_has_no_cpu_path():
    from bmhrl_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.consensus(torch.zeros(4, 6, dtype=torch.int64), 5, 2, END)


def test_idf_weights():
    counts = torch.tensor([0, 1, 4, 100, 400])
    w = idf_weights(counts, total=100)
    assert w.dtype == torch.float32 and w.shape == (5,)
    want = [math.log(100.0), math.log(100.0), math.log(25.0), 0.0, 0.0]            # max(1, count); clamped at 0
    assert all(abs(a - b) <= 2.0 ** -23 * max(b, 1.0) for a, b in zip(w.tolist(), want)), w
    assert w[3] == 0 and w[4] == 0
    w2 = idf_weights(counts.float())                                                # total: the sum of the counts
    want2 = [math.log(505.0), math.log(505.0), math.log(505.0 / 4.0), math.log(5.05), math.log(505.0 / 400.0)]
    assert all(abs(a - b) <= 2.0 ** -23 * max(b, 1.0) for a, b in zip(w2.tolist(), want2)), w2
    with pytest.raises(ValueError):
        idf_weights(torch.zeros(3))
    with pytest.raises(ValueError):
        idf_weights(torch.ones(2, 2))


def test_consensus_decoders_drive_predict_1by1():
    from bmhrl_amd.epoch_loops import captioning_bmrl_loops as loops
    from bmhrl_amd.epoch_loops.validation_loops import predict_1by1, tokens_to_sentences
    assert loops.sample_decoder is sample_decoder and loops.beam_decoder is beam_decoder and loops.idf_weights is idf_weights
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
    cfg = SimpleNamespace(max_len=L, modality=AV)
    w = idf_weights(torch.arange(V) * 3)
    for factory, direct in ((sample_decoder(4, top_p=0.9, seed=6, select="consensus", consensus_weight=w),
                             lambda: sample_decode(model, fs, L, START, END, PAD, AV, n=4, top_p=0.9, seed=6, select="consensus",
                                                   consensus_weight=w)),
                            (beam_decoder(3, select="consensus", consensus_n=2),
                             lambda: beam_decode(model, fs, L, START, END, PAD, AV, beam_size=3, select="consensus", consensus_n=2))):
        pred = predict_1by1(cfg, model, Loader([batch]), factory)
        want = tokens_to_sentences(direct().numpy(), itos)
        got = [seg["sentence"] for vid in ("v0", "v1") for seg in pred["results"][vid]]
        assert sorted(got) == sorted(want) and len(got) == B
