"""CPU checks of the caption rewards (bmhrl_amd/rewards.py): the float64 restatement (tests/reward_reference.py) against
the reference scorers' own outputs (tests/golden/rewards.npz, tests/golden/make_reward_golden.py), the string table and
vocab maps, the document-frequency hash table against a precook_corpus dict, and the opt-in metrics.* aliases."""
import random
import sys
import types

import numpy as np
import pytest

from tests import reward_reference as rr


@pytest.fixture(scope="module")
def fx(golden):
    return golden("rewards")


def _case_rows(fx, c):
    n, sigma, one = fx["cases"][c]
    return int(n), float(sigma), fx["hyp1"] if one else fx["hyp"]


def _df(fx):
    return rr.precook_corpus([c.split() for c in fx["corpus"]])


def test_restatement_matches_reference_scorers(fx):
    itos, caps = [str(s) for s in fx["itos"]], [str(s) for s in fx["captions"]]
    gamma = float(fx["gamma"][0])
    df = _df(fx)
    assert len(fx["cases"]) == 8
    for c in range(len(fx["cases"])):
        n, sigma, hyp = _case_rows(fx, c)
        cs = np.stack([rr.cider_scores(itos, row, caps[b], df, n, sigma) for b, row in enumerate(hyp)])
        np.testing.assert_allclose(cs, fx[f"c{c}_cider_rewards"], rtol=1e-12, atol=0)
        bs = np.stack([rr.bleu_scores(itos, row, caps[b], n) for b, row in enumerate(hyp)])
        np.testing.assert_array_equal(bs, fx[f"c{c}_bleu_rewards"])
        np.testing.assert_allclose(rr.discount(rr.delta_row(cs), gamma), fx[f"c{c}_cider_worker"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(rr.discount(rr.delta_row(bs), gamma), fx[f"c{c}_bleu_worker"], rtol=0, atol=1e-6)


def test_fixture_covers_the_quirks(fx):
    """end token first / in the middle / absent / repeated; no-word entries; an empty caption; L = 1; n = 1..4"""
    itos = [str(s) for s in fx["itos"]]
    rows = [[itos[i] for i in r] for r in fx["hyp"]]
    eos_at = [r.index("</s>") if "</s>" in r else None for r in rows]
    assert 0 in eos_at and None in eos_at and any(e not in (None, 0) for e in eos_at)
    assert any(r.count("</s>") > 1 for r in rows)
    assert any(itos[i].split() == [] for r in fx["hyp"] for i in r)
    assert "" in [str(c) for c in fx["captions"]]
    assert fx["hyp1"].shape[1] == 1 and sorted({int(n) for n, _, _ in fx["cases"]}) == [1, 2, 3, 4]
    assert (fx["c0_cider_rewards"][0] == np.float64(np.float32(-0.1))).all()


def test_string_table_and_vocab_maps():
    from bmhrl_amd.rewards import StringTable, vocab_word_ids
    t = StringTable()
    itos = ["<pad>", "Man", " red ", "  ", "", "</s>"]
    for s in itos:
        t.add(s)
        t.add(s.lower())
    for s in itos:
        for w in s.split() + s.lower().split():
            t.add(w)
    raw, low = vocab_word_ids(itos, t, lower=False), vocab_word_ids(itos, t, lower=True)
    assert raw.dtype == np.int32 and raw[1] == t["Man"] and low[1] == t["man"] and raw[1] != low[1]
    assert raw[2] == t["red"] and raw[3] == -1 and raw[4] == -1 and raw[5] == t["</s>"]
    with pytest.raises(ValueError, match="splits into 2 words"):
        vocab_word_ids(["Man", "two words"], t, lower=False)


def test_scorers_refuse_multi_word_vocab_entries():
    from bmhrl_amd.rewards import BleuScorer, CiderScorer
    vocab = types.SimpleNamespace(itos=["<pad>", "</s>", "a b"])
    with pytest.raises(ValueError):
        CiderScorer(vocab, [["a"]], "cpu", 0.9, 0.9)
    with pytest.raises(ValueError):
        BleuScorer(vocab, "cpu", 0.9, 0.9)


def test_doc_frequency_table_matches_precook_corpus():
    from bmhrl_amd.rewards import DocFrequency, StringTable
    rng = random.Random(7)
    words = [f"w{i}" for i in range(60)] + ["A", "a"]
    corpus = [[rng.choice(words[:12] if rng.random() < 0.5 else words) for _ in range(rng.randint(0, 14))] for _ in range(400)]
    corpus.append("abab")                    # a string caption is sliced into characters, as precook_corpus does
    ref = rr.precook_corpus(corpus)
    t = StringTable()
    df = DocFrequency(iter(corpus), t)
    assert df.grams.shape[0] == len(ref) and df.cap >= 2 * len(ref) and df.cap & (df.cap - 1) == 0
    for gram, cnt in ref.items():
        assert df.lookup([t[w] for w in gram]) == np.log(max(1.0, cnt))
    # misses: grams counted once, never seen, or made of words outside the table
    counts = {}
    for cap in corpus:
        for k in range(1, 5):
            for i in range(len(cap) - k + 1):
                counts[tuple(cap[i:i + k])] = counts.get(tuple(cap[i:i + k]), 0) + 1
    once = [g for g, c in counts.items() if c == 1][:200]
    assert once
    for gram in once:
        assert df.lookup([t[w] for w in gram]) == 0.0
    assert df.lookup([len(t) + 5]) == 0.0 and df.lookup([t["w1"], len(t) + 1, t["w2"]]) == 0.0


def test_install_registers_metrics_modules_only():
    import bmhrl_amd.install as inst
    from bmhrl_amd import rewards
    before = dict(inst.ALIASES)
    saved = {k: sys.modules.get(k) for k in ("metrics", "metrics.cider", "metrics.bleu")}
    try:
        for k in saved:
            sys.modules.pop(k, None)
        assert rewards.install() == ["metrics.cider", "metrics.bleu"]
        from metrics.cider import CiderScorer
        from metrics.bleu import BleuScorer
        assert CiderScorer is rewards.CiderScorer and BleuScorer is rewards.BleuScorer
        assert inst.ALIASES == before and not any(k.startswith("metrics") for k in inst.ALIASES)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
