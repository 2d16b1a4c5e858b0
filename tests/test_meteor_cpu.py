"""CPU checks of the METEOR rewards: the plain-Python restatement (tests/meteor_reference.py) against
the values nltk documents, its edge cases, the host tables of bmhrl_amd/rewards.py MeteorTables, install(), and what the
random cases shared with tests/test_meteor_gpu.py exercise."""
import sys
import types

import numpy as np
import pytest

from tests import meteor_reference as mr

HYP1 = "It is a guide to action which ensures that the military always obeys the commands of the party"
REF1 = "It is a guide to action that ensures that the military will forever heed Party commands"


def same(word):
    return word


def always_forever(word):
    return ["forever"] if word == "always" else []


def test_documented_values():
    """nltk's docstrings: 0.7398 for the first pair (the only synonym hit is always -> forever), 0.5 and 0.0"""
    assert abs(mr.meteor_sentence(HYP1, REF1, same, always_forever) - 0.7398275988019579) <= 1e-15
    assert round(mr.meteor_sentence(HYP1, REF1, same, always_forever), 4) == 0.7398
    assert abs(mr.meteor_sentence(HYP1, REF1) - 0.6944444444444445) <= 1e-15
    assert abs(mr.meteor_sentence("on the mat sat the cat", "the cat sat on the mat") - 0.5) <= 1e-15
    assert mr.meteor_sentence("non matching hypothesis", "this is a cat") == 0.0


def test_prefix_scores_are_not_monotone():
    words = HYP1.split()
    s = [mr.meteor_sentence(" ".join(words[:l + 1]), REF1, same, always_forever) for l in range(len(words))]
    assert len(s) == 18 and s[-1] == mr.meteor_sentence(HYP1, REF1, same, always_forever)
    falls = [l for l in range(1, 18) if s[l] < s[l - 1]]
    assert {6, 12, 13} <= set(falls) and falls == [6, 12, 13, 15, 16]      # which, obeys, ... and the unmatched of, the


def test_empty_sides_give_zeros():
    itos = ["", " ", "a", "b"]
    assert (mr.meteor_scores(itos, [2, 3, 2], "") == 0).all()                  # empty reference
    assert (mr.meteor_scores(itos, [0, 1, 0], "a b") == 0).all()               # a row without a word
    assert mr.meteor_prefix([], ["a"]) == 0.0 and mr.meteor_prefix([], []) == 0.0
    s = mr.meteor_scores(itos, [0, 2, 1, 3], "a b")                            # a no-word position repeats the score before it
    assert s[0] == 0 and s[1] > 0 and s[2] == s[1] and s[3] > s[2]
    assert (mr.meteor_scores(itos, [-1, 4, 2], "a") == [0, 0, 1 * mr.meteor_prefix(["a"], ["a"])]).all()


def test_a_repeated_word_moves_between_prefixes():
    """the walk starts at the prefix's last word: "a" alone takes the last reference "a", with a second "a" behind it the
    first one"""
    m1, _ = mr.align(["a"], ["a", "x", "a"])
    m2, _ = mr.align(["a", "a"], ["a", "x", "a"])
    assert m1 == [(0, 2)] and m2 == [(0, 0), (1, 2)]
    assert mr.count_chunks(m2) == 2 and mr.count_chunks(mr.align(["a", "a"], ["a", "a"])[0]) == 1
    # stages run on what is left: the exact stage takes walk and large, the stem stage pairs walks -> walked, the synonym
    # stage big -> huge; large -> huge is no match (the set belongs to the hypothesis word)
    st = mr.DictStemmer().stem
    m, counts = mr.align(["walks", "walk", "big", "large"], ["walk", "walked", "large", "huge"], st, mr.dict_synonyms)
    assert counts == [2, 1, 1] and m == [(0, 1), (1, 0), (2, 3), (3, 2)]
    m, counts = mr.align(["big"], ["huge", "great"], st, mr.dict_synonyms)
    assert m == [(0, 1)] and counts == [0, 0, 1]
    assert mr.align(["large"], ["huge"], st, mr.dict_synonyms)[0] == []


# ---- host tables
ITOS = ["<unk>", "", " ", "Walks", "walk", "big", "large", "cat", "jumped"]


def _tables(**kw):
    from bmhrl_amd.rewards import MeteorTables
    kw.setdefault("stemmer", mr.DictStemmer())
    kw.setdefault("synonyms", mr.dict_synonyms)
    return MeteorTables(ITOS, **kw)


def test_host_tables():
    t = _tables()
    assert t.vmap.dtype == np.int32 and t.vstem.dtype == np.int32 and t.syn_off.dtype == np.int32 and t.syn_ids.dtype == np.int32
    assert list(t.vmap[:3]) == [t.strings["<unk>"], -1, -1] and t.vmap[3] == t.strings["walks"]
    # stems: Walks and walk share one, words without a rule are their own stem, no word -> -1
    assert t.vstem[3] == t.vstem[4] == t.stems["walk"] and t.vstem[8] == t.stems["jump"] and t.vstem[7] == t.stems["cat"]
    assert list(t.vstem[1:3]) == [-1, -1]
    # CSR rows: ascending distinct word ids of what `synonyms` returned -- the word itself only when it was returned
    assert t.syn_off[0] == 0 and len(t.syn_off) == len(ITOS) + 1 and t.syn_off[-1] == len(t.syn_ids)
    row = lambda v: list(t.syn_ids[t.syn_off[v]:t.syn_off[v + 1]])                                        # noqa: E731
    assert row(5) == sorted(t.strings[w] for w in ("large", "huge", "great")) and t.strings["big"] not in row(5)
    assert row(4) == sorted(t.strings[w] for w in ("stroll", "walk")) and t.strings["walk"] in row(4)
    assert row(6) == [t.strings["big"]] and row(7) == [t.strings["feline"]] and row(0) == row(1) == row(3) == []
    # a synonym outside the vocabulary is in the word table, so the reference word gets that id; others are fresh
    words, stems = t.encode(["Great cat zebra zebras", "", "zebras walker"])
    n, ns = len(t.strings), len(t.stems)
    assert words[0] == [t.strings["great"], t.strings["cat"], n, n + 1] and words[1] == [] and words[2] == [n + 1, n + 2]
    assert stems[0] == [ns, t.stems["cat"], ns + 1, ns + 2] and stems[2] == [ns + 2, t.stems["walk"]]
    assert len(t.strings) == n and len(t.stems) == ns                             # fresh ids are per batch
    with pytest.raises(ValueError):
        t.encode(["w " * 513])


def test_stages_switch_off():
    t = _tables(stemmer=False)
    assert t.vstem is None and t.syn_off is not None
    assert t.encode(["walk zebra"])[1] == [[-1, -1]]
    t = _tables(synonyms=False)
    assert t.syn_off is None and t.syn_ids is None and t.vstem is not None
    t = _tables(synonyms=lambda w: [])
    assert t.syn_off[-1] == 0 and len(t.syn_ids) == 1                              # never an empty array: no null pointer


def test_multi_word_entry_is_refused():
    from bmhrl_amd.rewards import MeteorTables
    with pytest.raises(ValueError, match="splits into 2 words"):
        MeteorTables(ITOS + ["two words"], mr.DictStemmer(), mr.dict_synonyms)


def test_defaults_need_nltk(monkeypatch):
    from bmhrl_amd.rewards import MeteorTables
    for name in ("nltk", "nltk.stem", "nltk.stem.porter", "nltk.corpus"):
        monkeypatch.setitem(sys.modules, name, None)            # importing it raises ImportError
    for kw in ({}, {"synonyms": False}, {"stemmer": False}, {"stemmer": mr.DictStemmer()}, {"synonyms": mr.dict_synonyms}):
        with pytest.raises(ImportError, match="stemmer=.*synonyms="):
            MeteorTables(ITOS, **kw)
    MeteorTables(ITOS, stemmer=False, synonyms=False)


def test_install_registers_meteor_on_request():
    from bmhrl_amd import rewards
    saved = {k: sys.modules.get(k) for k in ("metrics", "metrics.cider", "metrics.bleu", "metrics.batched_meteor")}
    try:
        for k in saved:
            sys.modules.pop(k, None)
        assert rewards.install() == ["metrics.cider", "metrics.bleu"]
        assert "metrics.batched_meteor" not in sys.modules
        assert rewards.install(meteor=True) == ["metrics.cider", "metrics.bleu", "metrics.batched_meteor"]
        from metrics.batched_meteor import MeteorScorer, segment_reward
        from bmhrl_amd import rl_glue
        assert MeteorScorer is rewards.MeteorScorer and segment_reward is rl_glue.segment_reward
        assert MeteorScorer.type == "METEOR"
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


# ---- the random cases of the GPU test
@pytest.mark.parametrize("seed", [3, 7])
def test_random_cases_cover_the_ground(seed):
    itos, caps, hyp = mr.random_case(seed)
    assert hyp.shape == (32, 30) and 35 <= len(itos) <= 45 and "" in itos and " " in itos
    assert any(s != s.lower() for s in itos) and max(len(c.split()) for c in caps) <= 20
    cov = mr.coverage(itos, caps, hyp, mr.DictStemmer().stem, mr.dict_synonyms)
    assert all(n >= 1 for n in cov["stages"]), cov
    assert cov["max_chunks"] >= 3 and cov["empty"] >= 1 and cov["disagree"] >= 1, cov
    # the tables built for these cases hold every stem and synonym cluster
    from bmhrl_amd.rewards import MeteorTables
    t = MeteorTables(itos, mr.DictStemmer(), mr.dict_synonyms)
    assert len(set(t.vstem[t.vstem >= 0].tolist())) < (t.vmap >= 0).sum() and t.syn_off[-1] > 10


def test_reduced_form_equals_the_pop_loops():
    """"highest unmatched reference position, hypothesis words from last to first" is what the pop loops do: bit-equal rows"""
    itos, caps, hyp = mr.random_case(7)
    st = mr.DictStemmer().stem
    for stem, syn in ((None, None), (st, None), (None, mr.dict_synonyms), (st, mr.dict_synonyms)):
        for b, row in enumerate(hyp.tolist()):
            a = mr.meteor_scores(itos, row, caps[b], stem, syn)
            assert np.array_equal(a, mr.meteor_scores_reduced(itos, row, caps[b], stem, syn)), (b, stem, syn)
    row = [-1, 6, len(itos), 7, 4, 6]
    assert np.array_equal(mr.meteor_scores(itos, row, "a the a"), mr.meteor_scores_reduced(itos, row, "a the a"))


# ---- optional: nltk's own function
class _FakeLemma:
    def __init__(self, name):
        self._name = name

    def name(self):
        return self._name


class _FakeSynset:
    def __init__(self, names):
        self._names = names

    def lemmas(self):
        return [_FakeLemma(n) for n in self._names]


class _FakeWordnet:
    def synsets(self, word):
        names = mr.dict_synonyms(word)
        return [_FakeSynset(names)] if names else []


def test_restatement_matches_nltk():
    pytest.importorskip("nltk")
    from nltk.translate.meteor_score import single_meteor_score
    itos, caps, hyp = mr.random_case(3, B=8)
    stemmer = mr.DictStemmer()
    for b, row in enumerate(hyp.tolist()):
        words = [itos[i] for i in row]
        for l in range(len(words)):
            h = " ".join(words[:l + 1])
            got = mr.meteor_sentence(h, caps[b], stemmer.stem, mr.dict_synonyms)
            want = single_meteor_score(caps[b], h, stemmer=stemmer, wordnet=_FakeWordnet())
            assert abs(got - want) <= 1e-15, (b, l, got, want)
