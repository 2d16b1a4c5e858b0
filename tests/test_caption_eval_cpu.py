"""The host half of the dense-captioning evaluator (bmhrl_amd/evaluate.py) without a GPU: the float64
restatement (tests/caption_eval_reference.py) against the fixture recorded from the reference's ANETcaptions
(tests/golden/caption_eval.json) and against the hand-checked four pairs, the pairing and detection helpers against the
fixture, the tokenizer, the constructor's refusals and the loop's unchanged behaviour without an evaluator."""
import json
import os
import sys
from types import SimpleNamespace

import pytest

from tests import caption_eval_reference as cr
from tests.conftest import GOLDEN
from tests.meteor_reference import DictStemmer, dict_synonyms


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLDEN, "caption_eval.json")) as f:
        return json.load(f)


def rel(a, b):
    return abs(a - b) / abs(b) if b else abs(a)


def test_restatement_reproduces_the_hand_checked_pairs():
    got = cr.bleu_group(cr.HAND_PAIRS)
    assert all(rel(g, w) <= 1e-12 for g, w in zip(got, cr.HAND_BLEU)), got
    per_pair = cr.cider_pairs(cr.HAND_PAIRS)
    assert all(rel(g, w) <= 1e-12 for g, w in zip(per_pair, cr.HAND_CIDER_PAIRS)), per_pair
    assert per_pair[2] == 0.0 and per_pair[3] == 0.0
    assert rel(cr.mean(per_pair), cr.HAND_CIDER) <= 1e-12
    assert [cr.lcs(h, r) for h, r in cr.HAND_PAIRS] == cr.HAND_LCS
    rouge = [cr.rouge_pair(h, r) for h, r in cr.HAND_PAIRS]
    assert all(rel(g, w) <= 1e-12 for g, w in zip(rouge, cr.HAND_ROUGE)), rouge


def test_restatement_cider_consequences():
    one = [("a man sits".split(), "a man sits down".split())]
    assert cr.cider_pairs(one) == [0.0]                         # one pair: every weight is 0
    # "the" is in every reference: weight 0, so a hypothesis sharing only "the" scores 0 against any of them
    pairs = [("the".split(), "the cat".split()), ("a dog".split(), "the dog".split())]
    assert cr.cider_pairs(pairs)[0] == 0.0 and cr.cider_pairs(pairs)[1] > 0.0


def test_restatement_reproduces_the_fixture(fixture):
    from bmhrl_amd.evaluate import tokenize
    got = cr.evaluate(fixture["ground_truths"], fixture["submission"], fixture["tious"], fixture["max_proposals"], tokenize,
                      DictStemmer().stem, dict_synonyms)
    assert sorted(got) == sorted(fixture["scores"])
    for name, want in fixture["scores"].items():
        assert len(got[name]) == len(want) == 4
        for g, w in zip(got[name], want):
            assert rel(g, w) <= 1e-12, (name, g, w)


def test_fixture_covers_its_cases(fixture):
    gts, sub = fixture["ground_truths"], fixture["submission"]["results"]
    ids = [set(g) for g in gts]
    assert ids[0] - ids[1] and ids[1] - ids[0]                                   # a video in one file only, both ways
    assert (ids[0] | ids[1]) - set(sub)                                          # a video without predictions
    assert set(sub) - (ids[0] | ids[1])                                          # a prediction-only video
    assert any(len(v) > fixture["max_proposals"] for v in sub.values())          # a list longer than max_proposals
    assert all(len(v) > 0 for v in sub.values())                                 # no empty prediction list
    sentences = [s["sentence"] for v in sub.values() for s in v]
    assert "" in sentences and any(ord(c) > 127 for s in sentences for c in s)
    assert any(ord(c) > 127 for g in gts for v in g.values() for s in v["sentences"] for c in s)
    for pairs in fixture["pairs"]:
        assert any(r is None for _, r in pairs)                                  # a prediction overlapping none
    assert any(sum(1 for h, _ in fixture["pairs"][0] if h == hyp) >= 2 for hyp, _ in fixture["pairs"][0])   # ... two


def test_pairing_and_detection_reproduce_the_fixture(fixture):
    from bmhrl_amd.evaluate import detection_scores, ground_truth_video_ids, pair_captions
    gts = fixture["ground_truths"]
    prediction = {v: s[:fixture["max_proposals"]] for v, s in fixture["submission"]["results"].items()}
    for t, tiou in enumerate(fixture["tious"]):
        paired = pair_captions(gts, prediction, tiou)
        assert list(paired) == ground_truth_video_ids(gts) == sorted(set(gts[0]) | set(gts[1]))
        flat = [[h, r] for v in paired for h, r in paired[v]]
        assert flat == fixture["pairs"][t]
        assert flat == [[h, r] for v, ps in cr.pairs_of(gts, prediction, tiou).items() for h, r in ps]
        precision, recall = detection_scores(gts, prediction, tiou)
        assert rel(precision, fixture["scores"]["Precision"][t]) <= 1e-12
        assert rel(recall, fixture["scores"]["Recall"][t]) <= 1e-12
        assert (precision, recall) == cr.detection(gts, prediction, tiou)
    # an empty prediction list counts precision 0 for that file (the reference's stale pred_i is not kept)
    gt = {"v": {"timestamps": [[0, 10]], "sentences": ["x"]}, "w": {"timestamps": [[0, 10]], "sentences": ["y"]}}
    pred = {"v": [{"sentence": "x", "timestamp": [0, 10]}], "w": []}
    assert detection_scores([gt], pred, 0.5) == (0.5, 0.5) == cr.detection([gt], pred, 0.5)
    assert pair_captions([gt], pred, 0.5) == {"v": [("x", "x")], "w": []}


def test_tiou_keeps_the_reference_arithmetic():
    from bmhrl_amd.evaluate import tiou
    assert tiou([0, 10], [0, 10]) == 10.0 / (10 + 1e-8) < 1.0
    assert tiou([0, 10], [20, 30]) == 0.0
    assert tiou([0, 10], [5, 15]) == 5.0 / (15 + 1e-8)
    assert tiou([0, 1], [0, 2]) == cr.iou([0, 1], [0, 2])


def test_tokenizer():
    from bmhrl_amd.evaluate import remove_nonascii, tokenize
    assert tokenize("") == [] and tokenize("   ") == []
    assert tokenize("?!. , -- ... ; : ' `") == []
    assert tokenize("A Man, playing the GUITAR.") == ["a", "man", "playing", "the", "guitar"]
    assert tokenize("a man's dog (big) & 2 cats") == ["a", "man", "s", "dog", "(", "big", ")", "&", "2", "cats"]
    assert remove_nonascii("café — ok") == "caf    ok"
    assert tokenize(remove_nonascii("A woman in a café — reads…")) == ["a", "woman", "in", "a", "caf", "reads"]


def test_constructor_refusals_and_proposal_only_scores(fixture, tmp_path, monkeypatch):
    from bmhrl_amd.evaluate import GARBAGE, DenseCaptionEvaluator
    gts, sub = fixture["ground_truths"], fixture["submission"]
    with pytest.raises(IOError, match="tIoU"):
        DenseCaptionEvaluator(gts, sub, [], only_proposals=True)
    with pytest.raises(IOError, match="ground truth"):
        DenseCaptionEvaluator([], sub, [0.5], only_proposals=True)
    with pytest.raises(IOError, match="prediction"):
        DenseCaptionEvaluator(gts, None, [0.5], only_proposals=True)
    with pytest.raises(IOError):
        DenseCaptionEvaluator([str(tmp_path / "missing.json")], sub, [0.5], only_proposals=True)
    with pytest.raises(IOError):
        DenseCaptionEvaluator(gts, str(tmp_path / "missing.json"), [0.5], only_proposals=True)
    with pytest.raises(IOError):
        DenseCaptionEvaluator(gts, {"results": {}}, [0.5], only_proposals=True)      # version, external_data missing
    paths = []
    for name, obj in (("a.json", gts[0]), ("b.json", gts[1]), ("s.json", sub)):
        paths.append(str(tmp_path / name))
        with open(paths[-1], "w") as f:
            json.dump(obj, f)
    ev = DenseCaptionEvaluator(paths[:2], paths[2], fixture["tious"], fixture["max_proposals"], verbose=True,
                               only_proposals=True)
    assert all(len(v) <= fixture["max_proposals"] for v in ev.prediction.values())
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        ev.evaluate()
    assert sorted(ev.scores) == ["Precision", "Recall"]
    for name in ("Precision", "Recall"):
        assert all(rel(g, w) <= 1e-12 for g, w in zip(ev.scores[name], fixture["scores"][name]))
    quiet = DenseCaptionEvaluator(gts, sub, [0.5], only_proposals=True)
    quiet.evaluate()
    assert quiet.scores == {}
    # nltk's stemmer and synonyms are the defaults: without nltk the error names the two keywords
    for name in ("nltk", "nltk.stem", "nltk.stem.porter", "nltk.corpus"):
        monkeypatch.setitem(sys.modules, name, None)
    with pytest.raises(ImportError, match="stemmer=.*synonyms="):
        DenseCaptionEvaluator(gts, sub, [0.5])
    ev = DenseCaptionEvaluator(gts, sub, [0.5], stemmer=False, synonyms=False)        # both stages off: no nltk needed
    assert ev.meteor_tables().vstem is None and ev.meteor_tables().syn_off is None
    # the tokenizer is a parameter; groups are the sorted ground-truth videos, those without a pair included
    ev = DenseCaptionEvaluator(gts, sub, [0.5], fixture["max_proposals"], tokenizer=str.split, stemmer=False, synonyms=False)
    vids, off, hyps, refs = ev.tokenized_pairs(0.5)
    assert vids == sorted(set(gts[0]) | set(gts[1])) and len(off) == len(vids) + 1 and off[-1] == len(hyps) == len(refs)
    assert [list(h) for h in hyps] == [h.split() for h, _ in fixture["pairs"][1]]
    assert [list(r) for r in refs] == [[GARBAGE] if r is None else r.split() for _, r in fixture["pairs"][1]]
    assert off[vids.index("v07") + 1] == off[vids.index("v07")]                     # no predictions: an empty group
    # nothing predicted for any ground-truth video: zeros, and no launch (this runs without a GPU)
    only = dict(sub, results={"p99": sub["results"]["p99"]})
    ev = DenseCaptionEvaluator(gts, only, [0.3, 0.5], stemmer=False, synonyms=False)
    ev.evaluate()
    assert sorted(ev.scores) == sorted(["Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "METEOR", "ROUGE_L", "CIDEr"])
    assert all(v == [0.0, 0.0] for v in ev.scores.values())


def test_loop_without_the_keyword_still_returns_the_predictions(tmp_path):
    import torch
    from bmhrl_amd.epoch_loops.validation_loops import calculate_metrics, validation_1by1_loop
    itos = ["<unk>", "<blank>", "<s>", "</s>", "a", "man", "runs", "fast"]
    ds = SimpleNamespace(start_idx=2, end_idx=3, pad_idx=1, phase="val_1", train_vocab=SimpleNamespace(itos=itos),
                         update_iterator=lambda: None)

    class Loader(list):
        dataset = ds
    batches = [dict(feature_stacks={}, video_ids=["v1", "v2"], starts=torch.tensor([[0.0], [1.5]]),
                    ends=torch.tensor([[2.0], [3.5]]))]
    model = SimpleNamespace(eval=lambda: None)
    cfg = SimpleNamespace(max_len=4, modality="audio_video", log_path=str(tmp_path), reference_paths=["r1", "r2", "r3", "r4"],
                          max_prop_per_vid=100, tIoUs=[0.3, 0.5, 0.7, 0.9])
    decoder = lambda *a: torch.tensor([[2, 4, 5, 3, 1], [2, 6, 7, 7, 7]])                     # noqa: E731
    out = validation_1by1_loop(cfg, model, Loader(batches), decoder, 3, None)
    assert out["submission_path"] == str(tmp_path / "captioning_results_val_1_e3.json")
    assert out["results"]["v1"] == [{"sentence": "A man", "timestamp": [0.0, 2.0]}]
    cfg.caption_evaluator = None                                                             # None in the config: the same
    out = validation_1by1_loop(cfg, model, Loader(batches), decoder, 4, None)
    assert out["submission_path"] == str(tmp_path / "captioning_results_val_1_e4.json")
    with pytest.raises(ValueError, match="unknown caption evaluator"):
        calculate_metrics(["r1"], out["submission_path"], [0.5], 100, evaluator="java")
