"""Runs the reference's own ANETcaptions (evaluation/evaluate.py) on two small ground-truth files and one submission and
writes tests/golden/caption_eval.json: the inputs, the pairs it formed and its .scores at tIoU 0.3, 0.5, 0.7 and 0.9.

evaluate.py imports pycocoevalcap (Java PTB tokenizer, METEOR jar), which is not in the reference checkout.  Stand-ins
written for this generator are put into sys.modules instead:
  tokenizer  bmhrl_amd.evaluate.tokenize, joined with spaces (what the device evaluator uses);
  Bleu       pycocoevalcap's calling sequence around the reference's own BleuScorerObj (metrics/bleu.py);
  Cider      pycocoevalcap's calling sequence and document frequencies around the reference's own CiderScorerObj
             (metrics/cider.py), values times 10;
  Rouge, Meteor   tests/caption_eval_reference.py (ROUGE-L; nltk-3.5 METEOR with the stub stemmer and synonym table of
             tests/meteor_reference.py), mean over the pairs.
metrics/*.py import nltk and tqdm without using them here: empty stand-in modules let them import.  ANETcaptions iterates
a set of video ids and draws random garbage references; the generator sorts the ids and seeds `random`, so a rerun
reproduces the file byte for byte.
usage: make_caption_eval_golden.py REFERENCE_CHECKOUT"""
import contextlib
import io
import json
import os
import random
import sys
import tempfile
import types
from collections import defaultdict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "caption_eval.json")
TIOUS = [0.3, 0.5, 0.7, 0.9]
MAX_PROPOSALS = 5


def gt(duration, *segments):
    return {"duration": duration, "timestamps": [[s, e] for s, e, _ in segments], "sentences": [c for _, _, c in segments]}


# v07: no predictions; v08, v09, v11: first file only; v10: second file only; p99 (submission): no ground truth
GT_1 = {
    "v01": gt(60.0, (0.0, 20.0, "A man is playing a guitar on stage."), (20.0, 60.0, "The crowd claps and the man walks away.")),
    "v02": gt(90.0, (0.0, 50.0, "A big dog runs on the grass."), (10.0, 60.0, "The dog jumps and plays with a ball."),
              (60.0, 90.0, "A woman walks with the dog.")),
    "v03": gt(30.0, (0.0, 10.0, "A cat sits in a small box.")),
    "v04": gt(45.5, (5.0, 25.0, "Two men are playing cards."), (25.0, 45.5, "One man walked away from the table.")),
    "v05": gt(80.0, (0.0, 40.0, "A woman drinks coffee in a café."), (40.0, 80.0, "She reads a naïve little book — slowly.")),
    "v06": gt(120.0, (0.0, 30.0, "A man is walking fast."), (30.0, 70.0, "The man jumps on a large rock."),
              (70.0, 120.0, "He walks and the dogs play.")),
    "v07": gt(20.0, (0.0, 20.0, "Nobody predicted this one.")),
    "v08": gt(50.0, (0.0, 25.0, "A quick cat jumps on the man."), (25.0, 50.0, "The cats play.")),
    "v09": gt(40.0, (0.0, 10.0, "The the the cat."), (5.0, 40.0, "a man , a dog ; and the cat !")),
    "v11": gt(33.3, (1.0, 30.0, "WALKING in THE park... with a Dog -- fast")),
}
GT_2 = {
    "v01": gt(60.0, (0.0, 25.0, "A man plays the guitar."), (22.0, 58.0, "People clap.")),
    "v02": gt(90.0, (5.0, 55.0, "A large dog is running in a field."), (58.0, 90.0, "A woman and the dog walk.")),
    "v03": gt(30.0, (0.0, 12.0, "A little cat is in a box."), (12.0, 30.0, "The cat jumped.")),
    "v04": gt(45.5, (0.0, 30.0, "Men play cards on a table.")),
    "v05": gt(80.0, (0.0, 80.0, "A woman is in a café and reads.")),
    "v06": gt(120.0, (0.0, 60.0, "A man walks and jumps."), (60.0, 120.0, "Dogs are playing with the man.")),
    "v10": gt(25.0, (0.0, 12.5, "A huge rock."), (12.5, 25.0, "A man walked on the big rock.")),
}


def seg(start, end, sentence):
    return {"sentence": sentence, "timestamp": [start, end]}


SUBMISSION = {
    "version": "VERSION 1.0",
    "external_data": {"used": True, "details": ""},
    "results": {
        "v01": [seg(0.0, 22.0, "A man is playing a guitar"), seg(21.0, 59.0, "The crowd claps")],
        "v02": [seg(4.0, 56.0, "A large dog plays on the grass"), seg(61.0, 88.0, "A woman is walking with a dog")],   # two overlaps
        "v03": [seg(20.0, 29.0, "The cat jumps"), seg(0.0, 11.0, "A small cat sits in the box")],
        "v04": [seg(6.0, 26.0, ""), seg(24.0, 45.0, "A man walks away")],                                  # an empty sentence
        "v05": [seg(0.0, 42.0, "A woman drinks café coffee"), seg(38.0, 80.0, "She reads a book … slowly")],   # non-ASCII
        "v06": [seg(0.0, 30.0, "A man walks fast"), seg(31.0, 69.0, "The man jumped on a big rock"),       # > MAX_PROPOSALS
                seg(70.0, 119.0, "He walks and the dog plays"), seg(0.0, 61.0, "A man is walking and jumping"),
                seg(100.0, 110.0, "Dogs"), seg(0.0, 120.0, "cut off by max proposals"), seg(0.0, 30.0, "cut off too")],
        "v08": [seg(30.0, 31.0, "Nothing overlaps this"), seg(0.0, 24.0, "A fast cat jumps on a man")],   # overlaps nothing
        "v09": [seg(0.0, 9.0, "The the the"), seg(4.0, 40.0, "A man, a dog and the cat.")],
        "v10": [seg(0.0, 12.0, "A big rock"), seg(12.0, 25.0, "A man walks on a large rock")],
        "v11": [seg(0.0, 31.0, "Walking in the park with a dog")],
        "p99": [seg(0.0, 10.0, "No ground truth for this video")],
    },
}


def mod(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def stub_modules(record):
    unused = lambda *a, **k: None           # noqa: E731
    mod("nltk")
    mod("nltk.translate", meteor=unused)
    mod("nltk.translate.meteor_score", meteor_score=unused, single_meteor_score=unused)
    mod("nltk.tokenize")
    mod("nltk.tokenize.treebank", TreebankWordDetokenizer=type("TreebankWordDetokenizer", (), {}))
    mod("tqdm", tqdm=unused)
    from metrics.bleu import BleuScorerObj
    from metrics.cider import CiderScorerObj
    from bmhrl_amd.evaluate import tokenize
    from tests import caption_eval_reference as restatement
    from tests.meteor_reference import DictStemmer, dict_synonyms

    class PTBTokenizer:
        def tokenize(self, captions):
            record(captions)
            return {i: [" ".join(tokenize(c["caption"])) for c in caps] for i, caps in captions.items()}

    def check(gts, res):
        assert list(gts.keys()) == list(res.keys())
        for i in gts:
            assert len(res[i]) == 1 and len(gts[i]) == 1
        return list(gts.keys())

    class Bleu:
        def __init__(self, n=4):
            self._n = n

        def compute_score(self, gts, res):
            scorer = BleuScorerObj(n=self._n)
            for i in check(gts, res):
                scorer += (res[i][0], gts[i])
            _, bleus = scorer.compute_score(option="closest", verbose=0)
            return bleus, None

        def method(self):
            return "Bleu"

    class Cider:
        def compute_score(self, gts, res):
            scorer = CiderScorerObj(defaultdict(float), n=4, sigma=6.0)
            for i in check(gts, res):
                scorer += (res[i][0], gts[i][0])
            for refs in scorer.crefs:           # document frequencies the pycocoevalcap way
                for ngram in set(ngram for ref in refs for ngram in ref):
                    scorer.document_frequency[ngram] += 1
            per_pair = [float(s) * 10.0 for s in scorer.compute_cider()]
            return restatement.mean(per_pair), np.array(per_pair)

        def method(self):
            return "CIDEr"

    class Rouge:
        def compute_score(self, gts, res):
            per_pair = [restatement.rouge_pair(res[i][0].split(), gts[i][0].split()) for i in check(gts, res)]
            return restatement.mean(per_pair), np.array(per_pair)

        def method(self):
            return "Rouge"

    class Meteor:
        def compute_score(self, gts, res):
            stem = DictStemmer().stem
            per_pair = [restatement.meteor_pair(res[i][0].split(), gts[i][0].split(), stem, dict_synonyms)
                        for i in check(gts, res)]
            return restatement.mean(per_pair), per_pair

        def method(self):
            return "METEOR"

    mod("pycocoevalcap")
    mod("pycocoevalcap.tokenizer")
    mod("pycocoevalcap.tokenizer.ptbtokenizer", PTBTokenizer=PTBTokenizer)
    for name, cls in (("bleu", Bleu), ("meteor", Meteor), ("rouge", Rouge), ("cider", Cider)):
        mod(f"pycocoevalcap.{name}")
        mod(f"pycocoevalcap.{name}.{name}", **{cls.__name__: cls})


def main(reference):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, reference)
    calls = []
    stub_modules(calls.append)
    from evaluation.evaluate import ANETcaptions
    from bmhrl_amd.evaluate import remove_nonascii
    random.seed(0)
    with tempfile.TemporaryDirectory() as tmp:
        paths = []
        for name, obj in (("gt_1.json", GT_1), ("gt_2.json", GT_2), ("submission.json", SUBMISSION)):
            paths.append(os.path.join(tmp, name))
            with open(paths[-1], "w") as f:
                json.dump(obj, f)
        with contextlib.redirect_stdout(io.StringIO()):
            ev = ANETcaptions(paths[:2], paths[2], TIOUS, MAX_PROPOSALS, ["results", "version", "external_data"], True, False)
            ev.get_gt_vid_ids = lambda: sorted(ev.n_ref_vids)
            ev.evaluate()
    # the pairs of every tIoU, as the tokenizer first saw them: (prediction, reference), a garbage reference as null
    known = {remove_nonascii(s) for g in (GT_1, GT_2) for v in g.values() for s in v["sentences"]}
    per_tiou = len(calls) // len(TIOUS)      # one (res, gts) couple of calls per scorer
    pairs = []
    for t in range(len(TIOUS)):
        res, gts = calls[t * per_tiou], calls[t * per_tiou + 1]
        pairs.append([[res[i][0]["caption"], gts[i][0]["caption"] if gts[i][0]["caption"] in known else None] for i in res])
    out = {"ground_truths": [GT_1, GT_2], "submission": SUBMISSION, "max_proposals": MAX_PROPOSALS, "tious": TIOUS,
           "meteor": "tests.meteor_reference DictStemmer / dict_synonyms", "pairs": pairs,
           "scores": {k: [float(x) for x in v] for k, v in ev.scores.items()}}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
