"""Device dense-captioning evaluation (bmhrl_amd/evaluate.py, csrc/caption_eval.hip): one JSON line for a synthetic
ActivityNet-sized job -- 4 900 videos (--videos), two ground-truth files with 3-4 captions per video of 8..20 words
(Zipf-like draws from 10 000 words), scored
- "gt_props": once with the first file's own segments as proposals (one sentence each, half of its words redrawn), tIoU 0.5;
- "props100": once with 100 proposals per video (--proposals; random segments, sentences of 6..16 words), tIoUs 0.3 / 0.5 /
  0.7 / 0.9.
Per job: the host pairing time (pair_captions), the tokenisation time (every distinct sentence once), the host encoding
time (tokens -> id rows), the device time of the caption_eval call (events around the two launches, offsets check
included), the wall time of the METEOR launches with their host encoding (stub stemmer and synonym table of
tests/meteor_reference.py), and the time of the float64 host restatement (tests/caption_eval_reference.py, one thread) on
the pairs of --restate videos, with its extrapolation to all pairs."""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bmhrl_amd import evaluate as E, ops  # noqa: E402
from tests import caption_eval_reference as cr  # noqa: E402
from tests.meteor_reference import DictStemmer, dict_synonyms  # noqa: E402

V = 10000


def job(n_videos, n_props, seed=0):
    rng = random.Random(seed)
    word = lambda: f"w{min(int(rng.paretovariate(1.1)), V - 1)}"            # noqa: E731  (Zipf-like word draw)
    sent = lambda a, b: " ".join(word() for _ in range(rng.randint(a, b))).capitalize() + "."       # noqa: E731
    gts = [{}, {}]
    for v in range(n_videos):
        dur = rng.uniform(30.0, 240.0)
        for gt in gts:
            cuts = sorted(rng.uniform(0.0, dur) for _ in range(rng.randint(3, 4) - 1))
            stamps = [[a, b] for a, b in zip([0.0] + cuts, cuts + [dur])]
            gt[f"v_{v:05d}"] = {"duration": dur, "timestamps": stamps, "sentences": [sent(8, 20) for _ in stamps]}
    head = {"version": "VERSION 1.0", "external_data": {"used": True, "details": ""}}
    own = {}
    for vid, g in gts[0].items():
        own[vid] = []
        for stamp, s in zip(g["timestamps"], g["sentences"]):
            words = [w if rng.random() < 0.5 else word() for w in s.split()]
            own[vid].append({"sentence": " ".join(words), "timestamp": stamp})
    many = {}
    for vid, g in gts[0].items():
        many[vid] = []
        for _ in range(n_props):
            a, b = sorted((rng.uniform(0.0, g["duration"]), rng.uniform(0.0, g["duration"])))
            many[vid].append({"sentence": sent(6, 16), "timestamp": [a, b]})
    return gts, dict(head, results=own), dict(head, results=many)


def measure(gts, submission, tious, n_restate):
    ev = E.DenseCaptionEvaluator(gts, submission, tious, 1000, device="cuda:0", stemmer=DictStemmer(), synonyms=dict_synonyms)
    out = {"tious": tious, "pairs": [], "pairing_s": 0.0, "encode_s": 0.0, "device_ms": [], "meteor_s": 0.0}
    t0 = time.perf_counter()
    paired = [E.pair_captions(ev.ground_truths, ev.prediction, t) for t in tious]
    out["pairing_s"] = round(time.perf_counter() - t0, 3)
    t0 = time.perf_counter()
    for p in paired:
        for pairs in p.values():
            for h, r in pairs:
                ev._tok(h)
                if r is not None:
                    ev._tok(r)
    out["tokenize_s"] = round(time.perf_counter() - t0, 3)
    out["distinct_sentences"] = len(ev._tokens)
    scores = {}
    for t in tious:
        vids, off, hyps, refs = ev.tokenized_pairs(t)
        out["pairs"].append(len(hyps))
        t0 = time.perf_counter()
        arrays = E.encode_pairs(hyps, refs)
        out["encode_s"] += time.perf_counter() - t0
        dev = [torch.from_numpy(a).to("cuda:0") for a in arrays + (np.asarray(off, dtype=np.int32),)]
        ops.caption_eval(*dev)                                          # warm-up
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = ops.caption_eval(*dev)
        e1.record()
        torch.cuda.synchronize()
        out["device_ms"].append(round(e0.elapsed_time(e1), 3))
        t0 = time.perf_counter()
        meteor = E.meteor_pairs(hyps, refs, ev.meteor_tables(), "cuda:0")
        out["meteor_s"] += time.perf_counter() - t0
        gs = res[3].cpu().numpy()
        scores[t] = {"Bleu_4": float(gs[:, 3].mean()), "ROUGE_L": float(gs[:, 4].mean()), "CIDEr": float(gs[:, 5].mean()),
                     "METEOR_pair_mean": float(meteor.mean())}
        if t == tious[0]:                                               # the restatement, on the first videos' pairs
            n = min(n_restate, len(vids))
            t0 = time.perf_counter()
            st = DictStemmer().stem
            for g in range(n):
                grp = list(zip(hyps[off[g]:off[g + 1]], refs[off[g]:off[g + 1]]))
                if grp:
                    want = cr.group_scores([(list(h), list(r)) for h, r in grp], st, dict_synonyms)
                    assert abs(want["CIDEr"] - gs[g, 5]) <= 1e-9 * max(1.0, want["CIDEr"])
            dt = time.perf_counter() - t0
            out["restatement_videos"], out["restatement_pairs"] = n, off[n]
            out["restatement_s"] = round(dt, 3)
            out["restatement_all_pairs_s"] = round(dt * len(hyps) / max(1, off[n]), 1)
    out["encode_s"], out["meteor_s"] = round(out["encode_s"], 3), round(out["meteor_s"], 3)
    out["scores"] = scores
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=4900)
    ap.add_argument("--proposals", type=int, default=100)
    ap.add_argument("--restate", type=int, default=50)
    a = ap.parse_args()
    gts, own, many = job(a.videos, a.proposals)
    out = {"metric": "dense-captioning evaluation", "videos": a.videos, "proposals": a.proposals,
           "gt_props": measure(gts, own, [0.5], a.restate),
           "props100": measure(gts, many, [0.3, 0.5, 0.7, 0.9], a.restate)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
