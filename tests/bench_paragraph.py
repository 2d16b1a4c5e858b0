"""Paragraph evaluation (bmhrl_amd/evaluate.py paragraph_*, csrc/paragraph.hip): one JSON line for the
synthetic ActivityNet-sized job of tests/bench_caption_eval.py -- 4 900 videos (--videos), two ground-truth files with 3-4
captions per video of 8..20 words -- read as paragraphs
- "gt_props": with the first file's own segments as proposals (one sentence each, half of its words redrawn);
- "props10": with 10 proposals per video (--proposals; random segments, sentences of 6..16 words).
Per job: the host time of paragraph_groups (tokenisation included), the encoding time, the device time of the ONE
caption_eval call whose groups are the two files (events around a call after a warm one: the document-frequency scan of a
pair then walks every reference paragraph of its file), the wall time of the METEOR launches, the device time of the
ngram_stats launch over the predicted paragraphs (events, after a warm one; its offsets check included) and the time of the
Counter restatement (tests/paragraph_reference.py, one host thread) of the same statistics on --restate paragraphs, with
its extrapolation to all of them."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bmhrl_amd import evaluate as E, ops  # noqa: E402
from tests import paragraph_reference as pr  # noqa: E402
from tests.bench_caption_eval import job  # noqa: E402
from tests.meteor_reference import DictStemmer, dict_synonyms  # noqa: E402

DEV = "cuda:0"


def timed(fn):
    """(result, milliseconds between two events) of fn() after one warm call"""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, round(e0.elapsed_time(e1), 3)


def measure(gts, submission, n_restate):
    ev = E.DenseCaptionEvaluator(gts, submission, [0.5], 1000, device=DEV, stemmer=DictStemmer(), synonyms=dict_synonyms,
                                 paragraph=True)
    out = {}
    t0 = time.perf_counter()
    groups = E.paragraph_groups(ev.ground_truths, ev.prediction, ev._tok)
    out["groups_s"] = round(time.perf_counter() - t0, 3)
    hyps, refs, off = [], [], [0]
    for refs_of in groups.references:
        for vid in groups.vids:
            if vid in refs_of:
                hyps.append(E._flat(groups.predicted[vid]))
                refs.append(E._flat(refs_of[vid]))
        off.append(len(hyps))
    out["pairs"], out["files"] = len(hyps), len(off) - 1
    out["hyp_words_mean"] = round(float(np.mean([len(h) for h in hyps])), 1)
    out["ref_words_mean"] = round(float(np.mean([len(r) for r in refs])), 1)
    t0 = time.perf_counter()
    arrays = E.encode_pairs(hyps, refs)
    out["encode_s"] = round(time.perf_counter() - t0, 3)
    dev = [torch.from_numpy(a).to(DEV) for a in arrays + (np.asarray(off, dtype=np.int32),)]
    res, out["caption_eval_ms"] = timed(lambda: ops.caption_eval(*dev))
    t0 = time.perf_counter()
    meteor = E.meteor_pairs(hyps, refs, ev.meteor_tables(), DEV)
    out["meteor_s"] = round(time.perf_counter() - t0, 3)
    gs = res[3].cpu().numpy()
    out["scores"] = {"Para_Bleu_4": float(gs[:, 3].mean()), "Para_ROUGE_L": float(gs[:, 4].mean()),
                     "Para_CIDEr": float(gs[:, 5].mean()), "Para_METEOR_pair_mean": float(meteor.mean())}

    paras = [groups.predicted[vid] for vid in groups.vids]
    table = {}
    tok, sent_off, para_off = pr.flatten([[[table.setdefault(w, len(table)) for w in s] for s in p] for p in paras])
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=DEV)                                         # noqa: E731
    tok_d, sent_d, para_d = i32(tok), i32(sent_off), i32(para_off)
    stats, out["ngram_stats_ms"] = timed(lambda: ops.ngram_stats(tok_d, sent_d, para_d))
    stats = stats.cpu().numpy()
    out["paragraphs"], out["tokens"], out["longest_paragraph"] = len(paras), len(tok), int(stats[:, 0, 0].max())
    out["scores"].update(E.paragraph_means(stats))
    n = min(n_restate, len(paras))
    t0 = time.perf_counter()
    want = [pr.ngram_stats(p) for p in paras[:n]]
    dt = time.perf_counter() - t0
    assert stats[:n].tolist() == want
    out["restatement_paragraphs"], out["restatement_s"] = n, round(dt, 3)
    out["restatement_all_s"] = round(dt * len(paras) / max(1, n), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=4900)
    ap.add_argument("--proposals", type=int, default=10)
    ap.add_argument("--restate", type=int, default=4900)
    a = ap.parse_args()
    gts, own, many = job(a.videos, a.proposals)
    out = {"metric": "paragraph evaluation", "videos": a.videos, "proposals": a.proposals,
           "gt_props": measure(gts, own, a.restate), "props10": measure(gts, many, a.restate)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
