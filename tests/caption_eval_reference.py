"""Plain-Python float64 restatement of the dense-captioning evaluation: the tIoU pairing and detection
scores of the reference's evaluation/evaluate.py, and the four per-video metrics it asks of pycocoevalcap -- corpus BLEU
over a video's (prediction, reference) pairs, mean ROUGE-L, mean CIDEr with the pairs' own document frequencies, and the
mean whole-sentence METEOR of tests/meteor_reference.py.  Dicts, Python floats and the reference's order of operations;
tests/test_caption_eval_cpu.py pins it to tests/golden/caption_eval.json (recorded from the reference's ANETcaptions),
tests/test_caption_eval_gpu.py checks the device against it."""
import math
from collections import defaultdict

import numpy as np

from tests import meteor_reference

GARBAGE = "␀"          # the one word of the reference of a prediction that overlaps nothing (no ASCII sentence holds it)


def remove_nonascii(text):
    return "".join(c if ord(c) < 128 else " " for c in text)


def iou(a, b):
    inter = max(0, min(b[1], a[1]) - max(b[0], a[0]))
    union = min(max(b[1], a[1]) - min(b[0], a[0]), b[1] - b[0] + a[1] - a[0])
    return float(inter) / (union + 1e-8)


def video_ids(ground_truths):
    ids = set()
    for gt in ground_truths:
        ids |= set(gt.keys())
    return sorted(ids)


def cut(submission, max_proposals):
    return {vid: segs[:max_proposals] for vid, segs in submission["results"].items()}


def pairs_of(ground_truths, prediction, tiou):
    """video id -> [(hypothesis sentence, reference sentence or None)], every ground-truth video, sorted"""
    out = {}
    for vid in video_ids(ground_truths):
        out[vid] = []
        if vid not in prediction:
            continue
        for pred in prediction[vid]:
            n = len(out[vid])
            for gt in ground_truths:
                if vid in gt:
                    for i, stamp in enumerate(gt[vid]["timestamps"]):
                        if iou(pred["timestamp"], stamp) >= tiou:
                            out[vid].append((remove_nonascii(pred["sentence"]), remove_nonascii(gt[vid]["sentences"][i])))
            if len(out[vid]) == n:
                out[vid].append((remove_nonascii(pred["sentence"]), None))
    return out


def detection(ground_truths, prediction, tiou):
    """(precision, recall); an empty prediction list counts precision 0 for that file"""
    vids = video_ids(ground_truths)
    precision, recall = [0] * len(vids), [0] * len(vids)
    for v, vid in enumerate(vids):
        for gt in ground_truths:
            if vid not in gt:
                continue
            stamps = gt[vid]["timestamps"]
            covered_r, covered_p = set(), set()
            preds = prediction.get(vid, [])
            for pi, pred in enumerate(preds):
                for ri, stamp in enumerate(stamps):
                    if iou(pred["timestamp"], stamp) > tiou:
                        covered_r.add(ri)
                        covered_p.add(pi)
            if preds:
                precision[v] = max(precision[v], float(len(covered_p)) / len(preds))
            recall[v] = max(recall[v], float(len(covered_r)) / len(stamps))
    return sum(precision) / len(precision), sum(recall) / len(recall)


def grams(words, n=4):
    counts = defaultdict(int)
    for k in range(1, n + 1):
        for i in range(len(words) - k + 1):
            counts[tuple(words[i:i + k])] += 1
    return counts


# ---- BLEU: counts per pair, score of the summed counts
def bleu_counts(hyp, ref, n=4):
    """(guess[n], correct[n], len(hyp), len(ref)) of one pair"""
    hc, rc = grams(hyp, n), grams(ref, n)
    correct = [0] * n
    for g, c in hc.items():
        correct[len(g) - 1] += min(rc.get(g, 0), c)
    return [max(0, len(hyp) - k + 1) for k in range(1, n + 1)], correct, len(hyp), len(ref)


def bleu_group(pairs, n=4):
    small, tiny = 1e-9, 1e-15
    guess, correct, testlen, reflen = [0] * n, [0] * n, 0, 0
    for hyp, ref in pairs:
        g, c, tl, rl = bleu_counts(hyp, ref, n)
        testlen += tl
        reflen += rl
        for k in range(n):
            guess[k] += g[k]
            correct[k] += c[k]
    bleus, bleu = [], 1.
    for k in range(n):
        bleu *= float(correct[k] + tiny) / (guess[k] + small)
        bleus.append(bleu ** (1. / (k + 1)))
    ratio = (testlen + tiny) / (reflen + small)
    if ratio < 1:
        for k in range(n):
            bleus[k] *= math.exp(1 - 1 / ratio)
    return bleus


# ---- ROUGE-L
def lcs(a, b):
    row = [0] * (len(b) + 1)
    for x in a:
        prev = 0
        for j, y in enumerate(b):
            cur = row[j + 1]
            row[j + 1] = prev + 1 if x == y else max(row[j + 1], row[j])
            prev = cur
    return row[len(b)]


def rouge_pair(hyp, ref, beta=1.2):
    l = lcs(hyp, ref)
    if l == 0:
        return 0.0
    prec, rec = l / float(len(hyp)), l / float(len(ref))
    return ((1 + beta ** 2) * prec * rec) / float(rec + beta ** 2 * prec)


# ---- CIDEr with the group's own document frequencies
def cider_pairs(pairs, n=4, sigma=6.0):
    """the per-pair values (times 10)"""
    df = defaultdict(float)
    for _, ref in pairs:
        for g in set(grams(ref, n)):
            df[g] += 1
    ref_len = np.log(float(len(pairs)))

    def vec_of(counts):
        vec, norm, length = [defaultdict(float) for _ in range(n)], [0.0] * n, 0
        for g, tf in counts.items():
            k = len(g) - 1
            vec[k][g] = float(tf) * (ref_len - np.log(max(1.0, df[g])))
            norm[k] += pow(vec[k][g], 2)
            if k == 1:
                length += tf
        return vec, [np.sqrt(x) for x in norm], length

    out = []
    for hyp, ref in pairs:
        vh, nh, lh = vec_of(grams(hyp, n))
        vr, nr, lr = vec_of(grams(ref, n))
        delta = float(lh - lr)
        val = np.array([0.0] * n)
        for k in range(n):
            for g in vh[k]:
                val[k] += min(vh[k][g], vr[k][g]) * vr[k][g]
            if nh[k] != 0 and nr[k] != 0:
                val[k] /= nh[k] * nr[k]
            val[k] *= np.e ** (-(delta ** 2) / (2 * sigma ** 2))
        out.append(float(np.mean(val)) * 10.0)
    return out


def meteor_pair(hyp, ref, stem=None, syn=None):
    return meteor_reference.meteor_prefix([w.lower() for w in hyp], [w.lower() for w in ref], stem, syn)


def mean(xs):
    t = 0.0
    for x in xs:
        t += x
    return t / len(xs)


def group_scores(pairs, stem=None, syn=None):
    """the seven metrics of one video's token pairs [(hyp words, ref words)] (at least one)"""
    out = {f"Bleu_{k + 1}": b for k, b in enumerate(bleu_group(pairs))}
    out["METEOR"] = mean([meteor_pair(h, r, stem, syn) for h, r in pairs])
    out["ROUGE_L"] = mean([rouge_pair(h, r) for h, r in pairs])
    out["CIDEr"] = mean(cider_pairs(pairs))
    return out


METRICS = ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "METEOR", "ROUGE_L", "CIDEr")


def evaluate(ground_truths, submission, tious, max_proposals, tokenizer, stem=None, syn=None, verbose=True):
    """.scores of the evaluator: dict of lists, one entry per tIoU"""
    prediction = cut(submission, max_proposals)
    scores = {m: [] for m in METRICS}
    for tiou in tious:
        per_video = {m: [] for m in METRICS}
        for vid, pairs in pairs_of(ground_truths, prediction, tiou).items():
            toks = [(tokenizer(h), [GARBAGE] if r is None else tokenizer(r)) for h, r in pairs]
            s = group_scores(toks, stem, syn) if toks else {m: 0.0 for m in METRICS}
            for m in METRICS:
                per_video[m].append(s[m])
        for m in METRICS:
            scores[m].append(float(np.mean(per_video[m])))
    if verbose:
        scores["Recall"], scores["Precision"] = [], []
        for tiou in tious:
            p, r = detection(ground_truths, prediction, tiou)
            scores["Recall"].append(r)
            scores["Precision"].append(p)
    return scores


# ---- the four pairs of the hand check
HAND_PAIRS = [("a man is playing a guitar".split(), "a man plays the guitar on stage".split()),
              ("a man is playing a guitar".split(), "he is playing a guitar".split()),
              ("the crowd claps".split(), ["qzxv"]),
              ([], "a man sits".split())]
HAND_BLEU = [0.43656992628987906, 0.36896893068733144, 0.3047460173407026, 0.2577374189019271]
HAND_CIDER = 1.661135057887748
HAND_CIDER_PAIRS = [0.5147672060852395, 6.129773025465752, 0.0, 0.0]
HAND_LCS = [3, 4, 0, 0]
HAND_ROUGE = [0.45522388059701485, 0.7393939393939394, 0.0, 0.0]
