"""Float64 restatement of the reference's per-prefix caption rewards, written from metrics/cider.py (:28-70, :114-122,
:167-253), metrics/bleu.py (:26-58, :214-278) and metrics/util.py (:92-139): plain dicts over word tuples, one prefix at a
time, in the reference's arithmetic order.  tests/test_rewards_cpu.py checks it against the reference's own outputs
(tests/golden/rewards.npz); tests/test_rewards_gpu.py checks the device scorers against it on random cases.

Inputs are strings as the reference sees them: itos (vocab id -> string), a row of vocab ids, the reference caption and,
for CIDEr, the document-frequency dict of precook_corpus."""
from collections import defaultdict
import math

import numpy as np

EOS = "</s>"


def precook_corpus(caps, n=4):
    """metrics/cider.py precook_corpus: n-gram counts over the corpus, kept when above 1"""
    counts = defaultdict(int)
    for cap in caps:
        for k in range(1, n + 1):
            for i in range(len(cap) - k + 1):
                counts[tuple(cap[i:i + k])] += 1
    return {key: val for key, val in counts.items() if val > 1}


def precook(words, n):
    """n-gram -> count in first-occurrence order, lengths 1..n (metrics/util.py precook)"""
    counts = {}
    for k in range(1, n + 1):
        for i in range(len(words) - k + 1):
            g = tuple(words[i:i + k])
            counts[g] = counts.get(g, 0) + 1
    return counts


def _counts2vec(cnts, df, n):
    vec = [dict() for _ in range(n)]
    norm = [0.0] * n
    length = 0
    for gram, tf in cnts.items():
        d = np.log(max(1.0, df.get(gram, 0)))
        k = len(gram) - 1
        vec[k][gram] = float(tf) * (0.0 - d)          # ref_len = log(1 reference) = 0
        norm[k] += vec[k][gram] ** 2
        if k == 1:                                      # the "length" counts bigrams
            length += tf
    return vec, [np.sqrt(x) for x in norm], length


def cider_prefix(hyp_words, ref_words, df, n=4, sigma=6.0):
    """CIDEr of one hypothesis word list against one reference word list"""
    vh, nh, lh = _counts2vec(precook(hyp_words, n), df, n)
    vr, nr, lr = _counts2vec(precook(ref_words, n), df, n)
    delta = float(lh - lr)
    val = np.zeros(n)
    for k in range(n):
        for gram in vh[k]:
            r = vr[k].get(gram, 0.0)
            val[k] += min(vh[k][gram], r) * r
        if nh[k] != 0 and nr[k] != 0:
            val[k] /= nh[k] * nr[k]
        val[k] *= np.e ** (-(delta ** 2) / (2 * sigma ** 2))
    return float(np.mean(val))


def cider_scores(itos, row, caption, df, n=4, sigma=6.0):
    """the reference's `rewards` row (fp64, len(row)): every prefix up to the first end token (an end token first: the
    float32 -0.1), padded with the last scored prefix"""
    hypo = [itos[int(i)] for i in row]
    ref_words = caption.lower().split()
    scores, last = [], 0
    for l in range(len(hypo)):
        if hypo[l] == EOS:
            if not scores:
                scores.append(float(np.float32(-0.1)))
            break
        scores.append(cider_prefix(" ".join(hypo[:l + 1]).split(), ref_words, df, n, sigma))
        last = l
    return np.array(scores + [scores[last]] * (len(hypo) - len(scores)), dtype=np.float64)


def bleu_prefix(hyp_words, ref_words, n=4):
    """BleuScorerObj.compute_score of one hypothesis against one reference ("average" reflen): the fp32 average of the
    n cumulative BLEUs"""
    tiny, small = 1e-15, 1e-9
    testlen, reflen = len(hyp_words), float(len(ref_words))
    ref_counts = precook(ref_words, 4)
    correct = [0] * 4
    for gram, c in precook(hyp_words, 4).items():
        correct[len(gram) - 1] += min(ref_counts.get(gram, 0), c)
    guess = [max(0, testlen - k + 1) for k in range(1, 5)]
    bleus, bleu = [], 1.0
    for k in range(n):
        bleu *= float(correct[k] + tiny) / (guess[k] + small)
        bleus.append(bleu ** (1.0 / (k + 1)))
    ratio = (testlen + tiny) / (reflen + small)
    if ratio < 1:
        bleus = [b * math.exp(1 - 1 / ratio) for b in bleus]
    w = np.float32(1 / n)
    acc = np.float32(bleus[0]) * w
    for b in bleus[1:]:
        acc = np.float32(acc + np.float32(b) * w)
    return np.float32(acc)


def bleu_scores(itos, row, caption, n=4):
    """the reference's BLEU `rewards` row (fp32 values): every prefix, lowercased, no stop at the end token"""
    hypo = [itos[int(i)] for i in row]
    ref_words = caption.lower().split()
    return np.array([bleu_prefix(" ".join(hypo[:l + 1]).lower().split(), ref_words, n) for l in range(len(hypo))],
                    dtype=np.float32)


def delta_row(scores):
    """column 0: the score; then first differences (fp64 differences of CIDEr rows, fp32 of BLEU rows), as fp32"""
    s = np.asarray(scores)
    d = np.empty(s.shape, dtype=np.float32)
    d[..., 0] = s[..., 0]
    d[..., 1:] = (s[..., 1:] - s[..., :-1]).astype(np.float32)
    return d


def discount(x, gamma, n_step=100):
    """metrics/util.py discontinue_reward without segments, in fp64: out[t] = sum_{i < n_step} gamma^i x[t + i]"""
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros_like(x)
    L = x.shape[-1]
    for t in range(L):
        for i in range(min(n_step, L - t)):
            out[..., t] += gamma ** i * x[..., t + i]
    return out
