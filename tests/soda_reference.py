"""Plain-Python restatement of SODA_c as DESIGN.md section 25 states it (written from Fujita et al., ECCV 2020, not from
the authors' tool): tIoU, thresholding, the plain double loop of the ordered assignment, precision / recall / F, the choice
of the best file per video and the means, in Python floats; METEOR through tests/meteor_reference.py.
tests/test_soda_cpu.py pins the double loop to a brute-force enumeration and holds the hand examples;
tests/test_soda_gpu.py checks the device (csrc/soda.hip, bmhrl_amd/evaluate.py) against this file."""
import numpy as np

from tests import meteor_reference
from tests.caption_eval_reference import cut, iou, remove_nonascii, video_ids

METRICS = ("SODA_c", "SODA_c_Precision", "SODA_c_Recall")
MAX_REFS = 256


def cost_matrix(pred_segments, ref_segments, S, threshold):
    """c[i][j] = (iou < t ? 0 : iou) * S[i][j], iou of (prediction, reference) in that argument order"""
    c = []
    for i, p in enumerate(pred_segments):
        row = []
        for j, r in enumerate(ref_segments):
            v = iou(p, r)
            row.append((0.0 if v < threshold else v) * S[i][j])
        c.append(row)
    return c


def dp(c):
    """D[P][R] of D[i][j] = max(D[i-1][j], D[i][j-1], D[i-1][j-1] + c[i][j]) with zero borders"""
    P, R = len(c), len(c[0]) if c else 0
    D = [[0.0] * (R + 1) for _ in range(P + 1)]
    for i in range(1, P + 1):
        for j in range(1, R + 1):
            D[i][j] = max(D[i - 1][j], D[i][j - 1], D[i - 1][j - 1] + c[i - 1][j - 1])
    return D[P][R]


def prf(max_score, P, R):
    """[max_score, precision, recall, F]; zeros for an empty side"""
    if P == 0 or R == 0:
        return [0.0, 0.0, 0.0, 0.0]
    p, r = max_score / P, max_score / R
    return [max_score, p, r, 0.0 if p + r == 0 else 2 * p * r / (p + r)]


def group_scores(pred_segments, ref_segments, S, tious):
    """(T, 4) rows of one group"""
    P, R = len(pred_segments), len(ref_segments)
    return [prf(dp(cost_matrix(pred_segments, ref_segments, S, t)) if P and R else 0.0, P, R) for t in tious]


def matchings(P, R):
    """every order-preserving one-to-one matching, as a list of (i, j) in path order"""
    def rec(i, j):
        if i == P or j == R:
            yield []
            return
        for rest in rec(i + 1, j):                      # prediction i stays unmatched
            yield rest
        for jj in range(j, R):                          # prediction i takes reference jj
            for rest in rec(i + 1, jj + 1):
                yield [(i, jj)] + rest
    return rec(0, 0)


def brute_force(c):
    """(the largest sum over all order-preserving matchings, summed left to right in path order; the first matching of
    non-zero cells that reaches it)"""
    best, best_m = 0.0, []
    for m in matchings(len(c), len(c[0])):
        total = 0.0
        for i, j in m:
            total += c[i][j]
        if total > best:
            best, best_m = total, [(i, j) for i, j in m if c[i][j] != 0.0]
    return best, best_m


def best_reference_each(c):
    """what "every prediction takes its best reference" would sum to (no order, no one-to-one)"""
    total = 0.0
    for row in c:
        total += max(row)
    return total


# ---- sentences
def meteor_matrix(hyp_tokens, ref_tokens, stem=None, syn=None):
    """S[i][j]: whole-sentence METEOR of token list i against token list j (an empty side scores 0)"""
    return [[meteor_reference.meteor_prefix([w.lower() for w in h], [w.lower() for w in r], stem, syn) for r in ref_tokens]
            for h in hyp_tokens]


def by_time(stamps):
    return sorted(range(len(stamps)), key=lambda k: (float(stamps[k][0]), float(stamps[k][1])))


def groups_of(ground_truths, prediction, sort_references=False):
    """video id -> [(file, prediction segments, prediction sentences, reference segments, reference sentences)] for every
    ground-truth video; predictions by (start, end), stable; references in file order unless sort_references"""
    out = {}
    for vid in video_ids(ground_truths):
        out[vid] = []
        preds = prediction.get(vid, [])
        if not preds:
            continue
        order = by_time([p["timestamp"] for p in preds])
        for f, gt in enumerate(ground_truths):
            if vid not in gt or not gt[vid]["timestamps"]:
                continue
            stamps, sents = gt[vid]["timestamps"], gt[vid]["sentences"]
            rorder = by_time(stamps) if sort_references else list(range(len(stamps)))
            out[vid].append((f, [[float(x) for x in preds[k]["timestamp"]] for k in order],
                             [remove_nonascii(preds[k]["sentence"]) for k in order],
                             [[float(x) for x in stamps[k]] for k in rorder], [remove_nonascii(sents[k]) for k in rorder]))
    return out


def evaluate(ground_truths, submission, tious, max_proposals, tokenizer, stem=None, syn=None, sort_references=False):
    """(scores: SODA_c / SODA_c_Precision / SODA_c_Recall lists, one entry per tIoU; per_video: video id -> [(p, r, F)] per
    tIoU)"""
    per_video = {}
    for vid, groups in groups_of(ground_truths, cut(submission, max_proposals), sort_references).items():
        rows = []
        for _, psegs, psents, rsegs, rsents in groups:
            S = meteor_matrix([tokenizer(s) for s in psents], [tokenizer(s) for s in rsents], stem, syn)
            rows.append(group_scores(psegs, rsegs, S, tious))
        triples = []
        for t in range(len(tious)):
            best = (0.0, 0.0, 0.0)
            for k, row in enumerate(rows):
                if k == 0 or row[t][3] > best[2]:
                    best = (row[t][1], row[t][2], row[t][3])
            triples.append(best)
        per_video[vid] = triples
    scores = {m: [] for m in METRICS}
    for t in range(len(tious)):
        for m, col in zip(METRICS, (2, 0, 1)):
            total = 0.0
            for triples in per_video.values():
                total += triples[t][col]
            scores[m].append(total / len(per_video))
    return scores, per_video


# ---- the random cases tests/test_soda_cpu.py (brute force, coverage) and tests/test_soda_gpu.py (device) share
CASE_SEED, CASE_COUNT = 7, 400
CASE_TIOUS = (0.3, 0.5, 0.7, 0.9)


def random_cases(seed=CASE_SEED, count=CASE_COUNT):
    """[(prediction segments (P <= 7, by time), reference segments (R <= 5), S (P, R) with about 40 % zeros)]; the
    references tile [0, 10] with small gaps and overlaps, the predictions are jittered copies of references or random
    segments, so that every threshold of CASE_TIOUS keeps some cells and drops others; case 13 has an all-zero S"""
    rng = np.random.RandomState(seed)
    cases = []
    for n in range(count):
        P, R = int(rng.randint(1, 8)), int(rng.randint(1, 6))
        cuts = np.sort(rng.uniform(0.0, 10.0, R - 1)).tolist()
        refs = [[max(0.0, a - rng.uniform(0, 0.5)), min(10.0, b + rng.uniform(0, 0.5))]
                for a, b in zip([0.0] + cuts, cuts + [10.0])]
        preds = []
        for _ in range(P):
            if rng.rand() < 0.7:
                a, b = refs[rng.randint(R)]
                w = b - a
                preds.append([a + rng.uniform(-0.3, 0.3) * w, b + rng.uniform(-0.3, 0.3) * w])
            else:
                preds.append(np.sort(rng.uniform(0.0, 10.0, 2)).tolist())
        preds = [[float(a), float(max(a, b))] for a, b in preds]
        preds.sort(key=lambda s: (s[0], s[1]))
        S = rng.uniform(0.0, 1.0, (P, R))
        S[rng.rand(P, R) < 0.4] = 0.0
        if n == 13:
            S[:] = 0.0
        cases.append((preds, [[float(a), float(b)] for a, b in refs], S.tolist()))
    return cases


def random_matrices(seed=CASE_SEED, count=CASE_COUNT):
    """cost matrices of their own (no segments): P <= 7, R <= 5, uniform in (0, 1) with about 40 % zeros"""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(count):
        c = rng.uniform(0.0, 1.0, (int(rng.randint(1, 8)), int(rng.randint(1, 6))))
        c[rng.rand(*c.shape) < 0.4] = 0.0
        out.append(c.tolist())
    return out


# ---- the hand example: 2 x 2, the large scores on the anti-diagonal
HAND_PRED = [[0.0, 10.0], [10.0, 20.0]]
HAND_REF = [[0.0, 10.0], [10.0, 20.0]]
HAND_S = [[0.5, 0.0], [0.0, 0.25]]
HAND_ANTI_PRED = [[0.0, 12.0], [8.0, 20.0]]
HAND_ANTI_REF = [[8.0, 20.0], [0.0, 12.0]]
HAND_ANTI_S = [[0.25, 0.75], [0.5, 0.125]]
