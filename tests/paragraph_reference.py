"""Plain-Python restatement of the paragraph evaluation: the n-gram occurrence statistics S1-S2 with
collections.Counter, and the paragraphs, pairs, keys and per-video record P1-P8 with dicts and Python floats.  The four
metrics are those of tests/caption_eval_reference.py (METEOR: tests/meteor_reference.py).
tests/test_paragraph_cpu.py pins it to the hand check; tests/test_paragraph_gpu.py checks the device against it."""
from collections import Counter

from tests import caption_eval_reference as cr

MAX_N = 4
METRICS = cr.METRICS
STAT_KEYS = ("Para_RE_4", "Para_XRE_4", "Para_Div_1", "Para_Div_2")


# ---- S1-S2
def ngram_stats(paragraph):
    """[[total, distinct, in_repeated, cross, max_count] for n = 1..4] of one paragraph: a sequence of sentences, each a
    sequence of hashable tokens.  A gram lies inside one sentence."""
    rows = []
    for n in range(1, MAX_N + 1):
        per_sentence = [[tuple(s[i:i + n]) for i in range(len(s) - n + 1)] for s in paragraph]
        counts = Counter(g for grams in per_sentence for g in grams)
        total = sum(counts.values())
        seen, cross = set(), 0
        for grams in per_sentence:
            cross += sum(g in seen for g in grams)
            seen.update(grams)
        rows.append([total, len(counts), sum(c for c in counts.values() if c >= 2), cross, max(counts.values(), default=0)])
    return rows


def flatten(paragraphs, ids=None):
    """(tok, sent_off, para_off) lists of paragraphs of token sentences; ids: token -> int (default: the token itself)"""
    tok, sent_off, para_off = [], [0], [0]
    for para in paragraphs:
        for sent in para:
            tok += [t if ids is None else ids[t] for t in sent]
            sent_off.append(len(tok))
        para_off.append(len(sent_off) - 1)
    return tok, sent_off, para_off


# ---- P1-P8
def score_of(pred):
    s = pred.get("proposal_score", 0.0)
    return float(s[0] if isinstance(s, (list, tuple)) else s)


def clean(sentences, tokenizer):
    out = [tuple(tokenizer(cr.remove_nonascii(s))) for s in sentences]
    return [t for t in out if t]


def by_time(stamps, positions):
    """the positions ordered by (start, end) of their stamps; ties keep the order given"""
    return sorted(positions, key=lambda k: (float(stamps[k][0]), float(stamps[k][1])))


def predicted_paragraph(preds, tokenizer, top=None):
    ranked = sorted(range(len(preds)), key=lambda k: -score_of(preds[k]))            # stable: ties keep list order
    kept = sorted(ranked if top is None else ranked[:top])
    order = by_time([p["timestamp"] for p in preds], kept)
    return clean([preds[k]["sentence"] for k in order], tokenizer)


def reference_paragraph(entry, tokenizer, sort_references=False):
    positions = list(range(len(entry["sentences"])))
    if sort_references:
        positions = by_time(entry["timestamps"], positions)
    return clean([entry["sentences"][k] for k in positions], tokenizer)


def evaluate(ground_truths, submission, n_tious, max_proposals, tokenizer, stem=None, syn=None, top=None,
             sort_references=False):
    """(the Para_* part of .scores, .paragraph_per_video with the integers as nested lists)"""
    prediction = cr.cut(submission, max_proposals)
    vids = cr.video_ids(ground_truths)
    predicted = {vid: predicted_paragraph(prediction.get(vid, []), tokenizer, top) for vid in vids}
    flat = lambda para: [w for s in para for w in s]                                                       # noqa: E731
    per_file = []
    for gt in ground_truths:
        pairs = []
        for vid in vids:
            ref = reference_paragraph(gt[vid], tokenizer, sort_references) if vid in gt else []
            if ref:
                pairs.append((flat(predicted[vid]), flat(ref)))
        if pairs:
            per_file.append(cr.group_scores(pairs, stem, syn))
    out = {}
    for m in METRICS:
        out["Para_" + m] = sum(s[m] for s in per_file) / len(per_file) if per_file else 0.0
    stats = {vid: ngram_stats(predicted[vid]) for vid in vids}
    for key, n, value in (("Para_RE_4", 4, lambda r: (r[0] - r[1]) / r[0]), ("Para_XRE_4", 4, lambda r: r[3] / r[0]),
                          ("Para_Div_1", 1, lambda r: r[1] / r[0]), ("Para_Div_2", 2, lambda r: r[1] / r[0])):
        vals = [value(stats[vid][n - 1]) for vid in vids if stats[vid][n - 1][0] > 0]
        out[key] = sum(vals) / len(vals) if vals else 0.0
    per_video = {vid: {"stats": stats[vid], "sentences": len(predicted[vid]), "tokens": len(flat(predicted[vid]))}
                 for vid in vids}
    return {k: [v] * n_tious for k, v in out.items()}, per_video


# ---- the hand check
HAND_PARAGRAPH = ["a man is playing a guitar".split(), "a man is playing a guitar on stage".split(), "the crowd claps".split()]
HAND_STATS = [[17, 10, 12, 6, 4], [14, 9, 10, 5, 2], [11, 7, 8, 4, 2], [8, 5, 6, 3, 2]]
