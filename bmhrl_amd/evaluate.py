"""Dense-captioning evaluator on the device: the reference's evaluation/evaluate.py ANETcaptions (tIoU pairing, Bleu_1..4,
METEOR, ROUGE_L, CIDEr per video, detection precision / recall) without the Java PTB tokenizer, the METEOR jar or a
pycocoevalcap checkout.  DESIGN.md section 24 has the rules and the measurements.

The host pairs predictions with ground-truth captions (pair_captions), tokenizes every distinct sentence once, maps the
tokens to ids of one rewards.StringTable and hands the pairs of all videos, grouped per video, to one call of
ops.caption_eval (csrc/caption_eval.hip): BLEU over the video's pairs, mean ROUGE-L, mean CIDEr with the document
frequencies of those same pairs.  METEOR goes through the per-prefix reward launch (ops.meteor) and
reads the score of the whole hypothesis.

What is and is not the published protocol: `Bleu_*`, `ROUGE_L`, `CIDEr`, `Precision` and `Recall` are the pycocoevalcap /
evaluate.py functions of the tokens they are given.  `tokenize` is a stand-in for the Java PTB tokenizer (lowercase, words
split from punctuation, pycocoevalcap's punctuation tokens dropped), not that tokenizer; pass tokenizer= to use tokens
of your own.  `METEOR` is the nltk-3.5 formula (exact, stem, synonym stages; alpha 0.9, beta 3, gamma 0.5), the mean over
a video's pairs of the whole-hypothesis score -- not Java METEOR 1.5, which has other stages and weights and reports one
corpus aggregate per call.  It is comparable between runs of this package, not to published METEOR figures.

SODA_c (soda=True; soda_groups / soda_scores) is written from the paper (Fujita et al., "SODA: Story
Oriented Dense Video Captioning Evaluation Framework", ECCV 2020), not from its authors' tool, which this package has never
been compared with: per video and ground-truth file, the time-ordered one-to-one matching of predictions and references
that maximises the sum of tIoU x METEOR (ops.meteor_matrix scores every prediction against every reference by index,
ops.soda_dp runs the max-plus dynamic programme; csrc/soda.hip), its precision, recall and F1, the best file per video, the
mean over the ground-truth videos.  Its METEOR is the function above, so the figure is comparable between runs of this
package, not to published SODA_c.

Proposal metrics on the device (tiou_backend="device", proposal_recall=True; segment_tables, detection_scores_device,
pair_indices_device, proposal_recall): the tIoU tables of every group are evaluated in one launch
(ops.tiou_hits, csrc/proposal_eval.hip) with the bits of `tiou` below, and detection precision / recall, the caption pairing
and AR@AN / AUC are built from its integers.

Paragraph evaluation (paragraph=True; paragraph_groups, paragraph_scores, paragraph_stats, paragraph_means; DESIGN.md
section 33): a video's captions in time order read as one paragraph.  Para_Bleu_1..4 / Para_METEOR / Para_ROUGE_L /
Para_CIDEr score the predicted paragraph against each ground-truth file's paragraph through score_pairs with one group per
file; Para_RE_4 / Para_XRE_4 / Para_Div_1 / Para_Div_2 are the n-gram repetition, cross-sentence repetition and diversity
of the predicted paragraphs, from the exact occurrence counts of one ops.ngram_stats launch (csrc/paragraph.hip).  They are
written from the definitions in section 33 and have been compared with no published tool; METEOR is the function above,
and several ground-truth files are averaged where the usual paragraph protocol takes them as multiple references of one
score.  So the figures are comparable between runs of this package, not to published paragraph-level numbers.

Bootstrap intervals and run comparison (bootstrap=R; bootstrap, compare, summarize, bootstrap_ratios_host; DESIGN.md
section 37): .per_video keeps the per-video values every mean over videos is taken of, and the paired bootstrap over
videos (ops.bootstrap_ratios, csrc/bootstrap.hip: one launch per family; the same definition in numpy when the device is
the CPU) gives each such figure a percentile interval, and two evaluated runs over the same videos the interval of their
difference under the same resamples.  It says how much the sample of videos moves a figure, nothing more.
"""
from __future__ import annotations

import json
import re
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

PREDICTION_FIELDS = ("results", "version", "external_data")
METRICS = ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "METEOR", "ROUGE_L", "CIDEr")
# the tokens pycocoevalcap's tokenizer drops
PUNCTUATIONS = frozenset(["''", "'", "``", "`", "-LRB-", "-RRB-", "-LCB-", "-RCB-", ".", "?", "!", ",", ":", "-", "--", "...",
                          ";"])
# the one word of the reference a prediction without an overlap is scored against: not ASCII, so no sentence that passed
# remove_nonascii holds it
GARBAGE = "␀"
_TOKEN = re.compile(r"\.\.\.|--|\w+|[^\w\s]", re.ASCII)
_METEOR_CHUNK = 32768                         # pairs per METEOR launch (bounds the (pairs, L) score rows)
SODA_METRICS = ("SODA_c", "SODA_c_Precision", "SODA_c_Recall")
_SODA_CELLS = 4 << 20                         # cells of the score matrices per pair of SODA launches (32 MiB of fp64)


def remove_nonascii(text: str) -> str:
    return "".join(c if ord(c) < 128 else " " for c in text)


def tokenize(sentence: str) -> List[str]:
    """Stand-in for the Java PTB tokenizer: lowercase, runs of letters / digits / "_" are words, every other non-space
    character is a token of its own ("..." and "--" stay whole), pycocoevalcap's punctuation tokens are dropped.  An
    empty or punctuation-only sentence gives []."""
    return [t for t in _TOKEN.findall(sentence.lower()) if t not in PUNCTUATIONS]


def tiou(interval_1: Sequence[float], interval_2: Sequence[float]) -> float:
    """temporal intersection over union as evaluate.py computes it (the union is capped by the sum of the two lengths)"""
    start_i, end_i = interval_1[0], interval_1[1]
    start, end = interval_2[0], interval_2[1]
    intersection = max(0, min(end, end_i) - max(start, start_i))
    union = min(max(end, end_i) - min(start, start_i), end - start + end_i - start_i)
    return float(intersection) / (union + 1e-8)


def ground_truth_video_ids(ground_truths: Sequence[dict]) -> List[str]:
    """the union of the files' video ids, sorted"""
    return sorted(set().union(*[set(gt.keys()) for gt in ground_truths]))


def pair_captions(ground_truths: Sequence[dict], prediction: Dict[str, list], tiou_threshold: float
                  ) -> Dict[str, List[Tuple[str, Optional[str]]]]:
    """video id -> [(predicted sentence, ground-truth sentence)] for every ground-truth video id (sorted).  A prediction
    pairs with every caption of every ground-truth file whose tIoU is >= the threshold, in the order prediction, file,
    caption; a prediction that pairs with nothing gives one pair whose ground-truth sentence is None (scored against a
    reference no hypothesis shares a word with).  Sentences have passed remove_nonascii.  Videos without predictions
    get []; videos that only the prediction holds are left out."""
    out: Dict[str, List[Tuple[str, Optional[str]]]] = {}
    for vid in ground_truth_video_ids(ground_truths):
        pairs = out[vid] = []
        for pred in prediction.get(vid, ()):
            hyp = remove_nonascii(pred["sentence"])
            added = False
            for gt in ground_truths:
                if vid not in gt:
                    continue
                caps = gt[vid]
                for idx, stamp in enumerate(caps["timestamps"]):
                    if tiou(pred["timestamp"], stamp) >= tiou_threshold:
                        pairs.append((hyp, remove_nonascii(caps["sentences"][idx])))
                        added = True
            if not added:
                pairs.append((hyp, None))
    return out


def detection_scores(ground_truths: Sequence[dict], prediction: Dict[str, list], tiou_threshold: float
                     ) -> Tuple[float, float]:
    """(precision, recall) of the predicted segments as evaluate.py's evaluate_detection: per video and file, a
    prediction / a ground-truth segment is covered when some tIoU is > the threshold (strictly); the best value over
    the files; the mean over the ground-truth videos.  A video without predictions (none, or an empty list) counts
    precision 0."""
    vids = ground_truth_video_ids(ground_truths)
    precision, recall = [], []
    for vid in vids:
        best_p = best_r = 0.0
        preds = prediction.get(vid, ())
        for gt in ground_truths:
            if vid not in gt:
                continue
            stamps = gt[vid]["timestamps"]
            refs_hit, preds_hit = set(), set()
            for pi, pred in enumerate(preds):
                for ri, stamp in enumerate(stamps):
                    if tiou(pred["timestamp"], stamp) > tiou_threshold:
                        refs_hit.add(ri)
                        preds_hit.add(pi)
            if len(preds):
                best_p = max(best_p, float(len(preds_hit)) / len(preds))
            best_r = max(best_r, float(len(refs_hit)) / len(stamps))
        precision.append(best_p)
        recall.append(best_r)
    return sum(precision) / len(precision), sum(recall) / len(recall)


# ---- proposal metrics on the device
class SegmentTables:
    """What the tIoU launches of one (ground truths, prediction) job read, built once on the host (segment_tables):
    vids            the ground-truth video ids, sorted
    pred_seg        (NP, 2) fp64 start, end of the predictions of those videos, video by video
    pred_video      (NP,) int64 index into vids;  pred_off (V + 1) int64: video v owns rows [pred_off[v], pred_off[v + 1])
    pred_sentences  (NP) the predictions' sentences as given
    ref_seg         (NR, 2) fp64 of the references, video-major, file-minor, then caption order
    ref_file        (NR,) int64 file index;  ref_off (V + 1) int64;  ref_sentences (NR) as given
    file_groups     (G, 4) int32 [p0, P, r0, R], one row per (video, file that holds the video), video-major, file-minor;
                    group_video / group_file (G,) int64;  group_off (V + 1) int64: video v owns groups
                    [group_off[v], group_off[v + 1]) -- at least one
    video_groups    (V, 4) int32: the whole videos (all files' references of the video)
    n_files         the number of ground-truth files
    .on(device) gives the device copies (pred_seg, ref_seg, ops.TiouGroups of file_groups, of video_groups), made at first
    use and kept."""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self._dev = {}

    def on(self, device):
        import torch
        from . import ops
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.pred_seg).to(device), torch.from_numpy(self.ref_seg).to(device),
                              ops.TiouGroups(self.file_groups, device), ops.TiouGroups(self.video_groups, device))
        return self._dev[key]


def proposal_score_of(pred: dict) -> float:
    """a prediction's "proposal_score": a one-element list or tuple counts as its element, a missing key as 0.0"""
    score = pred.get("proposal_score", 0.0)
    if isinstance(score, (list, tuple)):
        score = score[0]
    return float(score)


def by_proposal_score(preds: Sequence[dict]) -> List[int]:
    """the positions ordered by proposal_score descending; ties keep list order"""
    scores = [proposal_score_of(p) for p in preds]
    return sorted(range(len(preds)), key=lambda k: -scores[k])


def segment_tables(ground_truths: Sequence[dict], prediction: Dict[str, list], by_score: bool = False) -> SegmentTables:
    """The segment arrays and both group tables of a job (see SegmentTables).  `prediction` is already cut to max_proposals
    per video.  The predictions of a video keep list order, or are ordered by_proposal_score when by_score; videos that only
    the prediction holds are left out.  Nothing here depends on a threshold: the tables serve every tIoU and metric."""
    vids = ground_truth_video_ids(ground_truths)
    pred_seg, pred_sent, pred_off = [], [], [0]
    ref_seg, ref_sent, ref_file, ref_off = [], [], [], [0]
    groups, group_video, group_file, group_off, video_groups = [], [], [], [0], []
    for v, vid in enumerate(vids):
        preds = prediction.get(vid, ())
        order = by_proposal_score(preds) if by_score else range(len(preds))
        p0, r_start = len(pred_seg), len(ref_seg)
        for k in order:
            pred_seg.append((float(preds[k]["timestamp"][0]), float(preds[k]["timestamp"][1])))
            pred_sent.append(preds[k].get("sentence", ""))
        for f, gt in enumerate(ground_truths):
            if vid not in gt:
                continue
            stamps = gt[vid]["timestamps"]
            groups.append((p0, len(preds), len(ref_seg), len(stamps)))
            group_video.append(v)
            group_file.append(f)
            for idx, stamp in enumerate(stamps):
                ref_seg.append((float(stamp[0]), float(stamp[1])))
                ref_sent.append(gt[vid]["sentences"][idx] if "sentences" in gt[vid] else "")
                ref_file.append(f)
        video_groups.append((p0, len(preds), r_start, len(ref_seg) - r_start))
        pred_off.append(len(pred_seg))
        ref_off.append(len(ref_seg))
        group_off.append(len(groups))
    i64 = lambda a: np.asarray(a, dtype=np.int64)                                                         # noqa: E731
    pred_off = i64(pred_off)
    return SegmentTables(
        vids=vids, pred_seg=np.asarray(pred_seg, dtype=np.float64).reshape(-1, 2),
        pred_video=np.repeat(np.arange(len(vids), dtype=np.int64), np.diff(pred_off)), pred_off=pred_off,
        pred_sentences=pred_sent, ref_seg=np.asarray(ref_seg, dtype=np.float64).reshape(-1, 2), ref_file=i64(ref_file),
        ref_off=i64(ref_off), ref_sentences=ref_sent, file_groups=np.asarray(groups, dtype=np.int32).reshape(-1, 4),
        group_video=i64(group_video), group_file=i64(group_file), group_off=i64(group_off),
        video_groups=np.asarray(video_groups, dtype=np.int32).reshape(-1, 4), n_files=len(ground_truths))


def _tiou_hits(pred_seg, ref_seg, groups, tious: Sequence[float], strict: bool):
    """ops.tiou_hits for any number of thresholds (launches of at most ops.TIOU_MAX_T): the two tables on the host"""
    import torch
    from . import ops
    tious = np.asarray(tious, dtype=np.float64)
    hits, first = [], []
    for lo in range(0, len(tious), ops.TIOU_MAX_T):
        h, f = ops.tiou_hits(pred_seg, ref_seg, groups, torch.from_numpy(tious[lo:lo + ops.TIOU_MAX_T]).to(pred_seg.device),
                             strict)
        hits.append(h)
        first.append(f)
    return torch.cat(hits).cpu().numpy(), torch.cat(first).cpu().numpy()


def _group_sums(flags: np.ndarray, counts: np.ndarray) -> np.ndarray:
    """(T, G) int64: per row of flags (T, sum counts) the number of set entries in each group's run (empty runs give 0)"""
    c = np.zeros((flags.shape[0], flags.shape[1] + 1), dtype=np.int64)
    np.cumsum(flags, axis=1, out=c[:, 1:])
    off = np.concatenate([[0], np.cumsum(counts)])
    return c[:, off[1:]] - c[:, off[:-1]]


def detection_scores_device(tables: SegmentTables, tious: Sequence[float], device="cuda") -> List[Tuple[float, float]]:
    """[(precision, recall)] per tIoU, the values of detection_scores: one strict launch over the (video, file) groups and
    every threshold; per group #(pred_hits > 0) / P and #(ref_first < P) / R, the best over a video's files, the mean over
    the ground-truth videos in their order (0 precision for a video without predictions) -- that function's float
    expressions over the launch's integers."""
    pred_seg, ref_seg, file_groups, _ = tables.on(device)
    hits, first = _tiou_hits(pred_seg, ref_seg, file_groups, tious, True)
    P, R = tables.file_groups[:, 1].astype(np.int64), tables.file_groups[:, 3].astype(np.int64)
    if (R == 0).any():
        raise ZeroDivisionError("a ground-truth video without timestamps")      # as detection_scores on that file
    preds_hit = _group_sums(hits > 0, P)
    refs_hit = _group_sums(first < np.repeat(P, R)[None, :], R)
    starts = tables.group_off[:-1]
    out = []
    for t in range(len(tious)):
        p = np.where(P > 0, preds_hit[t].astype(np.float64) / np.maximum(P, 1), 0.0)
        r = refs_hit[t].astype(np.float64) / R
        best_p, best_r = np.maximum.reduceat(p, starts).tolist(), np.maximum.reduceat(r, starts).tolist()
        out.append((sum(best_p) / len(best_p), sum(best_r) / len(best_r)))
    return out


def pair_indices_device(tables: SegmentTables, tiou_threshold: float, device="cuda") -> Tuple[np.ndarray, np.ndarray]:
    """(pred_index, ref_index) int64 arrays of a threshold's pairs in pair_captions' order (video, prediction, file,
    caption): rows of tables.pred_seg and of tables.ref_seg, ref_index -1 for the one pair of a prediction that reaches no
    reference.  Two launches over the whole videos: the hit counts (ops.tiou_hits, >=), their running sum
    (torch.cumsum), and the rows written in order (ops.tiou_pairs)."""
    import torch
    from . import ops
    pred_seg, ref_seg, _, video_groups = tables.on(device)
    NP = video_groups.sum_p
    if NP == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    tiou_threshold = float(tiou_threshold)
    hits, _ = ops.tiou_hits(pred_seg, ref_seg, video_groups, torch.tensor([tiou_threshold], dtype=torch.float64, device=device),
                            False)
    counts = hits[0].clamp(min=1).to(torch.int64)
    pair_off = torch.zeros(NP + 1, dtype=torch.int64, device=device)
    torch.cumsum(counts, 0, out=pair_off[1:])
    counts_h = counts.cpu().numpy()
    pair_ref = ops.tiou_pairs(pred_seg, ref_seg, video_groups, tiou_threshold, pair_off, int(counts_h.sum()))
    # a video's predictions are the rows pred_off[v] .. of pred_seg, and the video groups are laid out in that order
    return np.repeat(np.arange(NP, dtype=np.int64), counts_h), pair_ref.cpu().numpy().astype(np.int64)


def _trapezoid(y: Sequence[float], x: Sequence[float]) -> float:
    """the trapezoid rule, summed left to right"""
    total = 0.0
    for k in range(len(x) - 1):
        total += (x[k + 1] - x[k]) * (y[k + 1] + y[k]) / 2.0
    return total


def proposal_recall(ground_truths: Sequence[dict], prediction: Dict[str, list], tious: Sequence[float],
                    max_avg_nr_proposals: int = 100, points: int = 100, device="cuda") -> dict:
    """Average recall against the average number of proposals per video (AR@AN) and the area under that curve (AUC), the
    ActivityNet proposal metric, per tIoU: {"AUC": [T], "AR@AN": [T], "recall_curve": (T, points),
    "proposals_per_video": (points,)}.  `prediction` is already cut to max_proposals per video.

    Per ground-truth file, with V its videos and total the number of predictions over them:
    ratio = max_avg_nr_proposals * float(V) / total, pcn_k = (k / float(points)) * ratio for k = 1 .. points.  A video's
    predictions are ordered by proposal_score descending (by_proposal_score); at point k its first
    nr = int(min(P_v * pcn_k, P_v)) count.  A reference is matched at (t, k) when some counted prediction has
    tIoU >= tious[t] with it, that is when its first rank (ops.tiou_hits, one launch for all thresholds) is < nr;
    recall[t][k] = matched / (references of the file).  A video without predictions contributes its references and no
    match; total == 0 (or a file without references) gives a curve of zeros.  x_k = pcn_k * (float(total) / V),
    AUC_t = 100 * trapezoid(recall[t], x) / x[-1] (summed left to right), AR@AN_t = recall[t][-1].

    With several files the curves, x and both figures are the plain mean over the files: this package's convention for
    ActivityNet Captions' two annotation files, not part of the published metric.  The figure is comparable to
    ActivityNet's only with its ten thresholds 0.5, 0.55 .. 0.95 and ONE annotation file, and the tIoU is `tiou` of this
    module with its + 1e-8 in the denominator, where ActivityNet's has none."""
    T = len(tious)
    tables = segment_tables(ground_truths, prediction, by_score=True)
    pred_seg, ref_seg, file_groups, _ = tables.on(device)
    _, first = _tiou_hits(pred_seg, ref_seg, file_groups, tious, False)
    P, R = tables.file_groups[:, 1].astype(np.int64), tables.file_groups[:, 3].astype(np.int64)
    ref_group = np.repeat(np.arange(len(P)), R)                 # the group of every slot of `first`
    curves, xs, aucs, ars = [], [], [], []
    for f in range(tables.n_files):
        mine = np.nonzero(tables.group_file == f)[0]
        V, total, n_refs = len(mine), int(P[mine].sum()), int(R[mine].sum())
        recall = np.zeros((T, points), dtype=np.float64)
        x = np.zeros(points, dtype=np.float64)
        auc = [0.0] * T
        if total > 0 and n_refs > 0:
            ratio = max_avg_nr_proposals * float(V) / total
            pcn = np.array([(k / float(points)) * ratio for k in range(1, points + 1)], dtype=np.float64)
            nr = np.minimum(P[mine, None] * pcn[None, :], P[mine, None]).astype(np.int64)              # (V, points), int()
            slots = np.nonzero(tables.group_file[ref_group] == f)[0]
            nr_of_slot = nr[np.searchsorted(mine, ref_group[slots])]                                    # (refs, points)
            for t in range(T):
                matched = (first[t, slots, None] < nr_of_slot).sum(axis=0)
                recall[t] = matched / float(n_refs)
            x = pcn * (float(total) / V)
            auc = [100.0 * _trapezoid(recall[t].tolist(), x.tolist()) / float(x[-1]) for t in range(T)]
        curves.append(recall)
        xs.append(x)
        aucs.append(auc)
        ars.append([float(recall[t][-1]) for t in range(T)])
    n = float(len(curves))
    mean = lambda parts: sum(parts[1:], parts[0]) / n                                                  # noqa: E731
    return {"AUC": [sum(a[t] for a in aucs) / n for t in range(T)], "AR@AN": [sum(a[t] for a in ars) / n for t in range(T)],
            "recall_curve": mean(curves), "proposals_per_video": mean(xs)}


def _load(x):
    if isinstance(x, dict):
        return x
    with open(x) as f:
        return json.load(f)


class DenseCaptionEvaluator:
    """ANETcaptions of the reference's evaluation/evaluate.py: the same positional arguments, .evaluate() and .scores (a
    dict of lists, one entry per tIoU: Bleu_1..4, METEOR, ROUGE_L, CIDEr, and with verbose or only_proposals also Recall
    and Precision).  A ground-truth entry or the prediction may be an already loaded dict instead of a path.
    tokenizer: sentence -> list of words (default: tokenize).  stemmer / synonyms: as rewards.MeteorTables takes them
    (None: nltk's, an ImportError naming the two keywords when nltk is missing; False: the stage is off).
    soda=True (and not only_proposals): .evaluate() also fills SODA_c, SODA_c_Precision and SODA_c_Recall, one entry per
    tIoU, and .soda_per_video (video id -> [(precision, recall, F) per tIoU]); sort_references=True orders a video's
    references by (start, end) like its predictions instead of keeping the file's order.
    tiou_backend="device": evaluate_detection and tokenized_pairs read the tIoU tables of one device launch
    (segment_tables, detection_scores_device, pair_indices_device) instead of walking the interval
    pairs in Python; the values are the same.  "host" (default) runs the Python loops.
    proposal_recall=True: .evaluate() also fills AUC and AR@AN, one entry per tIoU, .recall_curve (T, points) and
    .proposals_per_video (points,): proposal_recall below with its defaults, which see for the definition.  The mean of AUC
    over the tIoUs is comparable to ActivityNet's proposal figure only with its ten thresholds 0.5 .. 0.95 and one
    annotation file; the tIoU is `tiou` with its + 1e-8.
    paragraph=True (and not only_proposals): .evaluate() also fills Para_Bleu_1..4, Para_METEOR, Para_ROUGE_L, Para_CIDEr
    (a video's captions in time order read as one paragraph, scored per ground-truth file and averaged over the files) and
    Para_RE_4, Para_XRE_4, Para_Div_1, Para_Div_2 (n-gram repetition, repetition across sentences and diversity of the
    predicted paragraphs: paragraph_groups, paragraph_scores, paragraph_stats, paragraph_means), one
    entry per tIoU, all equal, and .paragraph_per_video (video id -> {"stats": (4, 5) int32 total, distinct, in_repeated,
    cross, max_count per n, "sentences", "tokens"}).  paragraph_top=k reads only the k best-scored proposals of a video
    (by_proposal_score) as its paragraph; None reads all.  sort_references applies to the reference paragraphs too.
    .per_video (after .evaluate(), not only_proposals) keeps the per-video values the means were taken of: family ->
    (video ids, {metric: [fp64 array per tIoU]}) for "tiou" (the seven METRICS over tokenized_pairs' videos), "soda" (the
    SODA_METRICS over .soda_per_video's videos) and "paragraph" (Para_RE_4 / Para_XRE_4 / Para_Div_1 / Para_Div_2 as (2, N)
    arrays of value and weight: paragraph_values).  bootstrap=R: .evaluate() also fills .intervals = bootstrap(self, R,
    bootstrap_seed, bootstrap_alpha) below, {metric: [dict(value, lo, hi, se) per tIoU]} (what is
    out of its scope: see bootstrap).  .scores and the printed lines are the same with and without it."""

    def __init__(self, ground_truth_filenames=None, prediction_filename=None, tious=None, max_proposals=1000,
                 prediction_fields=PREDICTION_FIELDS, verbose=False, only_proposals=False, *, device="cuda",
                 tokenizer: Callable[[str], List[str]] = tokenize, stemmer=None, synonyms=None, soda=False,
                 sort_references=False, tiou_backend="host", proposal_recall=False, paragraph=False, paragraph_top=None,
                 bootstrap=None, bootstrap_seed=0, bootstrap_alpha=0.05):
        if tious is None or len(tious) == 0:
            raise IOError("Please input a valid tIoU.")
        if not ground_truth_filenames:
            raise IOError("Please input a valid ground truth file.")
        if not prediction_filename:
            raise IOError("Please input a valid prediction file.")
        self.only_proposals = only_proposals
        self.verbose = verbose
        self.tious = tious
        self.max_proposals = max_proposals
        self.pred_fields = prediction_fields
        self.device = device
        self.tokenizer = tokenizer
        self._stemmer, self._synonyms = stemmer, synonyms
        self.soda, self.sort_references = bool(soda), bool(sort_references)
        self.soda_per_video: Dict[str, List[Tuple[float, float, float]]] = {}
        if tiou_backend not in ("host", "device"):
            raise ValueError(f"unknown tiou_backend {tiou_backend!r} ('host' or 'device')")
        self.tiou_backend, self.proposal_recall = tiou_backend, bool(proposal_recall)
        self.recall_curve = self.proposals_per_video = None
        if paragraph_top is not None and (isinstance(paragraph_top, bool) or not isinstance(paragraph_top, (int, np.integer))
                                          or paragraph_top < 1):
            raise ValueError(f"paragraph_top {paragraph_top!r}: a positive integer or None expected")
        self.paragraph, self.paragraph_top = bool(paragraph), None if paragraph_top is None else int(paragraph_top)
        self.paragraph_per_video: Dict[str, dict] = {}
        if bootstrap is not None and (isinstance(bootstrap, bool) or not isinstance(bootstrap, (int, np.integer))
                                      or bootstrap < 1):
            raise ValueError(f"bootstrap {bootstrap!r}: a positive number of resamples or None expected")
        if not 0.0 < bootstrap_alpha < 1.0:
            raise ValueError(f"bootstrap_alpha {bootstrap_alpha!r}: a number in (0, 1) expected")
        self.bootstrap = None if bootstrap is None else int(bootstrap)
        self.bootstrap_seed, self.bootstrap_alpha = int(bootstrap_seed), float(bootstrap_alpha)
        self.per_video: Dict[str, tuple] = {}
        self.intervals: Dict[str, List[dict]] = {}
        self._tables = self._detection = self._table_tokens = None
        self.ground_truths = self.import_ground_truths(ground_truth_filenames)
        self.prediction = self.import_prediction(prediction_filename)
        self._tokens: Dict[str, Tuple[str, ...]] = {}
        self._meteor_tables = None
        self.scores: Dict[str, list] = {}
        if not only_proposals:
            self.meteor_tables()              # a missing stemmer / synonym source is reported here, not after the pairing

    # ---- loading
    def import_prediction(self, prediction_filename) -> Dict[str, list]:
        if self.verbose:
            print("| Loading submission...")
        try:
            submission = _load(prediction_filename)
        except OSError as e:
            raise IOError(f"Please input a valid prediction file. ({e})") from e
        if not all(field in submission.keys() for field in self.pred_fields):
            raise IOError("Please input a valid ground truth file.")
        return {vid: segs[:self.max_proposals] for vid, segs in submission["results"].items()}

    def import_ground_truths(self, filenames) -> List[dict]:
        if isinstance(filenames, (str, dict)):
            filenames = [filenames]
        gts = []
        self.n_ref_vids = set()
        for filename in filenames:
            try:
                gt = _load(filename)
            except OSError as e:
                raise IOError(f"Please input a valid ground truth file. ({e})") from e
            self.n_ref_vids.update(gt.keys())
            gts.append(gt)
        if self.verbose:
            print("| Loading GT. #files: %d, #videos: %d" % (len(gts), len(self.n_ref_vids)))
        return gts

    def get_gt_vid_ids(self) -> List[str]:
        return ground_truth_video_ids(self.ground_truths)

    # ---- scoring
    def evaluate(self) -> None:
        self.scores = {}
        self.per_video, self.intervals = {}, {}
        if not self.only_proposals:
            vids, kept = [], {m: [] for m in METRICS}
            for t in self.tious:
                out, vids, values = self.tiou_scores(t)
                for metric, score in out.items():
                    self.scores.setdefault(metric, []).append(score)
                for m in METRICS:
                    kept[m].append(values[m])
            self.per_video["tiou"] = (vids, kept)
            if self.soda:
                self.scores.update(self.evaluate_soda())
                self.per_video["soda"] = soda_values(self.soda_per_video, len(self.tious))
            if self.paragraph:
                self.scores.update(self.evaluate_paragraph())
                self.per_video["paragraph"] = paragraph_values(self.paragraph_per_video, len(self.tious))
            if self.bootstrap is not None:
                self.intervals = bootstrap(self, self.bootstrap, self.bootstrap_seed, self.bootstrap_alpha)
        if self.verbose:
            self.scores["Recall"], self.scores["Precision"] = [], []
            for t in self.tious:
                precision, recall = self.evaluate_detection(t)
                self.scores["Recall"].append(recall)
                self.scores["Precision"].append(precision)
        if self.proposal_recall:
            out = proposal_recall(self.ground_truths, self.prediction, self.tious, device=self.device)
            self.scores["AUC"], self.scores["AR@AN"] = out["AUC"], out["AR@AN"]
            self.recall_curve, self.proposals_per_video = out["recall_curve"], out["proposals_per_video"]

    def segment_tables(self) -> SegmentTables:
        """the job's segment_tables, built at first use (the device routes share them across thresholds and metrics)"""
        if self._tables is None:
            self._tables = segment_tables(self.ground_truths, self.prediction)
        return self._tables

    def evaluate_detection(self, tiou_threshold) -> Tuple[float, float]:
        if self.tiou_backend == "host":
            return detection_scores(self.ground_truths, self.prediction, tiou_threshold)
        if self._detection is None:            # one launch for all of the evaluator's thresholds
            tious = [float(t) for t in self.tious]
            self._detection = dict(zip(tious, detection_scores_device(self.segment_tables(), tious, self.device)))
        key = float(tiou_threshold)
        if key not in self._detection:
            self._detection[key] = detection_scores_device(self.segment_tables(), [key], self.device)[0]
        return self._detection[key]

    def _tok(self, sentence: str) -> Tuple[str, ...]:
        t = self._tokens.get(sentence)
        if t is None:
            t = self._tokens[sentence] = tuple(self.tokenizer(sentence))
        return t

    def tokenized_pairs(self, tiou_threshold):
        """(video ids, group_off, hypothesis token tuples, reference token tuples) of a threshold's pairs; the groups are
        the ground-truth videos in sorted order, those without a pair included (empty)"""
        if self.tiou_backend == "device":
            return self._tokenized_pairs_device(tiou_threshold)
        paired = pair_captions(self.ground_truths, self.prediction, tiou_threshold)
        vids = list(paired)
        off = [0]
        hyps, refs = [], []
        for vid in vids:
            for hyp, ref in paired[vid]:
                hyps.append(self._tok(hyp))
                refs.append((GARBAGE,) if ref is None else self._tok(ref))
            off.append(len(hyps))
        return vids, off, hyps, refs

    def _tokenized_pairs_device(self, tiou_threshold):
        tables = self.segment_tables()
        if self._table_tokens is None:         # every sentence of the tables, tokenized once
            self._table_tokens = ([self._tok(remove_nonascii(s)) for s in tables.pred_sentences],
                                  [self._tok(remove_nonascii(s)) for s in tables.ref_sentences])
        hyp_tok, ref_tok = self._table_tokens
        pred_index, ref_index = pair_indices_device(tables, tiou_threshold, self.device)
        per_video = np.bincount(tables.pred_video[pred_index], minlength=len(tables.vids))
        off = [0] + np.cumsum(per_video).tolist()
        hyps = [hyp_tok[i] for i in pred_index.tolist()]
        refs = [(GARBAGE,) if r < 0 else ref_tok[r] for r in ref_index.tolist()]
        return list(tables.vids), off, hyps, refs

    def evaluate_tiou(self, tiou_threshold) -> Dict[str, float]:
        return self.tiou_scores(tiou_threshold)[0]

    def tiou_scores(self, tiou_threshold):
        """(evaluate_tiou's dictionary, the video ids, {metric: (N,) fp64 per-video values}): the means of a threshold and
        what they were taken of, over tokenized_pairs' video list"""
        vids, off, hyps, refs = self.tokenized_pairs(tiou_threshold)
        if not hyps:                           # nothing was predicted for any ground-truth video: every video scores 0
            return {m: 0.0 for m in METRICS}, vids, {m: np.zeros(len(vids), dtype=np.float64) for m in METRICS}
        per_video = score_pairs(hyps, refs, off, self.device, self.meteor_tables())
        out = {m: float(np.mean(per_video[m])) for m in METRICS}
        if self.verbose:
            for m in METRICS:
                print("Calculated tIoU: %1.1f, %s: %0.3f" % (tiou_threshold, m, out[m]))
        return out, vids, {m: np.asarray(per_video[m], dtype=np.float64) for m in METRICS}

    def evaluate_soda(self) -> Dict[str, List[float]]:
        """SODA_c, SODA_c_Precision, SODA_c_Recall per tIoU and .soda_per_video"""
        groups, by_video = soda_groups(self.ground_truths, self.prediction, self.sort_references)
        per_group = soda_scores(groups, self.tious, self.meteor_tables(), self.device, self._tok)
        self.soda_per_video = soda_per_video(by_video, per_group, len(self.tious))
        out = soda_means(self.soda_per_video, len(self.tious))
        if self.verbose:
            for k, t in enumerate(self.tious):
                for m in SODA_METRICS:
                    print("Calculated tIoU: %1.1f, %s: %0.3f" % (t, m, out[m][k]))
        return out

    def evaluate_paragraph(self) -> Dict[str, List[float]]:
        """the Para_* keys, one entry per tIoU -- all equal: a paragraph does not depend on a
        threshold -- and .paragraph_per_video"""
        groups = paragraph_groups(self.ground_truths, self.prediction, self._tok, self.paragraph_top, self.sort_references)
        out = paragraph_scores(groups, self.device, self.meteor_tables())
        stats = paragraph_stats([groups.predicted[vid] for vid in groups.vids], self.device)
        out.update(paragraph_means(stats))
        self.paragraph_per_video = {
            vid: {"stats": stats[v].copy(), "sentences": len(groups.predicted[vid]),
                  "tokens": sum(map(len, groups.predicted[vid]))} for v, vid in enumerate(groups.vids)}
        if self.verbose:
            for m, score in out.items():
                print("Calculated %s: %0.3f" % (m, score))
        return {m: [score] * len(self.tious) for m, score in out.items()}

    def meteor_tables(self):
        """rewards.MeteorTables over the distinct hypothesis words of the submission (built at first use)"""
        if self._meteor_tables is None:
            from .rewards import MeteorTables
            words: Dict[str, None] = {}
            for vid in sorted(self.prediction):
                for seg in self.prediction[vid]:
                    for w in self._tok(remove_nonascii(seg["sentence"])):
                        words.setdefault(w.lower())
            self._meteor_tables = MeteorTables(list(words), self._stemmer, self._synonyms)
        return self._meteor_tables


def _distinct(seqs: Sequence[Sequence[str]]):
    """(the distinct token tuples in order of first appearance, (len(seqs),) int64 index of every sequence among them)"""
    index: Dict[Tuple[str, ...], int] = {}
    idx = np.empty(len(seqs), dtype=np.int64)
    for p, s in enumerate(seqs):
        idx[p] = index.setdefault(tuple(s), len(index))
    return list(index), idx


def _rows(sents, ids_of, dtype, fill):
    """(n, max(1, longest)) matrix of ids_of(sentence), padded with fill, and the (n,) lengths"""
    lens = np.array([len(s) for s in sents], dtype=np.int64)
    out = np.full((len(sents), max(1, int(lens.max()))), fill, dtype=dtype)
    for i, s in enumerate(sents):
        out[i, :len(s)] = ids_of(s)
    return out, lens


def encode_pairs(hyps: Sequence[Sequence[str]], refs: Sequence[Sequence[str]]):
    """word ids of one rewards.StringTable over every token of the call: hyp (P, L) / ref (P, R) int32 (zero padded, L and
    R at least 1) and their lengths.  Every distinct sentence is encoded once."""
    from . import ops
    from .rewards import StringTable
    table = StringTable()
    (hs, hi), (rs, ri) = _distinct(hyps), _distinct(refs)
    ids_of = lambda s: [table.add(w) for w in s]                                                          # noqa: E731
    (wh, lh), (wr, lr) = _rows(hs, ids_of, np.int32, 0), _rows(rs, ids_of, np.int32, 0)
    if wh.shape[1] > ops.REWARDS_MAX_L or wr.shape[1] > ops.REWARDS_MAX_R:
        raise ValueError(f"a sentence of {wh.shape[1]} / a reference of {wr.shape[1]} tokens; at most {ops.REWARDS_MAX_L} / "
                         f"{ops.REWARDS_MAX_R} are supported")
    return wh[hi], lh[hi].astype(np.int32), wr[ri], lr[ri].astype(np.int32)


def meteor_pairs(hyps: Sequence[Sequence[str]], refs: Sequence[Sequence[str]], tables, device) -> np.ndarray:
    """(P,) fp64: the METEOR score of every whole hypothesis against its reference, through the per-prefix launch
    (ops.meteor): the pair's score is the row's column hyp_len - 1; an empty hypothesis scores 0.  `tables`: a
    rewards.MeteorTables whose vocabulary holds every hypothesis word."""
    import torch
    from . import ops
    from .rewards import MeteorScorer
    P = len(hyps)
    out = np.zeros(P, dtype=np.float64)
    word_vocab = {}
    for v, wid in enumerate(tables.vmap):      # word id -> a vocab id that yields it
        if wid >= 0:
            word_vocab.setdefault(int(wid), v)
    (hs, hi), (rs, ri) = _distinct(hyps), _distinct(refs)
    ref_w, ref_s = tables.encode([" ".join(r) for r in rs])
    # hypothesis rows of vocab ids (-1: outside the vocabulary, yields no word); reference rows of word and stem ids
    wh, lh = _rows(hs, lambda s: [word_vocab[tables.strings[w.lower()]] for w in s], np.int64, -1)
    ww, lr = _rows(ref_w, lambda s: s, np.int32, 0)
    ws, _ = _rows(ref_s, lambda s: s, np.int32, 0)
    if wh.shape[1] > ops.REWARDS_MAX_L:
        raise ValueError(f"a sentence of {wh.shape[1]} tokens; at most {ops.REWARDS_MAX_L} are supported")
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)          # noqa: E731
    vmap, vstem, syn_off, syn_ids = dev(tables.vmap), dev(tables.vstem), dev(tables.syn_off), dev(tables.syn_ids)
    for lo in range(0, P, _METEOR_CHUNK):
        h, r = hi[lo:lo + _METEOR_CHUNK], ri[lo:lo + _METEOR_CHUNK]
        B, L, R = len(h), max(1, int(lh[h].max())), max(1, int(lr[r].max()))
        hyp_len = lh[h]
        hyp_d, ref_d, stem_d = dev(wh[h, :L]), dev(ww[r, :R]), dev(ws[r, :R])
        scores = torch.empty(B, L, dtype=torch.float64, device=device)
        delta = torch.empty(B, L, dtype=torch.float32, device=device)
        ops.meteor(hyp_d, vmap, vstem, syn_off, syn_ids, ref_d, stem_d if vstem is not None else None,
                   dev(lr[r].astype(np.int32)), MeteorScorer.alpha, MeteorScorer.beta, MeteorScorer.gamma_frag, scores, delta)
        whole = scores.gather(1, dev(np.maximum(hyp_len - 1, 0))[:, None])[:, 0].cpu().numpy()
        out[lo:lo + B] = np.where(hyp_len > 0, whole, 0.0)
    return out


def score_pairs(hyps, refs, group_off: Sequence[int], device, tables) -> Dict[str, np.ndarray]:
    """per-group values of the seven metrics, (G,) fp64 each, of the pairs hyps[p] / refs[p] (token sequences) grouped by
    group_off (G + 1, ascending from 0 to the number of pairs; an empty group scores 0).  One caption_eval call and the
    METEOR launches; at least one pair."""
    import torch
    from . import ops
    hyp, hyp_len, ref, ref_len = encode_pairs(hyps, refs)
    off = np.asarray(group_off, dtype=np.int32)
    dev = lambda a: torch.from_numpy(a).to(device)                                                         # noqa: E731
    _, _, _, group_scores = ops.caption_eval(dev(hyp), dev(hyp_len), dev(ref), dev(ref_len), dev(off))
    meteor = meteor_pairs(hyps, refs, tables, device)
    gs = group_scores.cpu().numpy()
    counts = np.diff(off)
    sums = np.zeros(len(counts), dtype=np.float64)
    for g in np.nonzero(counts)[0]:            # pair order within a group
        sums[g] = sum(meteor[off[g]:off[g + 1]].tolist())
    out = {f"Bleu_{k + 1}": gs[:, k].copy() for k in range(4)}
    out["METEOR"] = sums / np.maximum(counts, 1)
    out["ROUGE_L"] = gs[:, 4].copy()
    out["CIDEr"] = gs[:, 5].copy()
    return out


# ---- SODA_c
class SodaGroup(NamedTuple):
    """one (video, ground-truth file): the predictions in time order, the references in story order"""
    video: str
    file: int
    pred_segments: List[Tuple[float, float]]
    pred_sentences: List[str]
    ref_segments: List[Tuple[float, float]]
    ref_sentences: List[str]


def _by_time(stamps) -> List[int]:
    """the positions ordered by (start, end) ascending; ties keep their order"""
    return sorted(range(len(stamps)), key=lambda k: (float(stamps[k][0]), float(stamps[k][1])))


def soda_groups(ground_truths: Sequence[dict], prediction: Dict[str, list], sort_references: bool = False
                ) -> Tuple[List[SodaGroup], Dict[str, List[int]]]:
    """the host half of SODA_c: (groups, video id -> indices of its groups in file order) for every ground-truth video id
    (sorted).  `prediction` is already cut to max_proposals per video.  A group exists for every file that holds the video
    with at least one caption, when the video has a prediction; predictions are ordered by (start, end), stable;
    references keep the file's order unless sort_references.  Sentences have passed remove_nonascii.  Videos that only the
    prediction holds are left out."""
    groups: List[SodaGroup] = []
    by_video: Dict[str, List[int]] = {}
    for vid in ground_truth_video_ids(ground_truths):
        mine = by_video[vid] = []
        preds = prediction.get(vid, ())
        if not len(preds):
            continue
        order = _by_time([p["timestamp"] for p in preds])
        segs = [(float(preds[k]["timestamp"][0]), float(preds[k]["timestamp"][1])) for k in order]
        sents = [remove_nonascii(preds[k]["sentence"]) for k in order]
        for f, gt in enumerate(ground_truths):
            if vid not in gt or not len(gt[vid]["timestamps"]):
                continue
            stamps = gt[vid]["timestamps"]
            rorder = _by_time(stamps) if sort_references else range(len(stamps))
            mine.append(len(groups))
            groups.append(SodaGroup(vid, f, segs, sents, [(float(stamps[k][0]), float(stamps[k][1])) for k in rorder],
                                    [remove_nonascii(gt[vid]["sentences"][k]) for k in rorder]))
    return groups, by_video


def soda_encode(groups: Sequence[SodaGroup], tables, tokenizer: Callable[[str], Sequence[str]] = tokenize) -> dict:
    """the distinct sentences of the groups as id rows (host): "hyp" (Nh, L) int64 vocab ids (-1 pads) with "hyp_len",
    "ref" / "ref_stem" (Nr, R) int32 word / stem ids with "ref_len", and "members": per group the indices of its
    hypotheses and of its references among them.  Every distinct sentence is tokenized and encoded once."""
    from . import ops
    tokens: Dict[str, Tuple[str, ...]] = {}

    def tok(sentence):
        t = tokens.get(sentence)
        if t is None:
            t = tokens[sentence] = tuple(tokenizer(sentence))
        return t
    hyp_index: Dict[Tuple[str, ...], int] = {}
    ref_index: Dict[Tuple[str, ...], int] = {}
    members = []                                # per group: indices of its hypotheses, of its references
    for g in groups:
        if len(g.ref_sentences) > ops.SODA_MAX_REFS:
            raise ValueError(f"video {g.video}: {len(g.ref_sentences)} references in ground-truth file {g.file}; at most "
                             f"{ops.SODA_MAX_REFS} are supported")
        hs, rs = [tok(s) for s in g.pred_sentences], [tok(s) for s in g.ref_sentences]
        if max(map(len, hs)) > ops.REWARDS_MAX_L or max(map(len, rs)) > ops.REWARDS_MAX_R:
            raise ValueError(f"video {g.video}: a sentence of {max(map(len, hs))} / a reference of {max(map(len, rs))} "
                             f"tokens; at most {ops.REWARDS_MAX_L} / {ops.REWARDS_MAX_R} are supported")
        members.append((np.array([hyp_index.setdefault(h, len(hyp_index)) for h in hs], dtype=np.int32),
                        np.array([ref_index.setdefault(r, len(ref_index)) for r in rs], dtype=np.int32)))
    word_vocab = {}
    for v, wid in enumerate(tables.vmap):      # word id -> a vocab id that yields it
        if wid >= 0:
            word_vocab.setdefault(int(wid), v)
    ref_w, ref_s = tables.encode([" ".join(r) for r in ref_index])
    wh, lh = _rows(list(hyp_index), lambda s: [word_vocab[tables.strings[w.lower()]] for w in s], np.int64, -1)
    ww, lr = _rows(ref_w, lambda s: s, np.int32, 0)
    ws, _ = _rows(ref_s, lambda s: s, np.int32, 0)
    return {"hyp": wh, "hyp_len": lh, "ref": ww, "ref_stem": ws, "ref_len": lr.astype(np.int32), "members": members}


def soda_chunks(groups: Sequence[SodaGroup], encoded: dict, max_cells: int = _SODA_CELLS):
    """the groups in runs of at most max_cells cells (one group at least): yields (lo, hi, arrays) with the host operands
    of the two launches for groups[lo:hi] -- hyp_idx, ref_idx, hyp_off, ref_off, cell_off, pred_seg, ref_seg -- and the
    longest hypothesis "L" and reference "R" among them"""
    members = encoded["members"]
    off = lambda n, dt: np.concatenate([[0], np.cumsum(n)]).astype(dt)                                    # noqa: E731
    lo = 0
    while lo < len(groups):
        hi, cells = lo, 0
        while hi < len(groups) and (hi == lo or cells + len(members[hi][0]) * len(members[hi][1]) <= max_cells):
            cells += len(members[hi][0]) * len(members[hi][1])
            hi += 1
        hyp_idx = np.concatenate([members[g][0] for g in range(lo, hi)])
        ref_idx = np.concatenate([members[g][1] for g in range(lo, hi)])
        P = np.array([len(members[g][0]) for g in range(lo, hi)], dtype=np.int64)
        R = np.array([len(members[g][1]) for g in range(lo, hi)], dtype=np.int64)
        yield lo, hi, {
            "hyp_idx": hyp_idx, "ref_idx": ref_idx, "hyp_off": off(P, np.int32), "ref_off": off(R, np.int32),
            "cell_off": off(P * R, np.int64),
            "pred_seg": np.array([s for g in groups[lo:hi] for s in g.pred_segments], dtype=np.float64).reshape(-1, 2),
            "ref_seg": np.array([s for g in groups[lo:hi] for s in g.ref_segments], dtype=np.float64).reshape(-1, 2),
            "L": max(1, int(encoded["hyp_len"][hyp_idx].max())), "R": max(1, int(encoded["ref_len"][ref_idx].max()))}
        lo = hi


def soda_scores(groups: Sequence[SodaGroup], tious: Sequence[float], tables, device,
                tokenizer: Callable[[str], Sequence[str]] = tokenize, max_cells: int = _SODA_CELLS) -> np.ndarray:
    """the device half of SODA_c: (G, T, 4) fp64 max_score, precision, recall, F of every group at every tIoU.  Every
    distinct sentence is tokenized and encoded once (soda_encode: references through tables.encode, hypotheses as vocab
    ids, as meteor_pairs does); the groups go through ops.meteor_matrix and ops.soda_dp in chunks of about max_cells cells
    (soda_chunks), the score matrices staying on the device.  `tables`: a rewards.MeteorTables whose vocabulary holds
    every hypothesis word.  A video with more than ops.SODA_MAX_REFS references in a file, or a sentence past the METEOR
    limits, is a ValueError."""
    import torch
    from . import ops
    from .rewards import MeteorScorer
    T = len(tious)
    if not 1 <= T <= ops.SODA_MAX_T:
        raise ValueError(f"{T} tIoU thresholds; between 1 and {ops.SODA_MAX_T} are supported")
    out = np.zeros((len(groups), T, 4), dtype=np.float64)
    if not len(groups):
        return out
    enc = soda_encode(groups, tables, tokenizer)
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)          # noqa: E731
    vmap, vstem, syn_off, syn_ids = dev(tables.vmap), dev(tables.vstem), dev(tables.syn_off), dev(tables.syn_ids)
    hyp_d, ref_d, len_d = dev(enc["hyp"]), dev(enc["ref"]), dev(enc["ref_len"])
    stem_d = dev(enc["ref_stem"]) if vstem is not None else None
    tious_d = dev(np.asarray(tious, dtype=np.float64))
    for lo, hi, c in soda_chunks(groups, enc, max_cells):
        L, R = c["L"], c["R"]
        hyp_off, ref_off, cell_off = dev(c["hyp_off"]), dev(c["ref_off"]), dev(c["cell_off"])
        S = torch.empty(int(c["cell_off"][-1]), dtype=torch.float64, device=device)
        ops.meteor_matrix(hyp_d[:, :L], vmap, vstem, syn_off, syn_ids, ref_d[:, :R],
                          stem_d[:, :R] if stem_d is not None else None, len_d, dev(c["hyp_idx"]), dev(c["ref_idx"]), hyp_off,
                          ref_off, cell_off, MeteorScorer.alpha, MeteorScorer.beta, MeteorScorer.gamma_frag, S)
        out[lo:hi] = ops.soda_dp(dev(c["pred_seg"]), dev(c["ref_seg"]), hyp_off, ref_off, cell_off, S, tious_d).cpu().numpy()
    return out


def soda_per_video(by_video: Dict[str, List[int]], per_group: np.ndarray, T: int
                   ) -> Dict[str, List[Tuple[float, float, float]]]:
    """video id -> [(precision, recall, F) per tIoU]: the triple of the file with the highest F, the first such file in
    file order; (0, 0, 0) for a video without a group"""
    out = {}
    for vid, gs in by_video.items():
        triples = []
        for t in range(T):
            best = (0.0, 0.0, 0.0)
            for k, g in enumerate(gs):
                p, r, f = (float(x) for x in per_group[g, t, 1:4])
                if k == 0 or f > best[2]:
                    best = (p, r, f)
            triples.append(best)
        out[vid] = triples
    return out


def soda_means(per_video: Dict[str, List[Tuple[float, float, float]]], T: int) -> Dict[str, List[float]]:
    """the means over the videos (in their order) per tIoU: SODA_c is F, then precision and recall"""
    out = {m: [] for m in SODA_METRICS}
    for t in range(T):
        for m, c in zip(SODA_METRICS, (2, 0, 1)):
            total = 0.0
            for triples in per_video.values():
                total += triples[t][c]
            out[m].append(total / len(per_video))
    return out


# ---- paragraph evaluation
class ParagraphGroups(NamedTuple):
    """the host half of the paragraph evaluation: the ground-truth video ids (sorted), video id -> the predicted
    paragraph (token tuples, one per kept sentence, in time order; [] when nothing is left), and per ground-truth file
    video id -> the reference paragraph, for the videos that have one in that file"""
    vids: List[str]
    predicted: Dict[str, List[Tuple[str, ...]]]
    references: List[Dict[str, List[Tuple[str, ...]]]]


def _flat(sentences: Sequence[Sequence[str]]) -> Tuple[str, ...]:
    return tuple(w for s in sentences for w in s)


def paragraph_groups(ground_truths: Sequence[dict], prediction: Dict[str, list],
                     tokenizer: Callable[[str], Sequence[str]] = tokenize, top: Optional[int] = None,
                     sort_references: bool = False) -> ParagraphGroups:
    """The paragraphs of a job (see ParagraphGroups) for every ground-truth video id; videos that only the prediction holds
    are left out.  `prediction` is already cut to max_proposals per video.
    Predicted paragraph: the `top` first positions of by_proposal_score (None: all), ordered by list index and then
    stably by (start, end).  Reference paragraph of a file: its sentences of the video in file order, by (start, end) with
    sort_references.  Every sentence passes remove_nonascii and the tokenizer; a sentence without a token is dropped, and
    a file gives no reference paragraph for a video it lacks or of which no token is left.
    A predicted paragraph past ops.REWARDS_MAX_L tokens or a reference paragraph past ops.REWARDS_MAX_R is a ValueError
    naming the video (and the file): the scorers' limits, checked here, before anything goes to the device."""
    from . import ops
    clean = lambda sents: [t for t in (tuple(tokenizer(remove_nonascii(s))) for s in sents) if t]           # noqa: E731
    vids = ground_truth_video_ids(ground_truths)
    predicted: Dict[str, List[Tuple[str, ...]]] = {}
    references: List[Dict[str, List[Tuple[str, ...]]]] = [{} for _ in ground_truths]
    for vid in vids:
        preds = prediction.get(vid, ())
        kept = sorted(by_proposal_score(preds)[:top])
        order = _by_time([preds[k]["timestamp"] for k in kept])
        para = predicted[vid] = clean([preds[kept[o]]["sentence"] for o in order])
        n = sum(map(len, para))
        if n > ops.REWARDS_MAX_L:
            raise ValueError(f"video {vid}: a predicted paragraph of {n} tokens; at most {ops.REWARDS_MAX_L} are supported "
                             f"(paragraph_top=k reads only the k best-scored proposals)")
        for f, gt in enumerate(ground_truths):
            if vid not in gt:
                continue
            sents = gt[vid]["sentences"]
            rorder = _by_time(gt[vid]["timestamps"]) if sort_references else range(len(sents))
            ref = clean([sents[k] for k in rorder])
            n = sum(map(len, ref))
            if n > ops.REWARDS_MAX_R:
                raise ValueError(f"video {vid}: a reference paragraph of {n} tokens in ground-truth file {f}; at most "
                                 f"{ops.REWARDS_MAX_R} are supported (paragraph_top does not shorten a reference)")
            if ref:
                references[f][vid] = ref
    return ParagraphGroups(vids, predicted, references)


def paragraph_stats(paragraphs: Sequence[Sequence[Sequence[str]]], device="cuda") -> np.ndarray:
    """(G, 4, 5) int32 numpy: total, distinct, in_repeated, cross, max_count of the n-grams, n = 1..4, of every paragraph
    (a sequence of sentences, each a sequence of tokens; an empty sentence or paragraph is allowed): one ops.ngram_stats
    launch over word ids of a rewards.StringTable of its own.  Predictions and references alike."""
    import torch
    from . import ops
    from .rewards import StringTable
    G = len(paragraphs)
    if not G:
        return np.zeros((0, 4, ops.NGRAM_STATS_INTS), dtype=np.int32)
    table = StringTable()
    tok, sent_off, para_off = [], [0], [0]
    for g, para in enumerate(paragraphs):
        start = len(tok)
        for sent in para:
            tok.extend(table.add(w) for w in sent)
            sent_off.append(len(tok))
        if len(tok) - start > ops.PARAGRAPH_MAX_TOKENS:
            raise ValueError(f"paragraph {g} holds {len(tok) - start} tokens; at most {ops.PARAGRAPH_MAX_TOKENS} are supported")
        para_off.append(len(sent_off) - 1)
    dev = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int32)).to(device)                              # noqa: E731
    return ops.ngram_stats(dev(tok), dev(sent_off), dev(para_off)).cpu().numpy()


def paragraph_scores(groups: ParagraphGroups, device, tables) -> Dict[str, float]:
    """Para_Bleu_1..4, Para_METEOR, Para_ROUGE_L, Para_CIDEr of a job: group f holds the pairs (predicted paragraph,
    file f's reference paragraph) of the videos with a reference paragraph in f, in video order; all groups go through one
    score_pairs call, so BLEU is corpus-level over a file, CIDEr's document frequencies are the file's reference
    paragraphs, ROUGE-L and METEOR are means over the file's videos.  A video whose predicted paragraph is empty enters
    as an empty hypothesis.  Each figure is the mean over the files with at least one pair, in file order; 0.0 without a
    pair.  `tables`: a rewards.MeteorTables whose vocabulary holds every predicted word."""
    hyps, refs, off = [], [], [0]
    for refs_of in groups.references:
        for vid in groups.vids:
            if vid in refs_of:
                hyps.append(_flat(groups.predicted[vid]))
                refs.append(_flat(refs_of[vid]))
        off.append(len(hyps))
    out = {f"Para_{m}": 0.0 for m in METRICS}
    if not hyps:
        return out
    per_file = score_pairs(hyps, refs, off, device, tables)
    mine = [f for f in range(len(off) - 1) if off[f + 1] > off[f]]
    for m in METRICS:
        out[f"Para_{m}"] = sum(float(per_file[m][f]) for f in mine) / len(mine)
    return out


def paragraph_means(stats: np.ndarray) -> Dict[str, float]:
    """Para_RE_4, Para_XRE_4, Para_Div_1, Para_Div_2 of the (V, 4, 5) integers of the videos' predicted paragraphs: per
    video RE_n = (total - distinct) / total, XRE_n = cross / total, Div_n = distinct / total; each key is the mean over
    the videos whose total at that n is > 0, in video order, 0.0 when there is none"""
    out = {}
    for key, n, value in (("Para_RE_4", 4, lambda r: (r[0] - r[1]) / r[0]), ("Para_XRE_4", 4, lambda r: r[3] / r[0]),
                          ("Para_Div_1", 1, lambda r: r[1] / r[0]), ("Para_Div_2", 2, lambda r: r[1] / r[0])):
        vals = [value([int(x) for x in row]) for row in stats[:, n - 1] if row[0] > 0]
        out[key] = sum(vals) / len(vals) if vals else 0.0
    return out


# ---- bootstrap intervals and paired run comparison
PARAGRAPH_STAT_KEYS = ("Para_RE_4", "Para_XRE_4", "Para_Div_1", "Para_Div_2")
_BOOT_CHUNK = 1 << 22                         # count cells (resamples x videos) per pass of bootstrap_ratios_host
_U64 = np.uint64
BOOTSTRAP_LIMITS = (16384, 4096, 1 << 20)     # videos, columns, resamples: ops.BOOTSTRAP_MAX_N / _M / _R


def _hash_u32(seed: int, idx: np.ndarray) -> np.ndarray:
    """csrc/common.h's hash_u32 over a uint64 array (the arithmetic wraps modulo 2^64, as the device's)"""
    z = idx * _U64(0x9E3779B97F4A7C15) + _U64(seed)
    z = (z ^ (z >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> _U64(27))) * _U64(0x94D049BB133111EB)
    z = z ^ (z >> _U64(31))
    return z >> _U64(32)


def bootstrap_counts(N: int, rows: Sequence[int], seed: int) -> np.ndarray:
    """(len(rows), N) int64: the counts c_i of the rows `rows` of the bootstrap's definition -- all ones for row 0, and for
    row r >= 1 the number of the N draws i = (hash_u32(seed, (r << 32) | j) * N) >> 32, j = 0 .. N - 1, that hit video i"""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1)
    idx = (rows[:, None] << _U64(32)) | np.arange(N, dtype=np.uint64)[None, :]
    drawn = ((_hash_u32(seed, idx) * _U64(N)) >> _U64(32)).astype(np.int64)
    flat = drawn + (np.arange(len(rows), dtype=np.int64) * N)[:, None]
    counts = np.bincount(flat.reshape(-1), minlength=len(rows) * N).reshape(len(rows), N)
    counts[rows == 0] = 1
    return counts


def _check_bootstrap_inputs(values, weights, resamples, seed, limits):
    if values.ndim != 2 or (weights is not None and weights.shape != values.shape):
        raise ValueError("bootstrap: values (M, N) and weights (M, N) or None expected")
    M, N = values.shape
    max_n, max_m, max_r = limits
    if not (1 <= N <= max_n and 1 <= M <= max_m and 1 <= resamples <= max_r):
        raise ValueError(f"bootstrap: {N} videos, {M} columns, {resamples} resamples; at most {max_n}, {max_m}, {max_r} "
                         "and at least one of each are supported")
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"bootstrap: seed {seed} is no uint64")


def bootstrap_ratios_host(values, weights, resamples: int, seed: int = 0) -> np.ndarray:
    """ops.bootstrap_ratios in numpy, bit for bit (B1-B4 of bmhrl_bootstrap_ratios, include/bmhrl_hip.h): values (M, N)
    fp64, weights (M, N) fp64 or None -> stats (resamples + 1, M) fp64.  The hash is uint64 array arithmetic; the 64 lane
    sums run over the ceil(N / 64) strides in ascending order, vectorised over resamples, columns and lanes, product and sum
    as two numpy operations (two roundings); the butterfly adds the two halves of the lane axis six times.  Non-finite
    inputs are a ValueError.  The route of evaluate.bootstrap / compare when the evaluator's device is the CPU."""
    values = np.ascontiguousarray(values, dtype=np.float64)
    weights = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    R, seed = int(resamples), int(seed)
    _check_bootstrap_inputs(values, weights, R, seed, BOOTSTRAP_LIMITS)
    if not np.isfinite(values).all() or (weights is not None and not np.isfinite(weights).all()):
        raise ValueError("bootstrap: non-finite values or weights")
    M, N = values.shape
    stats = np.empty((R + 1, M), dtype=np.float64)
    strides = -(-N // 64)

    def padded(a):                              # (M, strides, 64): lane t of stride k is video 64 k + t
        out = np.zeros((M, strides * 64), dtype=np.float64)
        out[:, :N] = a
        return out.reshape(M, strides, 64)

    def lane_sums(c, a):                        # c (rows, strides, 64) fp64, a (M, strides, 64) -> S (rows, M), B2 and B3
        p = np.zeros((c.shape[0], M, 64), dtype=np.float64)
        last = N - (strides - 1) * 64           # the lanes of the last stride that hold a video
        for k in range(strides):
            n = 64 if k < strides - 1 else last
            p[:, :, :n] = p[:, :, :n] + (c[:, None, k, :n] * a[None, :, k, :n])
        for s in (32, 16, 8, 4, 2, 1):
            p = p + p.reshape(-1, M, 64 // (2 * s), 2, s)[:, :, :, ::-1, :].reshape(-1, M, 64)
        return p[:, :, 0]

    x = padded(values)
    w = None if weights is None else padded(weights)
    step = max(1, _BOOT_CHUNK // (max(M, 1) * strides * 64))
    for lo in range(0, R + 1, step):
        rows = np.arange(lo, min(lo + step, R + 1))
        c = np.zeros((len(rows), strides * 64), dtype=np.float64)
        c[:, :N] = bootstrap_counts(N, rows, seed)
        c = c.reshape(len(rows), strides, 64)
        num = lane_sums(c, x)
        if w is None:
            stats[rows] = num / np.float64(N)
        else:
            den = lane_sums(c, w)
            zero = den == 0.0
            stats[rows] = np.where(zero, 0.0, num / np.where(zero, 1.0, den))
    return stats


def soda_values(per_video: Dict[str, List[Tuple[float, float, float]]], T: int):
    """(video ids, {metric: [(N,) fp64 per tIoU]}) of .soda_per_video: the values soda_means takes its means of, in its
    order of the videos"""
    vids = list(per_video)
    return vids, {m: [np.array([per_video[v][t][c] for v in vids], dtype=np.float64) for t in range(T)]
                  for m, c in zip(SODA_METRICS, (2, 0, 1))}


def paragraph_values(per_video: Dict[str, dict], T: int):
    """(video ids, {key: [(2, N) fp64 per tIoU]}) of .paragraph_per_video for PARAGRAPH_STAT_KEYS: row 0 a video's ratio
    (paragraph_means' expressions) or 0.0, row 1 its weight, 1.0 where the video's total at the key's n is > 0, else 0.0.
    The mean of the weighted videos is paragraph_means' figure; the T entries of a key are one array."""
    vids = list(per_video)
    out = {}
    for key, n, value in (("Para_RE_4", 4, lambda r: (r[0] - r[1]) / r[0]), ("Para_XRE_4", 4, lambda r: r[3] / r[0]),
                          ("Para_Div_1", 1, lambda r: r[1] / r[0]), ("Para_Div_2", 2, lambda r: r[1] / r[0])):
        col = np.zeros((2, len(vids)), dtype=np.float64)
        for v, vid in enumerate(vids):
            row = [int(x) for x in per_video[vid]["stats"][n - 1]]
            if row[0] > 0:
                col[0, v], col[1, v] = value(row), 1.0
        out[key] = [col] * T
    return vids, out


def summarize(stats, alpha: float = 0.05):
    """(lo, hi, se), each (M,): the percentile interval and the standard error of the resampled rows 1 .. R of stats
    (R + 1, M) -- a torch tensor (sorted by torch.sort where it lives) or a numpy array (np.sort).  Per column over the R
    values sorted ascending: lo = sorted[clamp(int(floor(alpha / 2 * R)))], hi = sorted[clamp(int(ceil((1 - alpha / 2) * R))
    - 1)], the indices clamped to [0, R - 1]; se = their unbiased standard deviation (0.0 for R = 1).  Row 0, the observed
    statistic, is not read.  Returns what it was given: tensors for a tensor, arrays for an array."""
    import math
    if not 0.0 < alpha < 1.0:
        raise ValueError(f"alpha {alpha!r}: a number in (0, 1) expected")
    R = stats.shape[0] - 1
    if stats.ndim != 2 or R < 1:
        raise ValueError("summarize: stats (R + 1, M) with R >= 1 expected")
    clamp = lambda k: min(max(k, 0), R - 1)                                                                 # noqa: E731
    i_lo, i_hi = clamp(int(math.floor(alpha / 2 * R))), clamp(int(math.ceil((1 - alpha / 2) * R)) - 1)
    if isinstance(stats, np.ndarray):
        s = np.sort(stats[1:], axis=0)
        se = s.std(axis=0, ddof=1) if R > 1 else np.zeros(stats.shape[1], dtype=stats.dtype)
        return s[i_lo].copy(), s[i_hi].copy(), se
    import torch
    s = torch.sort(stats[1:], dim=0).values
    se = s.std(dim=0, unbiased=True) if R > 1 else torch.zeros_like(s[0])
    return s[i_lo].clone(), s[i_hi].clone(), se


def _family_columns(evaluator, family: str):
    """(video ids, [(metric, tIoU index)] per column, values (M, N), weights (M, N) or None) of one family of
    evaluator.per_video; the paragraph family carries weights, and its tIoU entries are one column each all the same"""
    vids, metrics = evaluator.per_video[family]
    names, cols, wts = [], [], []
    for m, per_tiou in metrics.items():
        for t, col in enumerate(per_tiou):
            names.append((m, t))
            if family == "paragraph":
                cols.append(col[0])
                wts.append(col[1])
            else:
                cols.append(col)
    values = np.asarray(cols, dtype=np.float64).reshape(len(cols), len(vids))
    weights = np.asarray(wts, dtype=np.float64).reshape(len(cols), len(vids)) if family == "paragraph" else None
    return vids, names, values, weights


def _evaluated(evaluator, what):
    per_video = getattr(evaluator, "per_video", None)
    if not per_video:
        raise ValueError(f"{what}: an evaluator after .evaluate() (and not only_proposals) expected")
    return per_video


def _stats_on(values, weights, resamples, seed, device):
    """the (R + 1, M) statistics where `device` says: a device tensor from the launch, or the host route's array"""
    import torch
    if torch.device(device).type == "cpu":
        return bootstrap_ratios_host(values, weights, resamples, seed)
    from . import ops
    for a in (values, weights):
        if a is not None and not np.isfinite(a).all():
            raise ValueError("bootstrap: non-finite values or weights")
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)             # noqa: E731
    return ops.bootstrap_ratios(dev(values), dev(weights), int(resamples), int(seed))


def _host(x) -> np.ndarray:
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def bootstrap(evaluator, resamples: int = 10000, seed: int = 0, alpha: float = 0.05) -> Dict[str, List[dict]]:
    """{metric: [dict(value, lo, hi, se) per tIoU]}: the paired bootstrap over videos (Koehn 2004) of every figure of an
    evaluated DenseCaptionEvaluator that is a mean over videos -- the seven METRICS, the SODA_METRICS with soda=True,
    Para_RE_4 / Para_XRE_4 / Para_Div_1 / Para_Div_2 with paragraph=True.  One bootstrap_ratios call per family of
    evaluator.per_video (their video lists can differ), on evaluator.device (the CPU runs bootstrap_ratios_host: the same
    bits), then summarize.  `value` is evaluator.scores' entry, not row 0 of the call; lo / hi are the 1 - alpha percentile
    interval of the resampled means, se their standard deviation.

    Out of scope: Para_Bleu_* .. Para_CIDEr (corpus-level per ground-truth file), Precision / Recall, AUC and AR@AN (not
    means over videos).  The corpus BLEU within a video stays as it is: the video is the resampling unit.  No
    multiple-comparison correction.  The interval says how much the sample of videos moves a figure; it says nothing about
    how close this package's stand-in METEOR is to published numbers."""
    out: Dict[str, List[dict]] = {}
    for family in _evaluated(evaluator, "bootstrap"):
        vids, names, values, weights = _family_columns(evaluator, family)
        if not names or not len(vids):
            continue
        lo, hi, se = (_host(a) for a in summarize(_stats_on(values, weights, resamples, seed, evaluator.device), alpha))
        for c, (m, t) in enumerate(names):
            out.setdefault(m, []).append({"value": float(evaluator.scores[m][t]), "lo": float(lo[c]), "hi": float(hi[c]),
                                          "se": float(se[c])})
    return out


def compare(evaluator_a, evaluator_b, resamples: int = 10000, seed: int = 0, alpha: float = 0.05) -> Dict[str, List[dict]]:
    """{metric: [dict(a, b, delta, lo, hi, wins, losses) per tIoU]}: two evaluated runs over the same videos under one
    resample.  Per family the columns of A and of B go into ONE (2 M, N) bootstrap_ratios call (on evaluator_a.device), so
    both runs see the same counts; delta_r = stat_A[r] - stat_B[r]; a / b are the two .scores entries and delta = a - b;
    lo / hi the percentile interval of delta over the resamples (summarize); wins the share of resamples with delta > 0,
    losses the share with delta < 0.  The families, metrics and tIoUs of the two evaluators must be the same and their
    video-id lists equal: otherwise a ValueError, naming the first differing id.  bootstrap's out-of-scope list applies:
    only means over videos, no multiple-comparison correction, nothing about published figures."""
    pa, pb = _evaluated(evaluator_a, "compare"), _evaluated(evaluator_b, "compare")
    if list(pa) != list(pb):
        raise ValueError(f"compare: the evaluators hold different families: {list(pa)} and {list(pb)}")
    out: Dict[str, List[dict]] = {}
    for family in pa:
        vids_a, names_a, values_a, weights_a = _family_columns(evaluator_a, family)
        vids_b, names_b, values_b, weights_b = _family_columns(evaluator_b, family)
        if list(vids_a) != list(vids_b):
            k = next((k for k, (u, v) in enumerate(zip(vids_a, vids_b)) if u != v), min(len(vids_a), len(vids_b)))
            first = vids_a[k] if k < len(vids_a) else None
            other = vids_b[k] if k < len(vids_b) else None
            raise ValueError(f"compare: the {family} video lists differ at position {k}: {first!r} and {other!r}")
        if names_a != names_b:
            raise ValueError(f"compare: the evaluators hold different {family} metrics or tIoUs")
        if not names_a or not len(vids_a):
            continue
        M = len(names_a)
        values = np.concatenate([values_a, values_b])
        weights = None if weights_a is None else np.concatenate([weights_a, weights_b])
        stats = _stats_on(values, weights, resamples, seed, evaluator_a.device)
        delta = stats[:, :M] - stats[:, M:]
        lo, hi, _ = (_host(a) for a in summarize(delta, alpha))
        d = _host(delta[1:])
        wins, losses = (d > 0).sum(axis=0) / float(d.shape[0]), (d < 0).sum(axis=0) / float(d.shape[0])
        for c, (m, t) in enumerate(names_a):
            a, b = float(evaluator_a.scores[m][t]), float(evaluator_b.scores[m][t])
            out.setdefault(m, []).append({"a": a, "b": b, "delta": a - b, "lo": float(lo[c]), "hi": float(hi[c]),
                                          "wins": float(wins[c]), "losses": float(losses[c])})
    return out
