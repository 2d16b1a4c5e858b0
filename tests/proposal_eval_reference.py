"""Plain-Python restatement of the proposal metrics: lists, floats and evaluate.tiou's arithmetic
written out.  The hit / first-rank tables and the ordered pair list of csrc/proposal_eval.hip, detection precision / recall
and AR@AN / AUC as bmhrl_amd.evaluate defines them.  Nothing here imports the package."""


def tiou(pred, ref):
    """evaluate.tiou(pred, ref), term for term"""
    start_i, end_i = pred[0], pred[1]
    start, end = ref[0], ref[1]
    intersection = max(0, min(end, end_i) - max(start, start_i))
    union = min(max(end, end_i) - min(start, start_i), end - start + end_i - start_i)
    return float(intersection) / (union + 1e-8)


def passes(iou, threshold, strict):
    return iou > threshold if strict else iou >= threshold


def iou_cells(pred_seg, ref_seg, groups):
    """per group (a row (p0, P, r0, R)) the P lists of R cell values"""
    return [[[tiou(pred_seg[p0 + i], ref_seg[r0 + j]) for j in range(R)] for i in range(P)] for p0, P, r0, R in groups]


def hit_tables(pred_seg, ref_seg, groups, tious, strict, cells=None):
    """(pred_hits, ref_first): lists of T rows over the running sums of the groups' P / R.  pred_hits: the number of the
    group's references the prediction passes; ref_first: the smallest in-group index of a prediction that passes the
    reference, P when there is none.  cells: iou_cells of the same arguments, when the caller has them already."""
    cells = iou_cells(pred_seg, ref_seg, groups) if cells is None else cells
    pred_hits, ref_first = [[] for _ in tious], [[] for _ in tious]
    for (p0, P, r0, R), cell in zip(groups, cells):
        for t, thr in enumerate(tious):
            for i in range(P):
                pred_hits[t].append(sum(1 for j in range(R) if passes(cell[i][j], thr, strict)))
            for j in range(R):
                first = P
                for i in range(P):
                    if passes(cell[i][j], thr, strict):
                        first = i
                        break
                ref_first[t].append(first)
    return pred_hits, ref_first


def pair_list(pred_seg, ref_seg, groups, threshold, cells=None):
    """[(slot, global reference row or -1)]: per group and prediction the references with tIoU >= threshold, ascending, or
    one -1; the slots count the predictions of the groups in order"""
    cells = iou_cells(pred_seg, ref_seg, groups) if cells is None else cells
    out, slot = [], 0
    for (p0, P, r0, R), cell in zip(groups, cells):
        for i in range(P):
            rows = [r0 + j for j in range(R) if cell[i][j] >= threshold]
            out.extend((slot, r) for r in (rows or [-1]))
            slot += 1
    return out


def video_ids(ground_truths):
    return sorted(set().union(*[set(gt) for gt in ground_truths]))


def pairs_of_job(ground_truths, prediction, threshold):
    """video id -> [(prediction index in the video's list, (file, caption index) or None)] in the order prediction, file,
    caption"""
    out = {}
    for vid in video_ids(ground_truths):
        pairs = out[vid] = []
        for pi, pred in enumerate(prediction.get(vid, ())):
            found = [(f, idx) for f, gt in enumerate(ground_truths) if vid in gt
                     for idx, stamp in enumerate(gt[vid]["timestamps"]) if tiou(pred["timestamp"], stamp) >= threshold]
            pairs.extend((pi, r) for r in (found or [None]))
    return out


def detection(ground_truths, prediction, threshold):
    """(precision, recall): per video and file the share of predictions / references with some tIoU > threshold, the best
    over the files, the mean over the videos; a video without predictions counts precision 0"""
    precision, recall = [], []
    for vid in video_ids(ground_truths):
        preds = prediction.get(vid, ())
        best_p = best_r = 0.0
        for gt in ground_truths:
            if vid not in gt:
                continue
            stamps = gt[vid]["timestamps"]
            segs = [p["timestamp"] for p in preds]
            hits, first = hit_tables(segs, stamps, [(0, len(segs), 0, len(stamps))], [threshold], True)
            if len(preds):
                best_p = max(best_p, float(sum(1 for h in hits[0] if h > 0)) / len(preds))
            best_r = max(best_r, float(sum(1 for f in first[0] if f < len(segs))) / len(stamps))
        precision.append(best_p)
        recall.append(best_r)
    return sum(precision) / len(precision), sum(recall) / len(recall)


def score_of(pred):
    score = pred.get("proposal_score", 0.0)
    if isinstance(score, (list, tuple)):
        score = score[0]
    return float(score)


def score_order(preds):
    """positions by score descending; ties keep list order"""
    order = list(range(len(preds)))
    order.sort(key=lambda k: -score_of(preds[k]))          # list.sort is stable
    return order


def trapezoid(y, x):
    total = 0.0
    for k in range(len(x) - 1):
        total += (x[k + 1] - x[k]) * (y[k + 1] + y[k]) / 2.0
    return total


def recall_of_file(gt, prediction, tious, max_avg_nr_proposals, points):
    """(recall[t][k], x[k], auc[t]) of one ground-truth file"""
    vids = sorted(gt)
    V = len(vids)
    total = sum(len(prediction.get(vid, ())) for vid in vids)
    n_refs = sum(len(gt[vid]["timestamps"]) for vid in vids)
    recall = [[0.0] * points for _ in tious]
    if total == 0 or n_refs == 0:
        return recall, [0.0] * points, [0.0] * len(tious)
    ratio = max_avg_nr_proposals * float(V) / total
    pcn = [(k / float(points)) * ratio for k in range(1, points + 1)]
    matched = [[0] * points for _ in tious]
    for vid in vids:
        preds = prediction.get(vid, ())
        segs = [preds[k]["timestamp"] for k in score_order(preds)]
        P = len(segs)
        stamps = gt[vid]["timestamps"]
        _, first = hit_tables(segs, stamps, [(0, P, 0, len(stamps))], tious, False)
        for k in range(points):
            nr = int(min(P * pcn[k], P))
            for t in range(len(tious)):
                matched[t][k] += sum(1 for f in first[t] if f < nr)
    for t in range(len(tious)):
        recall[t] = [m / float(n_refs) for m in matched[t]]
    x = [p * (float(total) / V) for p in pcn]
    auc = [100.0 * trapezoid(recall[t], x) / x[-1] for t in range(len(tious))]
    return recall, x, auc


def proposal_recall(ground_truths, prediction, tious, max_avg_nr_proposals=100, points=100):
    """{"AUC": [T], "AR@AN": [T], "recall_curve": T lists of points, "proposals_per_video": points}: the plain mean over the
    ground-truth files of recall_of_file's curves and figures"""
    parts = [recall_of_file(gt, prediction, tious, max_avg_nr_proposals, points) for gt in ground_truths]
    n = float(len(parts))
    T = len(tious)

    def mean(rows):                                         # element-wise, the files added in order
        acc = list(rows[0])
        for row in rows[1:]:
            acc = [a + b for a, b in zip(acc, row)]
        return [a / n for a in acc]
    return {"AUC": [sum(p[2][t] for p in parts) / n for t in range(T)],
            "AR@AN": [sum(p[0][t][-1] for p in parts) / n for t in range(T)],
            "recall_curve": [mean([p[0][t] for p in parts]) for t in range(T)],
            "proposals_per_video": mean([p[1] for p in parts])}
