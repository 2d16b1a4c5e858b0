"""Restatements the proposal kernels (bmhrl_amd/csrc/proposal.hip) are tested against.

assign / head: plain torch in float64, so autograd gives the gradient.  The anchor choice of `assign` is the one part kept in
fp32: it is defined as the reference's tiou_vectorized arithmetic on fp32 tensors (an argmax has no tolerance), with ties to
the smaller index.
select: plain Python on numpy float32 scalars -- the reference's postprocess_preds + non_max_suppresion with the tie rule
"equal confidences: the smaller row first", which the reference's argsort leaves open.
"""
import json
import os

import numpy as np
import torch

from bmhrl_amd.proposal_utils import tiou_vectorized

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden():
    """tests/golden/proposals.json + proposals.npz (tests/golden/make_proposal_golden.py) put back together: "inputs"[N] fp32
    (3, N, 3), and per case "postprocessed" fp32 (3, k_eff, 3), "nms" (one fp32 array per video, when the case has a
    threshold) and "results", the dictionary the reference's AnetPredictions held (as json reads it back: lists)"""
    with open(os.path.join(GOLDEN, "proposals.json")) as f:
        g = json.load(f)
    z = np.load(os.path.join(GOLDEN, "proposals.npz"))
    g["inputs"] = {int(k[3:]): z[k] for k in z.files if k.startswith("in_")}
    for case in g["cases"]:
        name = f"{case['N']}_{case['k']}_{case['nms_tiou']}"
        case["postprocessed"] = z[f"post_{case['N']}_{case['k']}"]
        if case["nms_tiou"] is not None:
            case["nms"] = np.split(z[f"nms_{name}"], np.cumsum(case["nms_counts"])[:-1])
        rows = iter(z[f"res_{name}"].tolist())
        case["results"] = {vid: [{"sentence": "", "proposal_score": [score], "timestamp": [start, end]}
                                 for start, end, score in (next(rows) for _ in range(n))] for vid, n in case["results_videos"]}
    return g


def assign(targets, anchors, cell_sec, B, S):
    """targets (N, 4) fp32, anchors (A) fp32 (CPU).  Returns owner (B, A, S) int64, tx, tw (N) float64, counts [n_obj,
    n_noobj], best (N) int64."""
    N, A = targets.shape[0], anchors.shape[0]
    owner = torch.full((B, A, S), -1, dtype=torch.int64)
    cs32 = torch.tensor(cell_sec, dtype=torch.float32)
    w32 = targets[:, 2] / cs32
    a32 = anchors / cs32
    best = torch.zeros(N, dtype=torch.int64)
    if N:
        tious = tiou_vectorized(a32.view(A, 1), w32.view(N, 1), without_center_coords=True)     # (A, N) fp32
        for r in range(N):
            col = tious[:, r]
            best[r] = int(torch.nonzero(col == col.max())[0])                                   # the smallest index of the maximum
    # the quotients are the kernel's fp32 ones (IEEE division: the same bits); what follows them is float64
    g = (targets[:, 1] / cs32).double()
    w = w32.double()
    fl = torch.floor(g)
    tx = g - fl
    tw = torch.log(w / a32.double()[best] + 1e-16) if N else torch.zeros(0, dtype=torch.float64)
    for r in range(N):
        b, cell = int(targets[r, 0]), int(fl[r])
        if 0 <= b < B and 0 <= cell < S:
            owner[b, int(best[r]), cell] = r                # sequential assignment: the largest row stays
    n_obj = int((owner >= 0).sum())
    return owner, tx, tw, [n_obj, B * A * S - n_obj], best


def _softplus(z):
    """log(1 + exp(z)), stable, and with the derivative sigmoid(z) at every z (a max / abs form has a kink at exactly 0)"""
    return -torch.nn.functional.logsigmoid(-z)


def _nonempty(assigned):
    """(owner, tx, tw) with one unused entry in tx / tw when there is no target, so that tx[owner.clamp(min=0)] indexes"""
    owner, tx, tw = assigned
    return (owner, tx, tw) if tx.numel() else (owner, torch.zeros(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64))


def head(x, anchors, cell_sec, assigned=None, obj_coeff=1.0, noobj_coeff=100.0):
    """x (B, S, 3A) float64 (requires_grad for the gradient), anchors (A).  Returns pred (B, A*S, 3) float64 and, with
    assigned = (owner (B, A, S) int64, tx, tw float64), sums (5) = [loss_x, loss_w, loss_obj, loss_noobj, total] and mags
    (5): the sums of the absolute values of what each was added up from, divided like the sum itself."""
    B, S, A3 = x.shape
    A = A3 // 3
    v = x.view(B, S, A, 3).permute(0, 2, 1, 3)              # (B, A, S, 3)
    c, l, o = v[..., 0], v[..., 1], v[..., 2]
    sc = torch.sigmoid(c)
    pos = torch.arange(S, dtype=x.dtype).view(1, 1, S)
    an = anchors.to(x.dtype).view(1, A, 1)
    pred = torch.stack([(sc + pos) * cell_sec, an * torch.exp(l), torch.sigmoid(o)], dim=-1).reshape(B, A * S, 3)
    if assigned is None:
        return pred
    owner, tx, tw = _nonempty(assigned)
    own = owner >= 0
    idx = owner.clamp(min=0)
    n_obj, n_noobj = int(own.sum()), int((~own).sum())
    zero = x.sum() * 0

    def mean(t, mask, n):
        return (t * mask).sum() / n if n else zero

    ex, ew = sc - tx.to(x.dtype)[idx], l - tw.to(x.dtype)[idx]
    lx, lw = mean(ex * ex, own, n_obj), mean(ew * ew, own, n_obj)
    lo, ln = mean(_softplus(-o), own, n_obj), mean(_softplus(o), ~own, n_noobj)
    total = lx + lw + obj_coeff * lo + noobj_coeff * ln
    sums = torch.stack([lx, lw, lo, ln, total])
    mags = torch.stack([lx, lw, lo, ln, lx + lw + abs(obj_coeff) * lo + abs(noobj_coeff) * ln]).detach()   # (all terms >= 0)
    return pred, sums, mags


def dx_magnitude(x, anchors, assigned, obj_coeff=1.0, noobj_coeff=100.0):
    """per element of d total / d x: the sum of the absolute values of the products it is a difference of (float64) -- what an
    fp32 evaluation's error scales with where sigmoid(c) - tx or l - tw cancels"""
    B, S, A3 = x.shape
    A = A3 // 3
    owner, tx, tw = _nonempty(assigned)
    own = owner >= 0
    idx = owner.clamp(min=0)
    n_obj, n_noobj = int(own.sum()), int((~own).sum())
    v = x.detach().view(B, S, A, 3).permute(0, 2, 1, 3)
    c, l, o = v[..., 0], v[..., 1], v[..., 2]
    sc = torch.sigmoid(c)
    inv_obj = 1.0 / n_obj if n_obj else 0.0
    inv_noobj = 1.0 / n_noobj if n_noobj else 0.0
    m_c = 2 * (sc.abs() + tx[idx].abs()) * sc * (1 - sc) * inv_obj * own
    m_l = 2 * (l.abs() + tw[idx].abs()) * inv_obj * own
    m_o = torch.where(own, obj_coeff * torch.sigmoid(-o) * inv_obj, noobj_coeff * torch.sigmoid(o) * inv_noobj)
    return torch.stack([m_c, m_l, m_o], dim=-1).permute(0, 2, 1, 3).reshape(B, S, A3)


def select(pred, durations, k, nms_tiou=None):
    """pred (B, N, 3) float32 numpy, durations (B).  Returns props (B, k, 3) float32 and count (B) int32."""
    pred = np.asarray(pred, dtype=np.float32)
    B, N, _ = pred.shape
    props = np.zeros((B, k, 3), dtype=np.float32)
    count = np.zeros(B, dtype=np.int32)
    f = np.float32
    for b in range(B):
        dur = f(durations[b])
        order = np.lexsort((np.arange(N), -pred[b, :, 2]))[:k]          # confidence descending, then the smaller row
        segs = []
        for j in order:
            centre, length, conf = pred[b, j]
            start, end = centre - length / f(2), centre + length / f(2)
            start = min(max(start, f(0)), dur)
            end = min(end, dur)
            segs.append((start, end, conf))
        alive = [True] * len(segs)
        if nms_tiou is not None and nms_tiou >= 0:
            thr = f(nms_tiou)
            for i in range(len(segs)):
                if not alive[i]:
                    continue
                s1, e1, _ = segs[i]
                for j in range(i + 1, len(segs)):
                    if not alive[j]:
                        continue
                    s2, e2, _ = segs[j]
                    inter = max(min(e1, e2) - max(s1, s2), f(0))
                    union = (e1 - s1) + (e2 - s2) - inter
                    union = min(max(e1, e2) - min(s1, s2), union)
                    if not (inter / (union + f(1e-8)) < thr):
                        alive[j] = False
        kept = [s for s, a in zip(segs, alive) if a]
        count[b] = len(kept)
        for j, s in enumerate(kept):
            props[b, j] = s
    return props, count
