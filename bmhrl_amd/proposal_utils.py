"""Post-processing of the proposal generator's predictions, the counterpart of the reference's utilities/proposal_utils.py:
tIoU, top-k, corner coordinates, trimming, greedy NMS, the ActivityNet submission dictionary and anchor lengths.

The tensor functions reproduce the reference's results (tests/golden/proposals.json / .npz record them) for callers that use them
piecemeal; they are plain torch and run wherever their input lives.  `AnetPredictions.add_new_predictions` does the whole
chain for a batch: for device input in ONE call of ops.proposal_select (csrc/proposal.hip: a fixed number of launches and no
host read before the single `.tolist()`), for host input through the piecewise functions.  Where the reference's `argsort`
leaves the order of equal confidences open, both routes here put the smaller row first.

Beyond the reference: Soft-NMS (`soft_nms`, cfg.nms_method "linear" / "gaussian") and a candidate pool larger than
max_prop_per_vid (cfg.nms_candidates); `soft_nms_settings` reads the optional cfg fields, `soft_select_rows` is the route
(ops.proposal_select_soft for device input), and a cfg without them takes the calls above unchanged.  Event-chain
selection (`event_chain`, cfg.chain_max_events and the other fields of `chain_settings`): of the rows any of those routes
selects, the time-ordered chain of at most L low-overlap events of largest total confidence, found exactly (on the device
by ops.proposal_chain, fed by the select kernels' output); `chain_predictions` applies it to a submission dictionary.

`anchors_from_segments` stands where the reference's `calc_anchors_using_kmeans` stands.  That one runs scikit-learn's KMeans
with a random initialisation (random_state=13); scikit-learn's generator is not reproduced here.  This is a deterministic
1-D k-means (Lloyd's iterations from quantile initial centres), so its anchors are close to, not equal to, the reference's.
"""
from __future__ import annotations

import contextlib
import io
import json
import math
import os
from time import time
from types import SimpleNamespace

import numpy as np
import torch


def tiou_vectorized(segments1, segments2, without_center_coords=False, center_length=True):
    """(M, N) temporal IoU of every pair.  Rows are (centre, length) when center_length, else (start, end); with
    without_center_coords the inputs are (M, 1) / (N, 1) lengths laid on a common centre."""
    if without_center_coords:
        segments1 = torch.cat([torch.zeros_like(segments1), segments1], dim=1)
        segments2 = torch.cat([torch.zeros_like(segments2), segments2], dim=1)
    M, N = segments1.shape[0], segments2.shape[0]
    if center_length:
        s1, e1 = segments1[:, 0] - segments1[:, 1] / 2, segments1[:, 0] + segments1[:, 1] / 2
        s2, e2 = segments2[:, 0] - segments2[:, 1] / 2, segments2[:, 0] + segments2[:, 1] / 2
    else:
        s1, e1 = segments1[:, 0], segments1[:, 1]
        s2, e2 = segments2[:, 0], segments2[:, 1]
    s1, e1 = s1.view(M, 1), e1.view(M, 1)
    s2, e2 = s2.view(1, N), e2.view(1, N)
    inter = torch.clamp(torch.min(e1, e2) - torch.max(s1, s2), min=0.0)
    union = (e1 - s1) + (e2 - s2) - inter
    union = torch.min(torch.max(e1, e2) - torch.min(s1, s2), union)      # never more than the hull
    return inter / (union + 1e-8)


def calculate_f1(recall, precision):
    return 2 * recall * precision / (recall + precision + 1e-16)


def add_dict_to_another_dict(one_dict, another_dict):
    return {k: another_dict.get(k, 0) + v for k, v in one_dict.items()}


def get_lr(optimizer):
    for group in optimizer.param_groups:
        return group["lr"]


def get_corner_coords(predictions):
    """(B, N, >=2) rows (centre, length, ...) -> (start, end, ...), in place as the reference does"""
    starts = predictions[:, :, 0] - predictions[:, :, 1] / 2
    ends = predictions[:, :, 0] + predictions[:, :, 1] / 2
    predictions[:, :, 0] = starts
    predictions[:, :, 1] = ends
    return predictions


def select_topk_predictions(model_output, k):
    """(B, N, F) -> the k rows of highest confidence (column 2) per video, in that order; equal confidences keep their row
    order (a stable sort: the reference's argsort does not say)"""
    B, N, F = model_output.shape
    order = model_output[:, :, 2].argsort(descending=True, stable=True)
    return model_output.gather(1, order.view(B, N, 1).expand(B, N, F))[:, :k, :]


def trim_proposals(model_output, duration_in_secs):
    """clip starts to [0, duration] and ends to (-inf, duration], in place"""
    dur = torch.as_tensor(duration_in_secs, dtype=model_output.dtype, device=model_output.device).view(-1, 1)
    zero = torch.zeros(1, dtype=model_output.dtype, device=model_output.device)
    model_output[:, :, 0] = torch.min(torch.max(model_output[:, :, 0], zero), dur)
    model_output[:, :, 1] = torch.min(model_output[:, :, 1], dur)
    return model_output


def non_max_suppresion(video_preds, tIoU_threshold):
    """greedy NMS of one video's (n, F) rows (start, end, ...) sorted by confidence: a kept row removes every later one whose
    tIoU with it is not below the threshold.  (The name is the reference's.)"""
    kept = []
    while len(video_preds) > 0:
        kept.append(video_preds[0:1, :])
        if len(video_preds) == 1:
            break
        tious = tiou_vectorized(video_preds[0:1, :], video_preds[1:, :], center_length=False).reshape(-1)
        video_preds = video_preds[1:, :][tious < tIoU_threshold]
    return torch.cat(kept) if kept else video_preds


NMS_METHODS = ("hard", "linear", "gaussian")


def soft_nms(video_preds, method, tiou_thresh=0.0, sigma=0.5, min_score=1e-3, k=None):
    """Soft-NMS (Bodla et al. 2017) of one video's (n, F >= 3) rows (start, end, conf, ...) sorted by confidence, the
    definition of bmhrl_proposal_select_soft in plain torch fp32 (and math.exp), bit for bit: at most k times (None: n) the
    alive row of largest current score is picked, ties to the earlier row; a score below min_score (None: no floor) ends
    the loop; every other alive row whose tIoU with the pick is not below tiou_thresh is removed ("hard") or rescored by
    1 - tIoU ("linear") or exp(-tIoU^2 / sigma) ("gaussian").  Returns the picked rows in pick order, column 2 rewritten."""
    if method not in NMS_METHODS:
        raise ValueError(f"soft_nms: method is one of {NMS_METHODS}, got {method!r}")
    n = len(video_preds)
    f32 = dict(dtype=torch.float32, device=video_preds.device)
    segs = video_preds[:, :2].to(torch.float32)
    scores = video_preds[:, 2].to(torch.float32).clone()
    thr = torch.tensor(tiou_thresh, **f32)
    floor = None if min_score is None else torch.tensor(min_score, **f32)
    sigma = torch.tensor(sigma, dtype=torch.float32).item()           # the fp32 value the kernel is handed, as a double
    alive = torch.ones(n, dtype=torch.bool, device=video_preds.device)
    picked, picked_scores = [], []
    for _ in range(n if k is None else min(int(k), n)):
        # the order-preserving integer image of the scores (-0.0 below +0.0, as the kernel's key has it); -1 = not alive
        u = scores.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        image = torch.where(u >= 0x80000000, 0xFFFFFFFF - u, u + 0x80000000)
        image = torch.where(alive, image, torch.full_like(image, -1))
        best = image.max()
        if int(best) < 0:
            break
        i = int(torch.nonzero(image == best)[0])                      # ties: the smaller rank
        if floor is not None and bool(scores[i] < floor):
            break
        picked.append(i)
        picked_scores.append(scores[i].clone())
        alive[i] = False
        tious = tiou_vectorized(segs[i:i + 1], segs, center_length=False).reshape(-1)
        hit = alive & ~(tious < thr)
        if method == "hard":
            alive &= ~hit
        elif method == "linear":
            scores = torch.where(hit, scores * (1 - tious), scores)
        else:
            # float64 weights, each rounded once to fp32 (torch.tensor does that); the product is fp32
            weights = [math.exp(-(t * t) / sigma) for t in tious[hit].tolist()]
            scores[hit] = scores[hit] * torch.tensor(weights, **f32)
    if not picked:
        return video_preds[:0]
    out = video_preds[torch.tensor(picked, device=video_preds.device)].clone()
    out[:, 2] = torch.stack(picked_scores).to(out.dtype)
    return out


CHAIN_MAX_EVENTS = 32                   # BMHRL_PROPOSAL_CHAIN_MAX_L of include/bmhrl_hip.h


def event_chain(video_rows, max_events, max_tiou=0.0, overlap_weight=0.0, event_cost=0.0, min_length=0.2):
    """Event-chain selection of one video's (n, F >= 3) rows (start, end, score, ...), the definition of
    bmhrl_proposal_chain in plain torch fp32, bit for bit: among the rows longer than min_length whose score exceeds
    event_cost, the chain of at most max_events rows with starts and ends both non-decreasing and a tIoU of neighbours of at
    most max_tiou that maximises the sum of (score - event_cost) minus overlap_weight times the neighbours' tIoUs (by
    dynamic programming over the levels; the first maximum wins everywhere).  Returns (the chosen rows in time order, their
    indices in video_rows as a list, the chain's value as a float; 0.0 for an empty chain)."""
    L = int(max_events)
    if not 1 <= L <= CHAIN_MAX_EVENTS:
        raise ValueError(f"event_chain: max_events is 1 .. {CHAIN_MAX_EVENTS}, got {max_events}")
    dev = video_rows.device
    f32 = dict(dtype=torch.float32, device=dev)
    tau, lam, cost, shortest = (torch.tensor(float(x), **f32) for x in (max_tiou, overlap_weight, event_cost, min_length))
    if not all(bool(x >= 0) for x in (tau, lam, cost, shortest)):
        raise ValueError("event_chain: max_tiou, overlap_weight, event_cost and min_length are numbers >= 0")
    start, end, score = (video_rows[:, c].to(torch.float32) for c in range(3))
    gain = score - cost
    idx = torch.nonzero(((end - start) > shortest) & (score == score) & (gain > 0)).reshape(-1)
    n = len(idx)
    if n == 0:
        return video_rows[:0], [], 0.0
    # (start, end, index) order: two stable sorts, the primary key last (+ 0.0: -0.0 and 0.0 are one value)
    idx = idx[torch.argsort(end[idx] + 0.0, stable=True)]
    idx = idx[torch.argsort(start[idx] + 0.0, stable=True)]
    s, e, g = start[idx], end[idx], gain[idx]
    t = tiou_vectorized(torch.stack([s, e], dim=1), torch.stack([s, e], dim=1), center_length=False)       # t[i, j]
    place = torch.arange(n, device=dev)
    allowed = (place.view(n, 1) < place.view(1, n)) & (e.view(n, 1) <= e.view(1, n)) & (t <= tau)
    penalty = lam * t
    neg = torch.tensor(float("-inf"), **f32)
    V, parents = [g], [None]
    for _ in range(2, L + 1):
        cand = (V[-1].view(n, 1) - penalty) + g.view(1, n)
        cand = torch.where(allowed & (V[-1] > neg).view(n, 1) & (cand > neg), cand, neg)              # (NaN > -inf is False)
        top = cand.max(dim=0).values
        if not bool((top > neg).any()):
            break
        parents.append(torch.where(cand == top.view(1, n), place.view(n, 1), n).min(dim=0).values)    # the first maximum
        V.append(top)
    V = torch.stack(V)
    best = V.max()
    l, j = (int(x) for x in torch.nonzero(V == best)[0])    # row-major: the smaller level, then the earlier position
    picked = []
    while True:
        picked.append(int(idx[j]))
        if l == 0:
            break
        j, l = int(parents[l][j]), l - 1
    picked.reverse()
    return video_rows[torch.tensor(picked, device=dev)], picked, float(best)


def chain_settings(cfg):
    """(max_events, max_tiou, overlap_weight, event_cost, min_length) when cfg sets chain_max_events, None for every other
    cfg.  The other fields are optional: chain_max_tiou 0.0, chain_overlap_weight 0.0, chain_event_cost 0.0,
    chain_min_length 0.2 (rows_to_segments' `shortest`).  Raises ValueError on what bmhrl_proposal_chain would refuse."""
    L = getattr(cfg, "chain_max_events", None)
    if L is None:
        return None
    if isinstance(L, bool) or int(L) != L or not 1 <= int(L) <= CHAIN_MAX_EVENTS:
        raise ValueError(f"chain_max_events is None or an integer 1 .. {CHAIN_MAX_EVENTS}, got {L!r}")
    values = []
    for field, default in (("chain_max_tiou", 0.0), ("chain_overlap_weight", 0.0), ("chain_event_cost", 0.0),
                           ("chain_min_length", 0.2)):
        x = getattr(cfg, field, None)
        x = default if x is None else float(x)
        if not x >= 0.0:                # (NaN included)
            raise ValueError(f"{field} is a number >= 0, got {x!r}")
        values.append(x)
    return (int(L), *values)


def postprocess_preds(model_output, cfg, batch):
    """top-cfg.max_prop_per_vid rows, corner coordinates in seconds, trimmed to the videos' durations: (B, k, F)"""
    model_output = select_topk_predictions(model_output, k=cfg.max_prop_per_vid)
    model_output = get_corner_coords(model_output)
    return trim_proposals(model_output, batch["duration_in_secs"])


def _chained(props, count, chain):
    """chain None: (props, count) as they are; the settings of chain_settings: ops.proposal_chain's (events, length) of
    them, on the device"""
    if chain is None:
        return props, count
    from . import ops
    events, _, length, _ = ops.proposal_chain(props, count, *chain)
    return events, length


def device_proposal_rows(model_output, duration_in_secs, k, nms_tiou, chain=None):
    """ops.proposal_select on a device (B, N, 3) output -> (per video the surviving (start, end, conf) rows as Python lists,
    rows considered per video), after ONE device-to-host copy.  chain: the settings of chain_settings; the survivors then
    go through ops.proposal_chain on the device and the rows are the chain, in time order."""
    from . import ops
    B = model_output.shape[0]
    dur = torch.as_tensor(duration_in_secs, dtype=torch.float32).to(model_output.device, non_blocking=True)
    k = int(k)
    props, count = _chained(*ops.proposal_select(model_output.detach().float().contiguous(), dur, k, nms_tiou), chain)
    packed = torch.cat([props.view(B, -1), count.view(B, 1).to(props.dtype)], dim=1).tolist()
    return [[row[3 * j:3 * j + 3] for j in range(int(row[-1]))] for row in packed], min(k, model_output.shape[1])


def soft_nms_settings(cfg):
    """(k, m, method, tiou_thresh, sigma, min_score) when cfg asks for a soft method (nms_method "linear" / "gaussian") or
    for a pool larger than max_prop_per_vid (nms_candidates), None for every other cfg.  The fields beyond
    max_prop_per_vid and nms_tiou_thresh are optional: nms_method None / "hard", nms_candidates = max_prop_per_vid,
    soft_nms_sigma 0.5, soft_nms_min_score 1e-3 (no floor with "hard").  nms_tiou_thresh None: 0.0 for the soft methods
    (every overlapping row is rescored), no suppression for "hard"."""
    method = getattr(cfg, "nms_method", None) or "hard"
    if method not in NMS_METHODS:
        raise ValueError(f"nms_method is None or one of {NMS_METHODS}, got {method!r}")
    k = int(cfg.max_prop_per_vid)
    m = getattr(cfg, "nms_candidates", None)
    m = k if m is None else int(m)
    if method == "hard" and m <= k:
        return None
    if m < k:
        raise ValueError(f"nms_candidates ({m}) is the pool max_prop_per_vid ({k}) proposals are picked from: it cannot be smaller")
    thr = cfg.nms_tiou_thresh
    if method == "hard":
        return k, m, method, float("inf") if thr is None else thr, 0.5, None
    return k, m, method, 0.0 if thr is None else thr, getattr(cfg, "soft_nms_sigma", 0.5), getattr(cfg, "soft_nms_min_score", 1e-3)


def soft_select_rows(model_output, duration_in_secs, k, m, method, tiou_thresh, sigma, min_score, chain=None):
    """select_rows for the settings of soft_nms_settings: the m rows of highest confidence are the pool, at most k are
    picked.  Device input within the kernel's limits in one call of ops.proposal_select_soft and one device-to-host copy,
    anything else through postprocess_preds (with k := m) and soft_nms; both give the same bits.  chain: the settings of
    chain_settings; the picks then go through ops.proposal_chain (on the device) or event_chain and the rows are the
    chain, in time order."""
    from . import ops
    B, N = model_output.shape[0], model_output.shape[1]
    m = min(int(m), N)
    k_eff = min(int(k), m)
    if model_output.is_cuda and 1 <= k_eff and m <= ops.PROPOSAL_SOFT_MAX_M and N <= ops.PROPOSAL_MAX_N and \
            model_output.shape[2] == 3:
        dur = torch.as_tensor(duration_in_secs, dtype=torch.float32).to(model_output.device, non_blocking=True)
        props, _, count = ops.proposal_select_soft(model_output.detach().float().contiguous(), dur, m, k_eff, method, tiou_thresh,
                                                   sigma, min_score)
        props, count = _chained(props, count, chain)
        packed = torch.cat([props.view(B, -1), count.view(B, 1).to(props.dtype)], dim=1).tolist()
        return [[row[3 * j:3 * j + 3] for j in range(int(row[-1]))] for row in packed], min(int(k), N)
    pool = postprocess_preds(model_output, SimpleNamespace(max_prop_per_vid=m), {"duration_in_secs": duration_in_secs})
    picks = [soft_nms(video_preds, method, tiou_thresh, sigma, min_score, k_eff) for video_preds in pool]
    if chain is not None:
        picks = [event_chain(video_preds, *chain)[0] for video_preds in picks]
    return [video_preds.tolist() for video_preds in picks], min(int(k), N)


def select_rows(model_output, cfg, batch):
    """(per video the (start, end, conf) rows that survive top-k, trimming and NMS, as Python lists; rows considered per
    video): device input in one call of ops.proposal_select, anything else through the piecewise functions.  A cfg with a
    soft nms_method or with nms_candidates > max_prop_per_vid goes through soft_select_rows instead.  A cfg with
    chain_max_events (chain_settings) gets, of those rows, the event chain in time order: on the device routes through
    ops.proposal_chain before the one copy to the host, on the host route through event_chain."""
    from . import ops
    soft = soft_nms_settings(cfg)
    chain = chain_settings(cfg)
    extra = {} if chain is None else {"chain": chain}       # (a cfg without the chain fields makes the calls it made)
    if soft is not None:
        return soft_select_rows(model_output, batch["duration_in_secs"], *soft, **extra)
    on_device = model_output.is_cuda and 1 <= int(cfg.max_prop_per_vid) <= ops.PROPOSAL_MAX_K and \
        1 <= model_output.shape[1] <= ops.PROPOSAL_MAX_N and model_output.shape[2] == 3
    if on_device:
        return device_proposal_rows(model_output, batch["duration_in_secs"], cfg.max_prop_per_vid, cfg.nms_tiou_thresh, **extra)
    model_output = postprocess_preds(model_output, cfg, batch)
    rows = []
    for video_preds in model_output:
        if cfg.nms_tiou_thresh is not None:
            video_preds = non_max_suppresion(video_preds, cfg.nms_tiou_thresh)
        if chain is not None:
            video_preds = event_chain(video_preds, *chain)[0]
        rows.append(video_preds.tolist())
    return rows, model_output.shape[1]


def chain_predictions(submission, cfg_or_settings, device=None):
    """The event chain of every video of an ActivityNet-captions submission dictionary (a prop_results_*.json): a new
    dictionary whose entries are the input's entries (sentence, proposal_score and timestamp untouched), filtered to the
    chain and in time order; a video whose chain is empty is left out, as AnetPredictions leaves out a video without
    proposals.  cfg_or_settings: a cfg with chain_max_events or the tuple of chain_settings.  With a device and at most
    ops.PROPOSAL_CHAIN_MAX_P entries per video all videos go through ONE ops.proposal_chain call (a padded (B, P, 3)
    table and its counts) and one copy back; otherwise through event_chain per video.  Times and scores are taken as fp32."""
    chain = tuple(cfg_or_settings) if isinstance(cfg_or_settings, (tuple, list)) else chain_settings(cfg_or_settings)
    if chain is None:
        raise ValueError("chain_predictions: the cfg sets no chain_max_events")
    results = submission["results"]
    vids = list(results)

    def score_of(entry):
        score = entry["proposal_score"]
        return float(score[0] if isinstance(score, (tuple, list)) else score)

    tables = [[[float(p["timestamp"][0]), float(p["timestamp"][1]), score_of(p)] for p in results[v]] for v in vids]
    P = max((len(t) for t in tables), default=0)
    picked = [[] for _ in vids]
    if P > 0:
        from . import ops
        if device is not None and torch.device(device).type == "cuda" and P <= ops.PROPOSAL_CHAIN_MAX_P:
            padded = torch.zeros(len(vids), P, 3)
            for b, t in enumerate(tables):
                if t:
                    padded[b, :len(t)] = torch.tensor(t, dtype=torch.float32)
            count = torch.tensor([len(t) for t in tables], dtype=torch.int32)
            _, index, length, _ = ops.proposal_chain(padded.to(device), count.to(device), *chain)
            packed = torch.cat([index, length.view(-1, 1)], dim=1).tolist()
            picked = [row[:row[-1]] for row in packed]
        else:
            picked = [event_chain(torch.tensor(t, dtype=torch.float32), *chain)[1] if t else [] for t in tables]
    out = {key: value for key, value in submission.items() if key != "results"}
    out["results"] = {v: [results[v][i] for i in rows] for v, rows in zip(vids, picked) if rows}
    return out


def rows_to_segments(video_rows, shortest=0.2):
    """one video's (start, end, conf) rows -> its entries of the submission dictionary: times and score rounded to 5 places,
    segments of at most `shortest` seconds dropped (the reference's AnetPredictions.add_new_predictions)"""
    vid_preds = []
    for pred_start, pred_end, pred_conf in video_rows:
        start, end = round(pred_start, 5), round(pred_end, 5)
        if end - start > shortest:
            # (the score is a one-element tuple in the reference: a trailing comma there; json writes it as a list)
            vid_preds.append({"sentence": "", "proposal_score": (round(pred_conf, 5),), "timestamp": [start, end]})
    return vid_preds


class AnetPredictions:
    """collects a validation pass's proposals in the ActivityNet-captions submission layout (the reference's class of the
    same name: same dictionary, same counters, same file name)"""

    def __init__(self, cfg, phase, epoch):
        self.predictions = {"version": "VERSION 1.0", "external_data": {"used": True, "details": ""}, "results": {}}
        self.phase = phase
        self.epoch = epoch
        self.cfg = cfg
        self.segments_used = 0
        self.segments_total = 0
        self.num_vid_w_no_props = 0

    def add_new_predictions(self, model_output, batch):
        """model_output (B, N, 3) rows (centre s, length s, confidence).  Returns the proposals written per video."""
        B = model_output.shape[0]
        rows, k = select_rows(model_output, self.cfg, batch)
        written = 0
        for b, video_rows in enumerate(rows):
            vid_preds = rows_to_segments(video_rows)
            written += len(vid_preds)
            if vid_preds:
                self.predictions["results"][batch["video_ids"][b]] = vid_preds
            else:
                self.num_vid_w_no_props += 1
        self.segments_total += B * k
        self.segments_used += written
        return written / B

    def write_anet_predictions_to_json(self):
        if self.phase != "val_1":       # val_1 and val_2 share their proposals; the reference writes val_1 only
            raise NotImplementedError
        folder = os.path.join(self.cfg.log_path, "submissions")
        name = f"prop_results_{self.phase}_e{self.epoch}_maxprop{self.cfg.max_prop_per_vid}.json"
        self.submission_path = os.path.join(folder, name)
        os.makedirs(folder, exist_ok=True)
        if os.path.exists(self.submission_path):
            self.submission_path = self.submission_path.replace(".json", f"_{time()}.json")
        with open(self.submission_path, "w") as f:
            json.dump(self.predictions, f)

    def evaluate_predictions(self):
        from .epoch_loops.validation_loops import calculate_metrics
        print(f"{self.cfg.max_prop_per_vid * self.segments_used / max(self.segments_total, 1):.2f} props/vid")
        if self.num_vid_w_no_props > 0:
            print(f"Number of videos with no proposals: {self.num_vid_w_no_props}")
        with contextlib.redirect_stdout(io.StringIO()):
            return calculate_metrics(self.cfg.reference_paths, self.submission_path, self.cfg.tIoUs, self.cfg.max_prop_per_vid,
                                     verbose=True, only_proposals=True, evaluator=getattr(self.cfg, "caption_evaluator", None),
                                     evaluator_options=getattr(self.cfg, "proposal_evaluator_options", None))


def anchors_from_segments(lengths, k, iters=100):
    """k anchor lengths (sorted list of floats) from ground-truth segment lengths: 1-D k-means, deterministic -- initial
    centres at the quantiles (i + 0.5) / k, Lloyd's iterations until nothing moves or `iters` are done, a cluster that
    loses all its points keeps its centre.  See the module docstring for how this relates to the reference's KMeans."""
    x = np.sort(np.asarray(lengths, dtype=np.float64).reshape(-1))
    x = x[x > 0]
    if k < 1 or x.size < k:
        raise ValueError(f"anchors_from_segments: need at least k = {k} positive lengths, got {x.size}")
    centres = np.quantile(x, (np.arange(k) + 0.5) / k)
    for _ in range(iters):
        edges = (centres[1:] + centres[:-1]) / 2            # sorted centres: clusters are intervals
        label = np.searchsorted(edges, x, side="left")
        sums = np.bincount(label, weights=x, minlength=k)
        cnts = np.bincount(label, minlength=k)
        new = np.where(cnts > 0, sums / np.maximum(cnts, 1), centres)
        new.sort()
        if np.array_equal(new, centres):
            break
        centres = new
    return [float(c) for c in centres]
