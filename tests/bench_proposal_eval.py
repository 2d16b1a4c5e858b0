"""Proposal metrics on the device against the host loops (bmhrl_amd/evaluate.py, csrc/proposal_eval.hip; DESIGN.md section
28): one JSON line for the "100 props" job of tests/bench_caption_eval.py -- 4 900 videos (--videos), 100 random proposals
each (--proposals), two ground-truth files, tIoUs 0.3 / 0.5 / 0.7 / 0.9 -- with a seeded proposal_score on every proposal.
In one process, alternating twice (both readings are kept):
- "detection": host detection_scores for the four thresholds against detection_scores_device, wall time to a synchronise
  with the table building and every copy included; the values must be equal;
- "hits_launch_ms": the ops.tiou_hits launch alone between events (tables resident, one warm-up), with the bytes it must
  move (segments and group tables in, the two int32 tables out) and their rate;
- "pairing": host tokenized_pairs for the four thresholds against the device route up to tokenized_pairs' return (tables,
  launches, copies and the indexing of the token tuples; every sentence tokenized beforehand on both sides); the returns
  must be equal;
- "pairs_launch_ms": the ops.tiou_pairs launch alone between events, threshold 0.5;
- "recall": proposal_recall at the ten thresholds 0.5 .. 0.95 (no host route exists; the restatement is checked in the tests)."""
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
from tests.bench_caption_eval import job  # noqa: E402

DEV = "cuda:0"
TIOUS = [0.3, 0.5, 0.7, 0.9]


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, round(time.perf_counter() - t0, 4)


def event_ms(fn):
    fn()                                                                # warm-up
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=4900)
    ap.add_argument("--proposals", type=int, default=100)
    a = ap.parse_args()
    gts, _, many = job(a.videos, a.proposals)
    rng = random.Random(1)
    for segs in many["results"].values():
        for seg in segs:
            seg["proposal_score"] = [round(rng.random(), 5)]
    make = lambda backend: E.DenseCaptionEvaluator(gts, many, TIOUS, 1000, only_proposals=True, device=DEV,  # noqa: E731
                                                   tiou_backend=backend)
    host, device = make("host"), make("device")
    torch.zeros(1, device=DEV)                                          # the context exists before anything is timed
    torch.cuda.synchronize()
    out = {"metric": "proposal evaluation", "videos": a.videos, "proposals": a.proposals, "tious": TIOUS,
           "detection": {"host_s": [], "device_s": []}, "pairing": {"host_s": [], "device_s": []}, "recall": {"device_s": []}}

    for _ in range(2):
        want, dt = wall(lambda: [E.detection_scores(host.ground_truths, host.prediction, t) for t in TIOUS])
        out["detection"]["host_s"].append(dt)
        got, dt = wall(lambda: E.detection_scores_device(E.segment_tables(device.ground_truths, device.prediction), TIOUS, DEV))
        out["detection"]["device_s"].append(dt)
        assert got == want
    out["detection"]["scores"] = got

    tables = device.segment_tables()
    pred_seg, ref_seg, file_groups, video_groups = tables.on(DEV)
    tious_d = torch.tensor(TIOUS, dtype=torch.float64, device=DEV)
    bufs = (torch.empty(4, file_groups.sum_p, dtype=torch.int32, device=DEV),
            torch.empty(4, file_groups.sum_r, dtype=torch.int32, device=DEV))
    moved = (pred_seg.numel() + ref_seg.numel()) * 8 + file_groups.groups.numel() * 4 + file_groups.out_off.numel() * 8 + \
        (bufs[0].numel() + bufs[1].numel()) * 4
    ms = [event_ms(lambda: ops.tiou_hits(pred_seg, ref_seg, file_groups, tious_d, True, out=bufs)) for _ in range(2)]
    out["hits_launch_ms"], out["hits_bytes"] = ms, moved
    out["hits_gb_per_s"] = [round(moved / (m * 1e-3) / 1e9, 1) for m in ms]
    out["groups"], out["cells"] = file_groups.G, int((tables.file_groups[:, 1].astype(np.int64) * tables.file_groups[:, 3]).sum())

    for s in [p["sentence"] for ps in host.prediction.values() for p in ps] + \
            [s for gt in gts for g in gt.values() for s in g["sentences"]]:
        host._tok(E.remove_nonascii(s))
        device._tok(E.remove_nonascii(s))
    for _ in range(2):
        want, dt = wall(lambda: [host.tokenized_pairs(t) for t in TIOUS])
        out["pairing"]["host_s"].append(dt)
        device._tables = device._table_tokens = None                    # the tables and the token lists are built again
        got, dt = wall(lambda: [device.tokenized_pairs(t) for t in TIOUS])
        out["pairing"]["device_s"].append(dt)
        assert got == want
    out["pairing"]["pairs"] = [len(g[2]) for g in got]

    hits, _ = ops.tiou_hits(pred_seg, ref_seg, video_groups, tious_d[1:2], False)
    counts = hits[0].clamp(min=1).to(torch.int64)
    pair_off = torch.zeros(video_groups.sum_p + 1, dtype=torch.int64, device=DEV)
    torch.cumsum(counts, 0, out=pair_off[1:])
    n_pairs = int(pair_off[-1])
    rows = torch.empty(n_pairs, dtype=torch.int32, device=DEV)
    out["pairs_launch_ms"] = [event_ms(lambda: ops.tiou_pairs(pred_seg, ref_seg, video_groups, TIOUS[1], pair_off, n_pairs, out=rows))
                              for _ in range(2)]

    ten = [0.5 + 0.05 * k for k in range(10)]
    for _ in range(2):
        res, dt = wall(lambda: E.proposal_recall(device.ground_truths, device.prediction, ten, device=DEV))
        out["recall"]["device_s"].append(dt)
    out["recall"]["AUC_mean"], out["recall"]["AR@AN_mean"] = sum(res["AUC"]) / 10.0, sum(res["AR@AN"]) / 10.0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
