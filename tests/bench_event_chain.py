"""Tuning aid (a script, not a test): event-chain selection beside the select call that feeds it,
timed as tests/bench_soft_nms.py times: graphs of repeated calls, replayed between two events after a warm replay.

  a  ops.proposal_select_soft, gaussian, m = k = 100: the call that feeds b
  b  ops.proposal_chain on a's output, B = 16, P = 100, L = 10
  c  ops.proposal_select_soft, gaussian, m = k = 1024: the call that feeds d
  d  ops.proposal_chain on c's output, B = 16, P = 1024, L = 32 (the worst case: every row eligible, every level run)
  e  d's table with L = 10
All in one process, a .. e and then e .. a, twice.

The same script takes tests/bench_soft_nms.py's synthetic set and reports, for hard NMS (section 26's route) and for a Gaussian
pool of 1024 followed by a chain (L = 10, tau = 0.1, lambda = 0.5, cost = 0.05): events per video, the mean over the videos of
the largest tIoU between two events of a video, and DenseCaptionEvaluator's detection precision / recall at tIoU 0.3 / 0.5 /
0.7 / 0.9.  Synthetic figures: no pass / fail, no claim about a trained generator.  Prints ONE JSON line."""
import json, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from types import SimpleNamespace
import numpy as np
from bmhrl_amd import ops, proposal_utils as pu
from bmhrl_amd.evaluate import DenseCaptionEvaluator
from tests.bench_proposals import timed
from tests.bench_soft_nms import B, N, DUR, synthetic_set

TIOUS = [0.3, 0.5, 0.7, 0.9]
CHAIN = dict(chain_max_events=10, chain_max_tiou=0.1, chain_overlap_weight=0.5, chain_event_cost=0.05)


def largest_tiou(rows):
    if len(rows) < 2:
        return 0.0
    seg = torch.tensor(rows, dtype=torch.float32)[:, :2]
    t = pu.tiou_vectorized(seg, seg, center_length=False)
    return float((t - torch.eye(len(rows))).max())


def synthetic_figures(dev):
    pred, durations, gt = synthetic_set()
    output = torch.from_numpy(pred).to(dev)
    vids = sorted(gt)
    figures = {}
    for name, extra in (("hard_nms", {}),
                        ("gaussian_pool1024_chain", {"nms_method": "gaussian", "nms_tiou_thresh": None, "nms_candidates": 1024, **CHAIN})):
        cfg = SimpleNamespace(**{"max_prop_per_vid": 100, "nms_tiou_thresh": 0.4, **extra})
        rows, _ = pu.select_rows(output, cfg, {"duration_in_secs": durations})
        results = {vid: pu.rows_to_segments(r) for vid, r in zip(vids, rows)}
        submission = {"version": "VERSION 1.0", "external_data": {"used": True, "details": ""},
                      "results": {vid: segs for vid, segs in results.items() if segs}}
        ev = DenseCaptionEvaluator([gt], submission, TIOUS, only_proposals=True, device=dev)
        detection = [ev.evaluate_detection(t) for t in TIOUS]
        figures[name] = {"events_per_video": round(sum(len(s) for s in results.values()) / len(vids), 2),
                         "mean_largest_tiou": round(float(np.mean([largest_tiou(r) for r in rows])), 4),
                         "precision": [round(float(p), 4) for p, _ in detection],
                         "recall": [round(float(r), 4) for _, r in detection]}
    return figures


def main():
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cpu").manual_seed(0)
    pred = torch.stack([torch.rand(B, N, generator=gen) * DUR, torch.rand(B, N, generator=gen) * 59.5 + 0.5,
                        torch.rand(B, N, generator=gen)], dim=-1).to(dev)
    dur = torch.tensor([DUR - b for b in range(B)], dtype=torch.float32, device=dev)
    feed100 = lambda: ops.proposal_select_soft(pred, dur, 100, 100, "gaussian", 0.0, 0.5, None)
    feed1024 = lambda: ops.proposal_select_soft(pred, dur, 1024, 1024, "gaussian", 0.0, 0.5, None)
    p100, _, c100 = feed100()
    p1024, _, c1024 = feed1024()
    res = {"config": {"B": B, "N": N, "chain": [0.1, 0.5, 0.05, 0.2]}, "runs": []}
    calls = {
        "a_select_soft_m100_us": feed100,
        "b_chain_P100_L10_us": lambda: ops.proposal_chain(p100, c100, 10, 0.1, 0.5, 0.05),
        "c_select_soft_m1024_us": feed1024,
        "d_chain_P1024_L32_us": lambda: ops.proposal_chain(p1024, c1024, 32, 0.1, 0.5, 0.05),
        "e_chain_P1024_L10_us": lambda: ops.proposal_chain(p1024, c1024, 10, 0.1, 0.5, 0.05),
    }
    res["rows_per_video"] = {"P100": round(float(c100.float().mean()), 1), "P1024": round(float(c1024.float().mean()), 1)}
    res["chain_length"] = {name: round(float(fn()[2].float().mean()), 1) for name, fn in calls.items() if "chain" in name}
    for run in range(2):
        for order in (list(calls), list(calls)[::-1]):
            res["runs"].append({name: round(timed(calls[name]), 1) for name in order})
    res["synthetic"] = synthetic_figures(dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
