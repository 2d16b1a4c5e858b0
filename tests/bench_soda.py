"""SODA_c on the device (bmhrl_amd/evaluate.py soda_groups / soda_scores, csrc/soda.hip): one JSON
line for the synthetic ActivityNet-sized job of tests/bench_caption_eval.py -- 4 900 videos (--videos), two ground-truth
files, scored
- "gt_props": with the first file's own segments as proposals, tIoU 0.5;
- "props100": with 100 proposals per video (--proposals), tIoUs 0.3 / 0.5 / 0.7 / 0.9.
Per job: the grouping time (soda_groups), the tokenize / encode time (soda_encode), the device time of the matrix launches
and of the DP launches (events around each call, the offsets check included), the wall time of soda_scores and of the
whole evaluate_soda, each twice.  The yardstick, in the same process: evaluate.meteor_pairs -- the per-prefix launch
reading column hyp_len - 1 -- on the same cells materialised as pairs, wall time and device time (events around every
ops.meteor call), twice.  When the job has more than --yardstick-cells cells the yardstick runs on the groups of the first
--yardstick-videos videos and its times are scaled by cells / yardstick cells ("yardstick_scale")."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bmhrl_amd import evaluate as E, ops  # noqa: E402
from bmhrl_amd.rewards import MeteorScorer  # noqa: E402
from tests.bench_caption_eval import job  # noqa: E402
from tests.meteor_reference import DictStemmer, dict_synonyms  # noqa: E402

DEV = "cuda:0"


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def timed_launches(groups, enc, tables, tious):
    """(matrix ms, dp ms, (G, T, 4) result) of the two launches over all chunks, events around each call"""
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)            # noqa: E731
    vmap, vstem, syn_off, syn_ids = dev(tables.vmap), dev(tables.vstem), dev(tables.syn_off), dev(tables.syn_ids)
    hyp_d, ref_d, stem_d, len_d = dev(enc["hyp"]), dev(enc["ref"]), dev(enc["ref_stem"]), dev(enc["ref_len"])
    tious_d = dev(np.asarray(tious, dtype=np.float64))
    out = np.zeros((len(groups), len(tious), 4))
    ms = [0.0, 0.0]
    for lo, hi, c in E.soda_chunks(groups, enc):
        L, R = c["L"], c["R"]
        hyp_off, ref_off, cell_off = dev(c["hyp_off"]), dev(c["ref_off"]), dev(c["cell_off"])
        hyp_idx, ref_idx, pred_seg, ref_seg = dev(c["hyp_idx"]), dev(c["ref_idx"]), dev(c["pred_seg"]), dev(c["ref_seg"])
        S = torch.empty(int(c["cell_off"][-1]), dtype=torch.float64, device=DEV)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        torch.cuda.synchronize()
        ev[0].record()
        ops.meteor_matrix(hyp_d[:, :L], vmap, vstem, syn_off, syn_ids, ref_d[:, :R], stem_d[:, :R], len_d, hyp_idx, ref_idx,
                          hyp_off, ref_off, cell_off, MeteorScorer.alpha, MeteorScorer.beta, MeteorScorer.gamma_frag, S)
        ev[1].record()
        res = ops.soda_dp(pred_seg, ref_seg, hyp_off, ref_off, cell_off, S, tious_d)
        ev[2].record()
        torch.cuda.synchronize()
        ms[0] += ev[0].elapsed_time(ev[1])
        ms[1] += ev[1].elapsed_time(ev[2])
        out[lo:hi] = res.cpu().numpy()
    return ms[0], ms[1], out


def yardstick(groups, tok, tables):
    """(wall s, device ms, scores) of evaluate.meteor_pairs on the groups' cells materialised as pairs"""
    hyps = [tok(h) for g in groups for h in g.pred_sentences for _ in g.ref_sentences]
    refs = [tok(r) for g in groups for _ in g.pred_sentences for r in g.ref_sentences]
    events = []
    launch = ops.meteor

    def recorded(*a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch(*a, **k)
        e1.record()
        events.append((e0, e1))
    ops.meteor = recorded
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scores = E.meteor_pairs(hyps, refs, tables, DEV)
        wall = time.perf_counter() - t0
    finally:
        ops.meteor = launch
    torch.cuda.synchronize()
    return wall, sum(a.elapsed_time(b) for a, b in events), scores


def measure(gts, submission, tious, yard_videos, yard_cells):
    ev = E.DenseCaptionEvaluator(gts, submission, tious, 1000, device=DEV, stemmer=DictStemmer(), synonyms=dict_synonyms,
                                 soda=True)
    tables = ev.meteor_tables()
    t0 = time.perf_counter()
    groups, by_video = E.soda_groups(ev.ground_truths, ev.prediction)
    out = {"tious": tious, "grouping_s": round(time.perf_counter() - t0, 3), "groups": len(groups)}
    t0 = time.perf_counter()
    enc = E.soda_encode(groups, tables, ev._tok)
    out["tokenize_encode_s"] = round(time.perf_counter() - t0, 3)
    out["distinct_hypotheses"], out["distinct_references"] = len(enc["hyp"]), len(enc["ref"])
    out["rows"] = int(sum(len(m[0]) for m in enc["members"]))
    out["cells"] = cells = int(sum(len(m[0]) * len(m[1]) for m in enc["members"]))
    note("encoded", out)
    timed_launches(groups[:64], enc, tables, tious)                          # warm-up
    out["matrix_ms"], out["dp_ms"] = [], []
    for _ in range(2):
        m, d, res = timed_launches(groups, enc, tables, tious)
        out["matrix_ms"].append(round(m, 3))
        out["dp_ms"].append(round(d, 3))
    out["soda_scores_s"], out["evaluate_soda_s"] = [], []
    for _ in range(2):
        t0 = time.perf_counter()
        again = E.soda_scores(groups, tious, tables, DEV, ev._tok)
        out["soda_scores_s"].append(round(time.perf_counter() - t0, 3))
        assert again.tobytes() == res.tobytes()
        t0 = time.perf_counter()
        scores = ev.evaluate_soda()
        out["evaluate_soda_s"].append(round(time.perf_counter() - t0, 3))
    out["scores"] = {k: [round(x, 6) for x in v] for k, v in scores.items()}
    note("new route", out)
    # the yardstick on the same cells (of the first videos when the job is large), scaled by the cell count
    part = groups
    if cells > yard_cells:
        first = set(sorted(by_video)[:yard_videos])
        part = [g for g in groups if g.video in first]
    n = sum(len(g.pred_sentences) * len(g.ref_sentences) for g in part)
    out["yardstick_cells"], out["yardstick_scale"] = n, round(cells / n, 3)
    out["yardstick_wall_s"], out["yardstick_device_ms"] = [], []
    for _ in range(2):
        wall, ms, pair_scores = yardstick(part, ev._tok, tables)
        out["yardstick_wall_s"].append(round(wall * cells / n, 3))
        out["yardstick_device_ms"].append(round(ms * cells / n, 3))
    # the same numbers by both routes: the yardstick's pairs are the first groups' cells in order
    S = []
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)                                     # noqa: E731
    head = part[:50]
    enc_h = E.soda_encode(head, tables, ev._tok)
    for lo, hi, c in E.soda_chunks(head, enc_h):
        s = torch.empty(int(c["cell_off"][-1]), dtype=torch.float64, device=DEV)
        ops.meteor_matrix(dev(enc_h["hyp"]), dev(tables.vmap), dev(tables.vstem), dev(tables.syn_off), dev(tables.syn_ids),
                          dev(enc_h["ref"]), dev(enc_h["ref_stem"]), dev(enc_h["ref_len"]), dev(c["hyp_idx"]), dev(c["ref_idx"]),
                          dev(c["hyp_off"]), dev(c["ref_off"]), dev(c["cell_off"]), MeteorScorer.alpha, MeteorScorer.beta,
                          MeteorScorer.gamma_frag, s)
        S.append(s.cpu().numpy())
    S = np.concatenate(S)
    assert S.tobytes() == pair_scores[:len(S)].tobytes()
    out["cells_compared_bitwise"] = len(S)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=4900)
    ap.add_argument("--proposals", type=int, default=100)
    ap.add_argument("--yardstick-videos", type=int, default=500)
    ap.add_argument("--yardstick-cells", type=int, default=500000)
    a = ap.parse_args()
    gts, own, many = job(a.videos, a.proposals)
    out = {"metric": "SODA_c evaluation", "videos": a.videos, "proposals": a.proposals,
           "gt_props": measure(gts, own, [0.5], a.yardstick_videos, a.yardstick_cells),
           "props100": measure(gts, many, [0.3, 0.5, 0.7, 0.9], a.yardstick_videos, a.yardstick_cells)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
