"""Runs the reference's own utilities/proposal_utils.py on synthetic predictions and writes tests/golden/proposals.json and
tests/golden/proposals.npz: the inputs and what its tiou_vectorized (both modes), postprocess_preds, non_max_suppresion and
AnetPredictions.add_new_predictions returned.  Inputs and recorded outputs only.

proposal_utils.py imports sklearn.cluster, utilities.captioning_utils and epoch_loops.captioning_epoch_loops for functions that
are not called here; empty stand-ins in sys.modules let it import (the file itself is loaded by path).

Cases: B = 3 videos of 12.5 / 60 / 211.3 s; N in {1, 5, 100, 101, 4097} candidates per video; k in {5, 100};
nms_tiou in {None, 0.4, 0.9}.  Every N > 1 carries, among its highest confidences, segments that start below 0, end past the
duration, start past the duration, shrink below 0.2 s when trimmed, are identical, and are nested; at N = 5 every candidate of
the first video starts past its duration, so that video ends with no proposal.  Confidences are pairwise distinct within a
video (asserted): the reference's argsort leaves the order of equal ones open.
The json holds the case list, the counters and the small tIoU records (fp32 as hex strings of the bit patterns, 8 digits per
element); the npz holds the tensors as they are -- `in_<N>` fp32 (3, N, 3), `post_<N>_<k>` fp32 (3, k_eff, 3), `nms_<case>`
fp32 rows of the three videos one after another (their counts are in the json) -- and the results dictionaries as
`res_<case>` float64 rows (start, end, score) in dictionary order (video ids and counts in the json): the other fields of a
segment are constants.  tests/proposal_reference.py load_golden() puts both back together.
usage: make_proposal_golden.py REFERENCE_CHECKOUT"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "proposals.json")
OUT_NPZ = os.path.join(HERE, "proposals.npz")
DURATIONS = [12.5, 60.0, 211.3]
VIDEO_IDS = ["v_short", "v_mid", "v_long"]
NS = [1, 5, 100, 101, 4097]
KS = [5, 100]
THRESHOLDS = [None, 0.4, 0.9]


def load_reference(checkout):
    for name, attrs in (("sklearn", {}), ("sklearn.cluster", {"KMeans": None}), ("utilities", {}),
                        ("utilities.captioning_utils", {"HiddenPrints": None}), ("epoch_loops", {}),
                        ("epoch_loops.captioning_epoch_loops", {"calculate_metrics": None})):
        mod = types.ModuleType(name)
        mod.__dict__.update(attrs)
        sys.modules[name] = mod
    spec = importlib.util.spec_from_file_location("reference_proposal_utils", os.path.join(checkout, "utilities", "proposal_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def bits(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32).reshape(-1)
    return "".join(f"{v:08x}" for v in a.view(np.uint32).tolist())


def special_rows(dur):
    """(centre, length) rows, most confident first"""
    return [
        (1.0, 6.0),                    # starts below 0
        (dur - 2.0, 10.0),             # ends past the duration
        (dur + 8.0, 4.0),              # starts past the duration: trimmed to (dur, dur)
        (dur + 0.05, 0.3),             # 0.2 s long before, 0.1 s after trimming
        (dur / 2, dur / 4),            # a segment ...
        (dur / 2, dur / 4),            # ... its identical twin ...
        (dur / 2, dur / 10),           # ... and one nested in both
        (dur / 2 + dur / 40, dur / 4),  # a near copy (tIoU 0.8 with the twins)
        (dur / 3, 0.1),                # shorter than 0.2 s from the start
    ]


def make_predictions(N, rng):
    pred = np.zeros((len(DURATIONS), N, 3), dtype=np.float32)
    for b, dur in enumerate(DURATIONS):
        centre = rng.uniform(-0.05 * dur, 1.05 * dur, N)
        length = rng.uniform(0.05, 0.5 * dur, N) * rng.choice([0.1, 0.5, 1.0], N)
        rank = rng.permutation(N)                                   # rank 0 = most confident
        if N == 5 and b == 0:
            centre = dur + 3.0 + rng.uniform(0, 5, N)               # every candidate starts past the end
            length = rng.uniform(0.5, 2.0, N)
        elif N > 1:
            rows = special_rows(dur)[:max(1, min(len(special_rows(dur)), N - 1))]
            where = rng.choice(N, len(rows), replace=False)
            for j, (w, (c, l)) in enumerate(zip(where, rows)):
                centre[w], length[w] = c, l
                other = int(np.nonzero(rank == j)[0][0])            # give row w the j-th highest confidence
                rank[other], rank[w] = rank[w], j
        conf = ((N - rank).astype(np.float64) / (N + 1)).astype(np.float32)
        assert len(set(conf.tolist())) == N, "confidences must be pairwise distinct within a video"
        pred[b, :, 0], pred[b, :, 1], pred[b, :, 2] = centre, length, conf
    return torch.from_numpy(pred)


def main():
    ref = load_reference(sys.argv[1])
    rng = np.random.default_rng(20260)
    out = {"durations": DURATIONS, "video_ids": VIDEO_IDS, "tiou": [], "cases": []}

    for M, N in ((1, 1), (3, 7), (8, 5)):
        a = torch.from_numpy(np.stack([rng.uniform(-5, 50, M), rng.uniform(0, 30, M)], 1).astype(np.float32))
        b = torch.from_numpy(np.stack([rng.uniform(-5, 50, N), rng.uniform(0, 30, N)], 1).astype(np.float32))
        b[0] = a[0]                                                  # an identical pair
        for mode, kw in (("center_length", {}), ("start_end", {"center_length": False})):
            x, y = a.clone(), b.clone()
            if mode == "start_end":
                x[:, 1] += x[:, 0]
                y[:, 1] += y[:, 0]
            out["tiou"].append({"mode": mode, "M": M, "N": N, "a": bits(x), "b": bits(y), "tiou": bits(ref.tiou_vectorized(x, y, **kw))})
        la, lb = a[:, 1:2].clone(), b[:, 1:2].clone()
        out["tiou"].append({"mode": "lengths", "M": M, "N": N, "a": bits(la), "b": bits(lb),
                            "tiou": bits(ref.tiou_vectorized(la, lb, without_center_coords=True))})

    batch = {"duration_in_secs": DURATIONS, "video_ids": VIDEO_IDS}
    arrays = {}
    f32 = lambda t: np.ascontiguousarray(t.detach().numpy(), dtype=np.float32)      # noqa: E731
    for N in NS:
        pred = make_predictions(N, rng)
        arrays[f"in_{N}"] = f32(pred)
        for k in KS:
            for thr in THRESHOLDS:
                cfg = types.SimpleNamespace(max_prop_per_vid=k, nms_tiou_thresh=thr)
                post = ref.postprocess_preds(pred.clone(), cfg, batch)
                arrays[f"post_{N}_{k}"] = f32(post)
                name = f"{N}_{k}_{thr}"
                case = {"N": N, "k": k, "nms_tiou": thr, "k_eff": post.shape[1]}
                if thr is not None:
                    kept = [f32(ref.non_max_suppresion(v.clone(), thr)) for v in post]
                    arrays[f"nms_{name}"] = np.concatenate(kept)
                    case["nms_counts"] = [len(v) for v in kept]
                anet = ref.AnetPredictions(cfg, "val_1", 0)
                case["returned"] = anet.add_new_predictions(pred.clone(), batch)
                results = anet.predictions["results"]
                for segs in results.values():
                    assert all(set(s) == {"sentence", "proposal_score", "timestamp"} and s["sentence"] == "" and
                               type(s["proposal_score"]) is tuple and len(s["proposal_score"]) == 1 for s in segs)
                case["results_videos"] = [[vid, len(segs)] for vid, segs in results.items()]
                arrays[f"res_{name}"] = np.array([s["timestamp"] + [s["proposal_score"][0]] for segs in results.values() for s in segs],
                                                 dtype=np.float64).reshape(-1, 3)
                case["segments_used"], case["segments_total"] = anet.segments_used, anet.segments_total
                case["num_vid_w_no_props"] = anet.num_vid_w_no_props
                out["cases"].append(case)
    assert any(c["num_vid_w_no_props"] > 0 for c in out["cases"])
    with open(OUT, "w") as f:
        row = lambda r: json.dumps(r, separators=(",", ":"))                     # noqa: E731  (one record per line)
        f.write('{"durations":%s,"video_ids":%s,\n"tiou":[\n%s],\n"cases":[\n%s]}\n' % (
            row(DURATIONS), row(VIDEO_IDS), ",\n".join(map(row, out["tiou"])), ",\n".join(map(row, out["cases"]))))
    np.savez_compressed(OUT_NPZ, **arrays)
    print(OUT, os.path.getsize(OUT), "bytes;", OUT_NPZ, os.path.getsize(OUT_NPZ), "bytes")


if __name__ == "__main__":
    main()
