"""Tuning aid (a script, not a test): the segment crop at the size of a validation pass on learned proposals -- V = 16 videos of
300 video / 800 audio rows, 100 proposals each with random starts and lengths (P = 1600 clips).

  crop     the three ops.crop_segments calls (rgb, flow, audio) out of the resident full-length stacks, output width = the
           longest crop of the stack, as predict.VideoFeatures.crop sizes it.  Timed as a graph of repeated calls between two
           events after a warm replay.  Bytes moved = the rows read plus every byte of the outputs written, over that time,
           beside the 6.29 TB/s a float4 copy streams on this chip.
  files    the route without it, for the same segments: FeaturePacker.pack + DeviceBatcher.upload from .npy files written to
           a temporary directory (memory-mapped, in the page cache), in batches of `--batch` clips, as wall time between
           synchronisations.
Both routes produce the same clips (checked on the first batch).  Prints ONE JSON line."""
import argparse, json, os, sys, tempfile, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bmhrl_amd import loader as L, ops

V, SV, SA, PER_VIDEO, PAD = 16, 300, 800, 100, 1
HBM_COPY_TBS = 6.29


def timed(fn, reps=10, rounds=5):
    """us per call of fn: a graph of `reps` calls, replayed `rounds` times between two events (after one warm replay)"""
    g = torch.cuda.CUDAGraph(); s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
        with torch.cuda.graph(g):
            for _ in range(reps):
                fn()
    torch.cuda.current_stream().wait_stream(s)
    g.replay(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(rounds):
        g.replay()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (reps * rounds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=100, help="clips per batch of the file route")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    durations = [float(d) for d in rng.uniform(60.0, 240.0, V)]
    segs = []
    for v in range(V):
        for _ in range(PER_VIDEO):
            start = float(rng.uniform(0.0, 0.9) * durations[v])
            segs.append((v, start, min(durations[v], start + float(rng.uniform(0.01, 0.5) * durations[v]))))
    P = len(segs)
    res = {"config": {"V": V, "S_video": SV, "S_audio": SA, "P": P, "file_route_batch": args.batch}, "runs": []}

    with tempfile.TemporaryDirectory() as folder:
        arrays = {"rgb": [], "flow": [], "audio": []}
        for v in range(V):
            for name, shape, fname in (("rgb", (SV, L.D_VIDEO), f"v{v}_rgb.npy"), ("flow", (SV, L.D_VIDEO), f"v{v}_flow.npy"),
                                       ("audio", (SA, L.D_AUDIO), f"v{v}.npy")):
                a = rng.standard_normal(shape).astype(np.float32)
                np.save(os.path.join(folder, fname), a)
                arrays[name].append(a)
        stacks = {k: torch.from_numpy(np.stack(a)).to(dev) for k, a in arrays.items()}
        lens = {"rgb": SV, "flow": SV, "audio": SA}
        src_len = {k: torch.full((V,), n, dtype=torch.int32, device=dev) for k, n in lens.items()}
        dur = torch.tensor(durations, dtype=torch.float64, device=dev)
        video = torch.tensor([s[0] for s in segs], dtype=torch.int32, device=dev)
        times = torch.tensor([s[1:] for s in segs], dtype=torch.float64, device=dev)
        rows = {k: [L.crop_rows(n, s, e, durations[v])[1] for v, s, e in segs] for k, n in lens.items()}
        width = {k: max(r) for k, r in rows.items()}
        pads = {"rgb": float(PAD), "flow": 0.0, "audio": float(PAD)}
        outs = {k: torch.empty(P, width[k], stacks[k].shape[2], device=dev) for k in stacks}

        def crop():
            for k in ("rgb", "flow", "audio"):
                ops.crop_segments(stacks[k], src_len[k], dur, video, times, pads[k], width[k], out=outs[k])

        moved = sum(4 * stacks[k].shape[2] * (sum(rows[k]) + P * width[k]) for k in stacks)      # rows read + outputs written
        res["crop_bytes_moved"] = moved
        res["crop_output_shapes"] = {k: list(o.shape) for k, o in outs.items()}

        packer = L.FeaturePacker(folder, folder, PAD)
        batcher = L.DeviceBatcher(packer, dev)
        clips = [L.Clip(f"v{v}", "", s, e, durations[v]) for v, s, e in segs]
        batches = [clips[i:i + args.batch] for i in range(0, P, args.batch)]

        def files():
            for b in batches:
                batch = batcher.upload(b)
                batcher.wait(batch)
                batcher.release(batch)
            torch.cuda.synchronize()

        crop()
        first = batcher.upload(batches[0])
        batcher.wait(first); torch.cuda.synchronize()
        n0 = len(batches[0])
        res["same_clips"] = all(
            torch.equal(outs[k][:n0, :first["feature_stacks"][k].shape[1]], first["feature_stacks"][k]) and
            bool((outs[k][:n0, first["feature_stacks"][k].shape[1]:] == pads[k]).all()) for k in outs)
        batcher.release(first)

        for _ in range(2):
            r = {"crop_us": round(timed(crop), 1)}
            r["crop_tb_per_s"] = round(moved / (r["crop_us"] * 1e-6) / 1e12, 3)
            r["crop_share_of_copy_rate"] = round(r["crop_tb_per_s"] / HBM_COPY_TBS, 3)
            files()                                                  # warm: staging buffers, page cache
            t0 = time.perf_counter()
            for _ in range(3):
                files()
            r["file_route_us"] = round((time.perf_counter() - t0) / 3 * 1e6, 1)
            res["runs"].append(r)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
