"""Tuning aid: the accumulate launch (bmhrl_accum_segments) over the captioning bucket of the bench configuration (B = 16,
Tv = 256, Ta = 800, L = 30, V = 10172), with the trainer's own table -- the gradients where autograd leaves them -- and over the
flat bucket (word 6 = 0): `first` form (8 B per element: read g, write accum) and `add` form (12 B per element: read g and
accum, write accum), against the Adam pass of the same table.  HIP events, warm, graphs of 20 launches replayed 10 times, two
runs in the process.  Prints ONE JSON line."""
import json, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bmhrl_amd import ops, synthetic as syn
from bmhrl_amd.train import CaptionTrainer

B, TV, TA, L, V = 16, 256, 800, 30, 10172


def timed(fn, reps=20, rounds=10):
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
    dev = torch.device("cuda:0")
    b = syn.synthetic_batch(B, TV, TA, L, V, seed=0)
    fs = {k: b[k].to(dev) for k in ("rgb", "flow", "audio")}; cap = b["captions"].to(dev)
    t = CaptionTrainer(syn.default_cfg(dout_p=0.1), V, dev, lr=1e-4)
    t.agent.train()
    for _ in range(2):
        t.step(fs, cap)
    torch.cuda.synchronize()
    o = t.opt
    table, n_seg, n_blk, _ = o._segment_plan()
    flat_table = table.clone(); flat_table[:, 6] = 0
    acc = torch.zeros_like(o.grad)
    ctl = torch.tensor([0.5, 1.0], dtype=torch.float32).to(dev)
    res = {"config": {"B": B, "Tv": TV, "Ta": TA, "L": L, "V": V}, "elements": o.n, "parameters": n_seg,
           "read_in_place": int((table[:, 6] != 0).sum()), "blocks": n_blk, "runs": []}
    for run in range(2):
        r = {}
        for label, tb in (("in_place", table), ("flat", flat_table)):
            ctl[1] = 1.0
            us_first = timed(lambda: ops.accum_segments(tb, n_seg, n_blk, o.grad, acc, ctl))
            ctl[1] = 0.0
            us_add = timed(lambda: ops.accum_segments(tb, n_seg, n_blk, o.grad, acc, ctl))
            r[label] = {"first_us": round(us_first, 1), "first_GBps": round(8 * o.n / us_first / 1e3, 1),
                        "add_us": round(us_add, 1), "add_GBps": round(12 * o.n / us_add / 1e3, 1)}
        us_adam = timed(lambda: ops.adam_segments(table, n_seg, n_blk, o.flat, o.grad, o.exp_avg, o.exp_avg_sq, 0.0, 0.9, 0.999,
                                                  1e-8, 0.0, 1, 1.0), reps=5, rounds=20)
        r["adam_us"] = round(us_adam, 1)
        r["adam_GBps"] = round(30 * o.n / us_adam / 1e3, 1)      # 16 B read + 12 B written + 2 B shadow per parameter
        res["runs"].append(r)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
