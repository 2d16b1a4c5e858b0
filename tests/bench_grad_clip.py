"""Tuning aid: the gradient-norm launch of the trainer at the config-2 bucket (both gradient placements) against the Adam
pass of the same trainer, and the captured config-2 step with and without grad_clip (A/B/A/B).  Event-timed, warm, graphs
of 20 launches; prints one line per measurement."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bmhrl_amd import ops, synthetic as syn
from bmhrl_amd.train import CaptionTrainer

dev = torch.device("cuda:0")
b = syn.synthetic_batch(16, 256, 800, 30, 10172, seed=0)
fs = {k: b[k].to(dev) for k in ("rgb", "flow", "audio")}; cap = b["captions"].to(dev)


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


def trainer(clip):
    tr = CaptionTrainer(syn.default_cfg(dout_p=0.1), 10172, dev, lr=1e-4, grad_clip=clip)
    tr.agent.train()
    return tr


tr = trainer(1.0)
for _ in range(2):
    tr.step(fs, cap)
torch.cuda.synchronize()
o = tr.opt
n = o.n
table, n_seg, n_blk, _ = o._segment_plan()
direct = int((table[:, 6] != 0).sum())
flat_table = table.clone(); flat_table[:, 6] = 0
for run in range(2):
    us_d = timed(lambda: ops.grad_norm(table, n_seg, n_blk, o.grad, 1.0, o._norm_ws, o.hyper))
    us_f = timed(lambda: ops.grad_norm(flat_table, n_seg, n_blk, o.grad, 1.0, o._norm_ws, o.hyper))
    us_a = timed(lambda: o.step(1.0), reps=5, rounds=20)
    print(f"run {run}: norm launch (2 kernels), {n / 1e6:.1f} M elements, {n_seg} parameters ({direct} read in place), {n_blk} blocks: "
          f"in place {us_d:.1f} us = {4 * n / us_d / 1e6:.2f} TB/s | flat bucket {us_f:.1f} us = {4 * n / us_f / 1e6:.2f} TB/s | "
          f"Adam pass {us_a:.1f} us = {30 * n / us_a / 1e6:.2f} TB/s (16 B read + 12 B written + 2 B shadow per parameter)")
del tr, o, table, flat_table

steps = {}
for label, clip in (("plain", None), ("clip", 1.0)):
    t = trainer(clip)
    t.capture(fs, cap, warmup=3)
    for _ in range(10):
        t.replay()
    steps[label] = t
torch.cuda.synchronize()
for run in range(2):
    for label in ("plain", "clip"):
        t = steps[label]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            t.replay()
        e1.record(); torch.cuda.synchronize()
        print(f"run {run}: captured config-2 step, {label}: {e0.elapsed_time(e1) / 200:.3f} ms")
print(f"last norm {float(steps['clip'].last_grad_norm):.4f}, coefficient {float(steps['clip'].last_clip_coef):.4f}")
