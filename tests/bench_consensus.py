"""Consensus choice: one JSON line with
  * the event-timed bmhrl_consensus launch at B = 16, K in {4, 16}, steps = 30, N = 4, with token weights and without: graphs
    of 20 launches replayed 10 times after one warm replay (method of tests/bench_accum.py), two runs, beside the host path
    of bmhrl_amd/decode.py (consensus_host, what a caller pays without the kernel: a sync, a copy and Python loops) on the same
    hypotheses, the minimum of three calls;
  * with --decode, the 30-token config-2 decode (B = 16, Tv = 256, Ta = 800, V = 10172, end_idx = -1) for sample n = 4 and beam
    K = 4 with select="logp" and select="consensus": the minimum of --reps timed decodes each (method of
    tests/bench_constrain.py).  On a tree without the keyword (the parent of the change that added it) only the launch-free
    figures of the plain decoders are printed: run both trees alternately in one session and compare the minima."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bmhrl_amd import _lib, ops  # noqa: E402
from bmhrl_amd import decode  # noqa: E402
from bmhrl_amd import synthetic as syn  # noqa: E402
from tests.bench_accum import timed  # noqa: E402
from tests.test_beam_gpu import _time_ms  # noqa: E402
from tests.test_decode_gpu import _agent  # noqa: E402

START, PAD, END = 2, 1, 3
HAS = hasattr(ops, "consensus")


def hypotheses(B, K, steps, V=40, seed=0):
    """(B * K, steps + 1) int64 over few ids (repeated grams, as captions of one clip share words); a third of the rows end"""
    g = torch.Generator().manual_seed(seed + K)
    h = torch.randint(4, V, (B * K, steps + 1), generator=g)
    h[:, 0] = START
    for r in range(0, B * K, 3):
        e = int(torch.randint(steps // 2, steps + 1, (1,), generator=g))
        h[r, e] = END
        h[r, e + 1:] = PAD
    return h


def launch_times(B=16, steps=30, N=4, V=40):
    dev = torch.device("cuda:0")
    lib = _lib.load()
    res = {}
    w = (torch.rand(V, generator=torch.Generator().manual_seed(1)) * 3.75 + 0.25).to(dev)
    for K in (4, 16):
        cpu = hypotheses(B, K, steps, V)
        hist = cpu.to(dev)
        util = torch.empty(B, K, dtype=torch.float64, device=dev)
        for tag, wt in (("plain", None), ("weighted", w)):
            fn = lambda: lib.bmhrl_consensus(hist.data_ptr(), hist.stride(0), B, K, steps, END, N, ops._ptr(wt),
                                             0 if wt is None else V, util.data_ptr(), None, ops.stream())
            res[f"K{K}_{tag}_us"] = [round(timed(fn), 2) for _ in range(2)]
            host = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                U = decode.consensus_host(hist.view(B, K, -1), END, N, wt)
                torch.cuda.synchronize()
                host.append((time.perf_counter() - t0) * 1e3)
            assert torch.equal(U, ops.consensus(hist, steps, K, END, N, wt))
            res[f"K{K}_{tag}_host_ms"] = round(min(host), 2)
    return res


def decode_times(reps, V=10172, L=30):
    agent = _agent(torch.device("cuda:0"), V)
    b = syn.synthetic_batch(16, 256, 800, L, V, seed=0)
    fs = {k: b[k].to("cuda:0") for k in ("rgb", "flow", "audio")}
    args = (agent, fs, L, START, -1, PAD, "audio_video")
    runs = {"sample4": lambda **kw: decode.sample_decode(*args, n=4, top_k=50, top_p=0.9, seed=4, **kw),
            "beam4": lambda **kw: decode.beam_decode(*args, beam_size=4, **kw)}
    ways = (("plain", {}),) if not HAS else (("plain", {}), ("logp", dict(select="logp")), ("consensus", dict(select="consensus")))
    times = {}
    for name, fn in runs.items():
        for tag, kw in ways:
            runs_ms = []
            for _ in range(reps):                                         # (_time_ms: one untimed run, then the timed one)
                ms, toks = _time_ms(lambda: fn(**kw))
                runs_ms.append(round(ms, 2))
            assert toks.shape == (16, L + 1)
            times[f"{name}_{tag}_ms"] = runs_ms
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--decode", action="store_true")
    a = ap.parse_args()
    res = {"bench": "consensus", "B": 16, "steps": 30, "N": 4, "has_consensus": HAS}
    if HAS:
        res.update(launch_times())
    if a.decode:
        res.update(decode_times(a.reps))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
