"""Sampled decoding: one JSON line with the event-timed bmhrl_sample_step launch (V=10172, R in {16, 64, 256}, over 200
launches) for plain sampling (T=1, k=0, p=1), top-k (k=50) and top-p (p=0.9), and the 30-token decode at config 2 (B=16,
Tv=256, Ta=800, end_idx=-1) for n in {1, 4, 8} samples per clip beside greedy (incremental) and beam K=4 in the same
process."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bmhrl_amd import ops  # noqa: E402
from bmhrl_amd import synthetic as syn  # noqa: E402
from bmhrl_amd.decode import beam_decode, greedy_decode, sample_decode  # noqa: E402
from tests.bench_beam import launch_us  # noqa: E402
from tests.test_beam_gpu import _time_ms  # noqa: E402
from tests.test_decode_gpu import _agent  # noqa: E402

START, PAD = 2, 1


def launch_times(V=10172):
    dev = torch.device("cuda:0")
    res = {}
    for R in (16, 64, 256):
        g = torch.Generator().manual_seed(R)
        lp = torch.log_softmax(torch.randn(R, V, generator=g) * 3, -1).to(dev)
        fin = torch.zeros(R, dtype=torch.uint8, device=dev)
        tok = torch.zeros(R, dtype=torch.int64, device=dev)
        out = torch.zeros(R, 31, dtype=torch.int64, device=dev)
        slp, slq = torch.zeros(R, 31, device=dev), torch.zeros(R, 31, device=dev)
        sums = torch.zeros(R, device=dev)
        seed = torch.zeros(1, dtype=torch.int64, device=dev)
        t = torch.zeros(1, dtype=torch.int64, device=dev)
        for name, (T, k, p) in (("plain", (1.0, 0, 1.0)), ("topk50", (1.0, 50, 1.0)), ("topp0.9", (1.0, 0, 0.9))):
            res[f"step_{name}_R{R}_us"] = round(launch_us(lambda: ops.sample_step(lp, V, R, V, T, k, p, 0, seed, t, -1, PAD, fin,
                                                                                   tok, out, sums, slp, slq)), 2)
    return res


def decode_times(V=10172, L=30):
    agent = _agent(torch.device("cuda:0"), V)
    b = syn.synthetic_batch(16, 256, 800, L, V, seed=0)
    fs = {k: b[k].to("cuda:0") for k in ("rgb", "flow", "audio")}
    times = {}
    times["greedy"], _ = _time_ms(lambda: greedy_decode(agent, fs, L, START, -1, PAD, "audio_video"))
    times["beam4"], _ = _time_ms(lambda: beam_decode(agent, fs, L, START, -1, PAD, "audio_video", beam_size=4))
    for n in (1, 4, 8):
        times[f"sample{n}"], toks = _time_ms(lambda: sample_decode(agent, fs, L, START, -1, PAD, "audio_video", n=n, top_k=50,
                                                                   top_p=0.9, seed=n))
        assert toks.shape == (16, L + 1)
    return times


def main():
    launches = launch_times()
    times = decode_times()
    print(json.dumps({"bench": "sample_decode_config2", "tokens": 30, "B": 16, "V": 10172, **launches,
                      **{f"{k}_ms": round(v, 2) for k, v in times.items()},
                      "sample4_over_beam4": round(times["sample4"] / times["beam4"], 3),
                      "sample1_over_greedy": round(times["sample1"] / times["greedy"], 3)}))


if __name__ == "__main__":
    main()
