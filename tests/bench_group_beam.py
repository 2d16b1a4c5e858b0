"""Diverse (group) beam search at config 2 (B=16, Tv=256, Ta=800, V=10172, 30 tokens, end_idx=-1): one JSON line with
  * the event-timed bmhrl_group_beam_select launch for (K, G) in {(4, 2), (8, 4), (16, 4)} beside bmhrl_beam_select at the
    same K, in the same process, on one token's real log-probs;
  * the 30-token decode for beam_groups in {1, 2, 4} at K = 4 and 8 beside the plain beam decode (no keywords: the code the
    package ran before it had groups), alternating, the least and the largest of `--rounds` rounds each.
--plain-only times the no-keyword decodes alone and uses nothing the keywords added."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bmhrl_amd import ops  # noqa: E402
from bmhrl_amd import synthetic as syn  # noqa: E402
from bmhrl_amd.decode import BeamDecoder, beam_decode  # noqa: E402
from tests.bench_beam import launch_us  # noqa: E402
from tests.test_decode_gpu import _agent  # noqa: E402

PAD, START = 1, 2


def select_times(agent, fs, V, B, L):
    out = {}
    for K, G in ((4, 2), (8, 4), (16, 4)):
        dec = BeamDecoder.for_batch(agent, fs, L, START, -1, PAD, K)
        with torch.no_grad():
            assert dec.begin(fs)
            dec.step()                                        # real log-probs in dec.logp
        R = B * K
        scores = torch.randn(R, device=dec.dev)               # (in place: the inputs stay valid candidates)
        fin = torch.zeros(R, dtype=torch.uint8, device=dec.dev)
        args = (dec.logp, V, scores, fin, dec.parent, dec.tok, dec.out, dec.t, dec.last_live, B, K, V, -1, PAD)
        out[f"beam_select_K{K}_us"] = round(launch_us(lambda: ops.beam_select(*args)), 2)
        out[f"group_select_K{K}_G{G}_us"] = round(launch_us(lambda: ops.group_beam_select(*args, G, 0.5)), 2)
        out[f"group_select_K{K}_G1_us"] = round(launch_us(lambda: ops.group_beam_select(*args, 1, 0.5)), 2)
        agent.__dict__.pop("_beam_decoders")                  # (K = 16 holds the most state: one decoder at a time)
        del dec
    return out


def decode_times(agent, fs, L, rounds, groups=(1, 2, 4)):
    out = {}
    for K in (4, 8):
        ms = {"plain": []}
        for G in groups or (None,):                           # one G at a time: a change of G captures the step again
            runs = [("plain", {})] + ([(f"G{G}", dict(beam_groups=G, diversity_penalty=0.5))] if groups else [])
            ms.update({name: [] for name, _ in runs[1:]})
            for r in range(rounds + 1):                       # round 0 warms up: construction, capture
                for name, kw in runs:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    toks = beam_decode(agent, fs, L, START, -1, PAD, "audio_video", beam_size=K, **kw)
                    torch.cuda.synchronize()
                    if r:
                        ms[name].append((time.perf_counter() - t0) * 1e3)
                    assert toks.shape == (fs["audio"].shape[0], L + 1)
        for name, v in ms.items():
            out[f"decode_K{K}_{name}_ms"] = [round(min(v), 2), round(max(v), 2)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--plain-only", action="store_true",
                    help="only the no-keyword decodes: this file, copied into a tree from before the keywords, times that tree")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    V, B, L = 10172, 16, 30
    agent = _agent(dev, V)
    b = syn.synthetic_batch(B, 256, 800, L, V, seed=0)
    fs = {k: b[k].to(dev) for k in ("rgb", "flow", "audio")}
    res = {"bench": "group_beam_config2", "tokens": L, "B": B, "V": V, "rounds": a.rounds}
    if a.plain_only:
        res.update(decode_times(agent, fs, L, a.rounds, groups=()))
    else:
        res.update(select_times(agent, fs, V, B, L))
        res.update(decode_times(agent, fs, L, a.rounds))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
