"""Beam-search decoding at config 2 (B=16, Tv=256, Ta=800, V=10172, 30 tokens, end_idx=-1): one JSON line with the decode
times of greedy (incremental), beam K in {1, 4, 8} and greedy over the batch repeated 4x, plus the per-launch times of
bmhrl_beam_select (K=4, one token) and of the two bmhrl_beam_reorder launches at the last step (every buffer moved: rows
[0, 29] of every beam whose parent is another beam)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bmhrl_amd import ops  # noqa: E402
from bmhrl_amd import synthetic as syn  # noqa: E402
from bmhrl_amd.decode import BeamDecoder  # noqa: E402
from tests.test_beam_gpu import config2_times  # noqa: E402
from tests.test_decode_gpu import _agent  # noqa: E402


def launch_us(fn, n=200):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def main():
    dev = torch.device("cuda:0")
    V, B, K, L = 10172, 16, 4, 30
    agent = _agent(dev, V)
    times = config2_times(agent)
    b = syn.synthetic_batch(B, 256, 800, L, V, seed=0)
    fs = {k: b[k].to(dev) for k in ("rgb", "flow", "audio")}
    dec = BeamDecoder.for_batch(agent, fs, L, 2, -1, 1, K)
    with torch.no_grad():
        assert dec.begin(fs)
        dec.step()                                            # real log-probs in dec.logp
    R = B * K
    scores = torch.randn(R, device=dev)                        # (select: a fresh copy of the state for every launch is not
    fin = torch.zeros(R, dtype=torch.uint8, device=dev)        #  needed -- in place, the inputs stay valid candidates)
    sel = launch_us(lambda: ops.beam_select(dec.logp, V, scores, fin, dec.parent, dec.tok, dec.out, dec.t, dec.last_live, B, K,
                                            V, -1, 1))
    dec.t.fill_(L - 1)
    dec.parent.copy_(torch.tensor([1, 0, 3, 2] * B, dtype=torch.int32))
    reorder = launch_us(lambda: [ops.beam_reorder(dec._table, dec._n_buffers, dec._n_blocks, dec.parent, R, K, dec.t, p)
                                 for p in (0, 1)])
    moved = sum(s.numel() * s.element_size() for s in dec._scratch)
    print(json.dumps({"bench": "beam_decode_config2", "tokens": L, "B": B, "V": V,
                      **{f"{k}_ms": round(v, 2) for k, v in times.items()},
                      "beam4_over_greedy_x4": round(times["beam4"] / times["greedy_x4"], 3),
                      "beam1_over_greedy": round(times["beam1"] / times["greedy"], 3),
                      "beam_select_us": round(sel, 2), "beam_reorder_us": round(reorder, 2),
                      "reorder_state_mb": round(moved / 2**20, 1)}))


if __name__ == "__main__":
    main()
