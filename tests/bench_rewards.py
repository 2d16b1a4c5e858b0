"""Device caption rewards (csrc/rewards.hip): one JSON line with
- the device time of one worker-reward call (scorer.reward_fn() on bound captions: the bmhrl_rewards launch and the
  discount product) and of the launch alone, for CIDEr and BLEU at B = 16 and 64, L = 30 (vocabulary 10172, a 20000-caption
  corpus, references of 8..20 words), from graphs of 20 calls; and the eager call (host enqueue included);
- the host restatement's time for the same CIDEr / BLEU rows at B = 16 (tests/reward_reference.py, one thread);
- the construction time of the CIDEr scorer (string table, vocab maps, document-frequency hash table);
- captured worker RL steps/s (bench.py's configuration, B = 16) with synthetic rewards and with device CIDEr
  rewards, re-bound before every replay or bound once."""
import json
import os
import random
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bmhrl_amd import synthetic as syn  # noqa: E402
from bmhrl_amd.rewards import BleuScorer, CiderScorer  # noqa: E402
from tests import reward_reference as rr  # noqa: E402

V, L, N_CORPUS = 10172, 30, 20000


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


def graph_us(fn, calls=20, n=50):
    """device time of one call: `calls` calls captured in one graph, replayed n times (no host work in the window)"""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    us = launch_us(g.replay, n) / calls
    del g
    return us


def data(seed=0):
    rng = random.Random(seed)
    itos = ["<unk>", "<pad>", "<s>", "</s>"] + [f"w{i}" for i in range(V - 4)]
    word = lambda: itos[4 + min(int(rng.paretovariate(1.1)), V - 5)]        # noqa: E731  (Zipf-like word draw)
    corpus = [[word() for _ in range(rng.randint(6, 20))] for _ in range(N_CORPUS)]
    caps = [" ".join(word() for _ in range(rng.randint(8, 20))) for _ in range(64)]
    stoi = {s: i for i, s in enumerate(itos)}
    hyp = torch.tensor([[stoi[word()] for _ in range(L)] for _ in range(64)], dtype=torch.int64)
    return itos, corpus, caps, hyp


def steps_per_s(reward_fn, bind=None, steps=50, warmup=5):
    from bmhrl_amd.train import CaptionTrainer
    dev = torch.device("cuda:0")
    cfg = syn.default_cfg(dout_p=0.1, rl_att_layers=2)
    b = syn.synthetic_batch(16, 256, 800, L, V, seed=0)
    tr = CaptionTrainer(cfg, V, dev, lr=1e-4, phase="worker", reward_fn=reward_fn)
    tr.agent.train()
    tr.value_net.train()
    fs = {k: b[k].to(dev) for k in ("rgb", "flow", "audio")}
    tr.capture(fs, b["captions"].to(dev), warmup=2)

    def step():
        if bind is not None:
            bind()
        tr.replay()
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


def main():
    dev = torch.device("cuda:0")
    itos, corpus, caps, hyp = data()
    vocab = types.SimpleNamespace(itos=itos)
    t0 = time.perf_counter()
    cid = CiderScorer(vocab, iter(corpus), dev, 0.9, 0.7)
    build_s = time.perf_counter() - t0
    ble = BleuScorer(vocab, dev, 0.9, 0.7)
    out = {"metric": "worker reward call", "cider_construction_s": round(build_s, 3), "df_entries": int(cid.df.grams.shape[0])}
    for name, sc in (("cider", cid), ("bleu", ble)):
        for B in (16, 64):
            pred = hyp[:B].to(dev)
            sc.bind(caps[:B])
            fn = sc.reward_fn()
            out[f"{name}_B{B}_call_us"] = round(graph_us(lambda: fn(pred, None)), 1)
            out[f"{name}_B{B}_launch_us"] = round(graph_us(lambda: sc._launch(pred)), 1)
            out[f"{name}_B{B}_eager_call_us"] = round(launch_us(lambda: fn(pred, None)), 1)
    df = rr.precook_corpus(corpus)
    rows = hyp[:16].tolist()
    t0 = time.perf_counter()
    for i, r in enumerate(rows):
        rr.cider_scores(itos, r, caps[i], df)
    out["host_restatement_cider_B16_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    t0 = time.perf_counter()
    for i, r in enumerate(rows):
        rr.bleu_scores(itos, r, caps[i])
    out["host_restatement_bleu_B16_ms"] = round((time.perf_counter() - t0) * 1e3, 1)

    Ls = syn.synthetic_batch(16, 256, 800, L, V, seed=0)["captions"].shape[1] - 1      # sampled tokens per caption
    rewards = syn.synthetic_rewards(16, Ls, seed=2).to(dev)
    out["captured_worker_steps_per_s_synthetic"] = round(steps_per_s(lambda s, c: rewards), 1)
    torch.cuda.empty_cache()
    cid.bind(caps[:16])
    out["captured_worker_steps_per_s_device_cider"] = round(steps_per_s(cid.reward_fn(), bind=lambda: cid.bind(caps[:16])), 1)
    torch.cuda.empty_cache()
    out["captured_worker_steps_per_s_device_cider_no_rebind"] = round(steps_per_s(cid.reward_fn()), 1)
    torch.cuda.empty_cache()
    out["captured_worker_steps_per_s_synthetic_again"] = round(steps_per_s(lambda s, c: rewards), 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
