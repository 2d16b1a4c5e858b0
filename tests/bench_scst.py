"""Tuning aid: the time split of one self-critical step (bmhrl_amd/scst.py) at the bench configuration (B = 16, Tv = 256,
Ta = 800, L = 30, V = 10172) with n = 4 rollouts per clip, i.e. 64 caption rows:
- the rollout (SampleDecoder: captured token steps, host reads of `done` included), the BLEU reward launch on the 64 rows,
  the eager training forward + backward over the sampled captions, each between HIP events around warm calls;
- the two new launches (bmhrl_rollout_advantage, bmhrl_policy_loss_fwd) and the dense backward bmhrl_policy_loss_bwd (without
  and with the entropy term) beside bmhrl_smooth_kl_bwd on the same (rows, V) in the same process -- both write a dense fp32
  (rows, V) gradient, 4 bytes per element (8 with the entropy term, which also reads the log-probs) -- from graphs of 20 launches
  replayed 10 times, the kernels alternating, two runs.  Prints ONE JSON line."""
import json, os, sys, types, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bmhrl_amd import ops, scst, synthetic as syn
from bmhrl_amd.epoch_loops.captioning_scst_loops import off_default_stream, rollout_forward
from bmhrl_amd.model.bm_hrl_agent import BMHrlAgent
from bmhrl_amd.rewards import BleuScorer

B, TV, TA, L, V, N = 16, 256, 800, 30, 10172, 4
PAD, START, END = 1, 2, 3


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


def eager_ms(fn, calls=3):
    """ms per eager call between two events (after one warm call); the calls end in a synchronise"""
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def main():
    dev = torch.device("cuda:0")
    b = syn.synthetic_batch(B, TV, TA, L, V, seed=0)
    fs = {k: b[k].to(dev) for k in ("rgb", "flow", "audio")}
    cfg = syn.default_cfg(dout_p=0.1)
    cfg.device = "cuda:0"
    agent = BMHrlAgent(cfg, types.SimpleNamespace(trg_voc_size=V, train_vocab=types.SimpleNamespace(vectors=None))).to(dev)
    agent.teach_worker()
    itos = ["<unk>", "<pad>", "<s>", "</s>"] + [f"w{i}" for i in range(V - 4)]
    scorer = BleuScorer(types.SimpleNamespace(itos=itos), dev, 0.9, 0.7)
    caps = [" ".join(itos[4 + (7 * i + 3 * j) % (V - 4)] for j in range(8 + i % 12)) for i in range(B)]
    rows = B * N
    ro = scst.rollout(agent, fs, L, START, END, PAD, "audio_video", n=N, seed=1)
    scores = scst.prefix_scores(scorer, ro.toks, caps)

    def step():
        with off_default_stream(dev):
            agent.train(); agent.zero_grad(set_to_none=True)
            pred = rollout_forward(agent, fs, ro, "audio_video", PAD)
            loss, _ = scst.self_critical_loss(pred, ro, scores, "mean")
            loss.backward()
    m = ro.m
    g = torch.Generator().manual_seed(0)
    logp = torch.log_softmax(torch.randn(rows * m, V, generator=g), -1).to(dev)
    R = rows * m
    act = ro.toks[:, 1:].reshape(-1).contiguous()
    trg = act.clone()
    w = torch.randn(R, generator=g).to(dev); beta = torch.rand(R, generator=g).to(dev); one = torch.ones(1, device=dev)
    drow = torch.ones(R, device=dev); grad = torch.empty(R, V, device=dev); rl = torch.empty(R, device=dev); re = torch.empty(R, device=dev)
    res = {"config": {"B": B, "Tv": TV, "Ta": TA, "L": L, "V": V, "n": N, "rows": rows, "steps": m, "loss_rows": R}, "runs": []}
    for run in range(2):
        r = {"rollout_ms": round(eager_ms(lambda: scst.rollout(agent, fs, L, START, END, PAD, "audio_video", n=N, seed=1)), 3),
             "reward_launch_us": round(timed(lambda: scorer._launch(ro.toks[:, 1:])), 1),
             "forward_backward_ms": round(eager_ms(step), 3),
             "rollout_advantage_us": round(timed(lambda: ops.rollout_advantage(ro.toks, N, m, END, scores)), 1),
             "policy_loss_fwd_us": round(timed(lambda: ops.policy_loss_fwd(logp, V, act, w, None, 0.0, None, rl, re, R, V)), 1),
             "policy_loss_fwd_entropy_us": round(timed(lambda: ops.policy_loss_fwd(logp, V, act, w, None, 0.0, beta, rl, re, R, V)), 1)}
        for rep in range(2):                                    # the kernels alternate
            for name, nbytes, fn in (
                    ("policy_loss_bwd", 4, lambda: ops.policy_loss_bwd(logp, V, act, w, None, 0.0, None, one, drow, grad, V, R, V)),
                    ("smooth_kl_bwd", 4, lambda: ops.smooth_kl_bwd(logp, V, trg, None, None, None, 0.7, PAD, -1, one, None, 0, grad,
                                                                   R, V, wrt_logits=False)),
                    ("policy_loss_bwd_entropy", 8, lambda: ops.policy_loss_bwd(logp, V, act, w, None, 0.0, beta, one, drow, grad, V,
                                                                               R, V))):
                us = timed(fn)
                r.setdefault(name, []).append({"us": round(us, 2), "GBps": round(nbytes * R * V / us / 1e3, 1)})
        res["runs"].append(r)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
