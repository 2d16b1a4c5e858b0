"""Tuning aid: the four launches of the DETR word loss (csrc/word_loss.hip) at the configuration's shape
(B = 16, Q = 100, C = V + 1 = 10173, L = 30), each alone and the whole forward + backward, next to (a) ops.log_softmax_ on
the same (1600, 10173) buffer -- the bytes-per-second yardstick of the two streaming passes -- and (b) the reference's
route on the device, on its own timeline (host clock around a synchronize): torch softmax + gather, the copy to the host,
scipy's linear_sum_assignment per sample, F.cross_entropy forward and backward.  HIP events, warm, graphs of 20 launches
replayed 10 times, two runs in the process.  Prints ONE JSON line."""
import json, os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bmhrl_amd import ops

B, Q, C, L, PAD, EOS = 16, 100, 10173, 30, 1, 0.1


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


def reference_route(x, cap):
    """what the reference's train_detr does for this loss, with the logits already on the device; us of host time"""
    from scipy.optimize import linear_sum_assignment
    torch.cuda.synchronize(); t0 = time.perf_counter()
    xr = x.detach().requires_grad_(True)
    prob = xr.detach().flatten(0, 1).softmax(-1)
    words = [c[c != PAD] for c in cap]
    cost = (-prob[:, torch.cat(words)]).view(B, Q, -1).cpu()
    sizes = [len(w) for w in words]
    idx = [linear_sum_assignment(c[i]) for i, c in enumerate(cost.split(sizes, -1))]
    cls = torch.full((B, Q), C - 1, dtype=torch.int64, device=x.device)
    for b, (i, j) in enumerate(idx):
        cls[b, torch.as_tensor(i, device=x.device)] = words[b][torch.as_tensor(j, device=x.device)]
    w = torch.ones(C, device=x.device); w[-1] = EOS
    torch.nn.functional.cross_entropy(xr.transpose(1, 2), cls, w).backward()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def main():
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    x = (3 * torch.randn(B, Q, C, generator=g)).to(dev)
    cap = torch.randint(4, C - 1, (B, L), generator=g)
    for b in range(B):
        cap[b, 8 + (b * 3) % 23:] = PAD
    cap = cap.to(dev)
    with torch.no_grad():
        words, n, lse, x_none, gathered, cost = ops.word_cost(x, cap, PAD)
        qot = ops.lsa_match(cost, n)
        tgt, row_w, ls = ops.word_loss(words, n, qot, lse, x_none, gathered, EOS, C)
        dx = torch.empty_like(x)
        lp = x.reshape(B * Q, C).clone()

        def whole():
            w_, n_, lse_, none_, g_, c_ = ops.word_cost(x, cap, PAD)
            t_, rw_, ls_ = ops.word_loss(w_, n_, ops.lsa_match(c_, n_), lse_, none_, g_, EOS, C)
            ops.word_loss_bwd(x, lse_, t_, rw_, ls_, None, out=dx)

        nbytes = 4 * B * Q * C
        res = {"config": {"B": B, "Q": Q, "C": C, "L": L, "words": n.cpu().tolist()}, "runs": []}
        for run in range(2):
            r = {}
            r["word_cost_us"] = timed(lambda: ops.word_cost(x, cap, PAD))
            r["lsa_match_us"] = timed(lambda: ops.lsa_match(cost, n, out=qot))
            r["word_loss_us"] = timed(lambda: ops.word_loss(words, n, qot, lse, x_none, gathered, EOS, C))
            r["word_loss_bwd_us"] = timed(lambda: ops.word_loss_bwd(x, lse, tgt, row_w, ls, None, out=dx))
            r["forward_backward_us"] = timed(whole)
            r["log_softmax_us"] = timed(lambda: ops.log_softmax_(lp, C, B * Q, C))
            r["word_cost_GBps"] = nbytes / r["word_cost_us"] / 1e3                 # one read of the logits
            r["word_loss_bwd_GBps"] = 2 * nbytes / r["word_loss_bwd_us"] / 1e3     # one read, one write
            r["log_softmax_GBps"] = 2 * nbytes / r["log_softmax_us"] / 1e3         # one read, one write (in place)
            res["runs"].append({k: round(v, 1) for k, v in r.items()})
    reference_route(x, cap)
    res["reference_route_us"] = [round(reference_route(x, cap), 1) for _ in range(3)]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
