"""Tuning aid (a script, not a test): the proposal post-processing and the head loss at the size of a full model --
B = 16 videos, N = 16 * 128 * 300 + 13 * 48 * 800 candidates per video, k = 100, nms_tiou = 0.4.

  select   ops.proposal_select (a fixed number of launches, no host read) against the piecewise torch route of
           bmhrl_amd.proposal_utils on the same device: argsort + gather + corners + trim, then greedy NMS per video in a
           Python loop that indexes with a boolean tensor, i.e. synchronises with the host in every iteration.  The device
           route is timed as graphs of repeated launches between two events after a warm replay; the torch route cannot be
           captured (it reads back), so it is timed eagerly between synchronisations, and its graphable top-k half alone too.
  head     ops.proposal_head (decode + four-term loss + d total / d x, one launch) for one video head (B = 16, S = 300,
           A = 128) against the same loss written in torch ops with autograd's backward, both as graphs.
Prints ONE JSON line."""
import json, os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from types import SimpleNamespace
from bmhrl_amd import ops, proposal_utils as pu

B, K, NMS = 16, 100, 0.4
N = 16 * 128 * 300 + 13 * 48 * 800
DUR = 120.0


def timed(fn, reps=5, rounds=5):
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


def torch_route(pred, cfg, batch):
    post = pu.postprocess_preds(pred, cfg, batch)
    return [pu.non_max_suppresion(v, cfg.nms_tiou_thresh) for v in post]


def torch_head_loss(x, anchors, cell_sec, owner, tx, tw, obj_coeff, noobj_coeff):
    Bn, S, A3 = x.shape
    A = A3 // 3
    v = x.view(Bn, S, A, 3).permute(0, 2, 1, 3)
    c, l, o = v[..., 0], v[..., 1], v[..., 2]
    sc = torch.sigmoid(c)
    pos = torch.arange(S, dtype=x.dtype, device=x.device).view(1, 1, S)
    pred = torch.stack([(sc + pos) * cell_sec, anchors.view(1, A, 1) * torch.exp(l), torch.sigmoid(o)], dim=-1).reshape(Bn, A * S, 3)
    own = owner >= 0
    idx = owner.clamp(min=0).long()
    n_obj, n_noobj = own.sum().clamp(min=1), (~own).sum().clamp(min=1)
    sp = torch.nn.functional.softplus
    lx = (((sc - tx[idx]) ** 2) * own).sum() / n_obj
    lw = (((l - tw[idx]) ** 2) * own).sum() / n_obj
    lo = (sp(-o) * own).sum() / n_obj
    ln = (sp(o) * ~own).sum() / n_noobj
    return pred, lx + lw + obj_coeff * lo + noobj_coeff * ln


def main():
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cpu").manual_seed(0)
    pred = torch.stack([torch.rand(B, N, generator=gen) * DUR, torch.rand(B, N, generator=gen) * 59.5 + 0.5,
                        torch.rand(B, N, generator=gen)], dim=-1).to(dev)
    durations = [DUR - b for b in range(B)]
    dur = torch.tensor(durations, dtype=torch.float32, device=dev)
    cfg = SimpleNamespace(max_prop_per_vid=K, nms_tiou_thresh=NMS)
    batch = {"duration_in_secs": durations}
    batch_dev = {"duration_in_secs": dur}                    # (a capture cannot hold the upload of a Python list)
    res = {"config": {"B": B, "N": N, "k": K, "nms_tiou": NMS}, "runs": []}

    props, count = ops.proposal_select(pred, dur, K, NMS)
    want = torch_route(pred, cfg, batch)
    same = all(int(count[b]) == len(want[b]) and torch.equal(props[b, :len(want[b])], want[b]) for b in range(B))
    res["device_equals_torch_route"] = bool(same)           # (random confidences: ties are not expected)
    res["survivors_per_video"] = round(float(count.float().mean()), 1)

    S, A, cell = 300, 128, 0.64
    x = torch.randn(B, S, 3 * A, generator=gen).to(dev)
    anchors = (torch.rand(A, generator=gen) * 100 + 0.5).sort().values.to(dev)
    targets = torch.stack([torch.randint(0, B, (64,), generator=gen).float(), torch.rand(64, generator=gen) * S * cell,
                           torch.rand(64, generator=gen) * 80 + 1, torch.zeros(64)], dim=1).to(dev)
    assigned = ops.proposal_assign(targets, anchors, cell, B, S)
    owner, tx, tw, counts = assigned
    out = torch.empty(B, A * S, 3, device=dev)
    dx, sums = torch.empty_like(x), torch.empty(5, device=dev)
    xg = x.clone().requires_grad_(True)

    def torch_head():
        xg.grad = None
        torch_head_loss(xg, anchors, cell, owner, tx, tw, 1.0, 100.0)[1].backward()

    for run in range(2):
        r = {}
        r["select_device_us"] = round(timed(lambda: ops.proposal_select(pred, dur, K, NMS)), 1)
        r["select_torch_topk_only_us"] = round(timed(lambda: pu.postprocess_preds(pred, cfg, batch_dev)), 1)
        torch_route(pred, cfg, batch); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            torch_route(pred, cfg, batch)
        torch.cuda.synchronize()
        r["select_torch_route_us"] = round((time.perf_counter() - t0) / 3 * 1e6, 1)
        r["assign_us"] = round(timed(lambda: ops.proposal_assign(targets, anchors, cell, B, S), reps=20), 1)
        r["head_device_us"] = round(timed(lambda: ops.proposal_head(x, anchors, cell, out, 0, assigned, 1.0, 100.0, sums=sums, dx=dx),
                                          reps=20), 1)
        r["head_torch_us"] = round(timed(torch_head, reps=5), 1)
        res["runs"].append(r)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
