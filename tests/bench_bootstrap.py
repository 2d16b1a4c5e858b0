"""Tuning aid (a script, not a test): the bootstrap launch beside its two baselines at the size of
an ActivityNet Captions validation run, N = 4917 videos, R = 10000 resamples, for M = 7 and M = 88 columns, with and without
weights.

  a  ops.bootstrap_ratios: one launch
  b  a plain torch-on-device formulation: torch.randint, index_select of the (N, M) rows, a sum over the N draws, in
     chunks of resamples that keep the gathered rows within 256 MiB.  Not the same draws, the same amount of work
  c  evaluate.bootstrap_ratios_host (numpy, the CPU route): timed once per shape with a host clock, it takes seconds

a and b: a warm call, then `reps` calls between two events; in the order a, b and then b, a, twice.  The first thing the
script does is hold a to c bit for bit at the timed sizes (with --host-resamples below R: on c's rows).  Every figure is
reported; the bytes a's workgroups read of values and weights (each workgroup reads its columns once per kRows rows) are
computed from the shapes.  Prints ONE JSON line."""
import argparse, json, os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from bmhrl_amd import ops
from bmhrl_amd.evaluate import bootstrap_ratios_host

N, R = 4917, 10000
GATHER_BYTES = 256 << 20


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps


def torch_formulation(values_t, weights_t, resamples):
    """values_t / weights_t (N, M) on the device -> (resamples, M)"""
    n, m = values_t.shape
    chunk = max(1, GATHER_BYTES // (n * m * 8))
    out = []
    for lo in range(0, resamples, chunk):
        rc = min(chunk, resamples - lo)
        idx = torch.randint(n, (rc * n,), device=values_t.device)
        num = values_t.index_select(0, idx).view(rc, n, m).sum(dim=1)
        if weights_t is None:
            out.append(num / n)
        else:
            out.append(num / weights_t.index_select(0, idx).view(rc, n, m).sum(dim=1))
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-resamples", type=int, default=R, help="resamples of the host baseline (its time is per call)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    res = {"config": {"N": N, "R": R, "reps": args.reps, "host_resamples": args.host_resamples,
                      "rows_per_workgroup": ops.bootstrap_rows(N, R)}, "shapes": {}}
    for M in (7, 88):
        for weighted in (False, True):
            x = rng.uniform(0.0, 1.0, (M, N))
            w = (rng.uniform(size=(M, N)) > 0.1).astype(np.float64) if weighted else None
            xd, wd = torch.from_numpy(x).to(dev), None if w is None else torch.from_numpy(w).to(dev)
            xt, wt = xd.t().contiguous(), None if wd is None else wd.t().contiguous()
            t0 = time.perf_counter()
            host = bootstrap_ratios_host(x, w, args.host_resamples, 0)
            host_s = time.perf_counter() - t0
            got = ops.bootstrap_ratios(xd, wd, R, 0).cpu().numpy()
            equal = bool(np.array_equal(got[:args.host_resamples + 1].view(np.uint64), host.view(np.uint64)))
            calls = {"a_launch_ms": lambda: ops.bootstrap_ratios(xd, wd, R, 0),
                     "b_torch_ms": lambda: torch_formulation(xt, wt, R)}
            runs = []
            for _ in range(2):
                for order in (list(calls), list(calls)[::-1]):
                    runs.append({name: round(timed(calls[name], args.reps), 3) for name in order})
            rows = ops.bootstrap_rows(N, R)                          # of the R + 1 a workgroup carries: it reads its columns once
            read = (R + 1 + rows - 1) // rows * M * N * 8 * (2 if weighted else 1)
            best = min(r["a_launch_ms"] for r in runs)
            res["shapes"][f"M{M}_{'weights' if weighted else 'noweights'}"] = {
                "runs": runs, "c_host_s": round(host_s, 2), "launch_equals_host_bits": equal,
                "bytes_read_by_workgroups": read, "implied_read_GBps_at_best": round(read / best / 1e6, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
