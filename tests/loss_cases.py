"""Inputs of the loss-tail tests, built once on the CPU and shared by tests/test_loss_reference_cpu.py (which proves that every
row is the case its name says, in float64) and tests/test_loss_paths_gpu.py (which runs them).  Nothing here touches the
package under test."""
import functools

import torch

from tests import loss_reference as R

# the special-row table: one row per name, all present at once.  `variant` "row0": the only padded row is row 0 (the original's
# index-sum guard leaves it as it is); "later": row 0 and the last row are padded (the guard zeroes both).
SPECIAL_ROWS = ("t_pad_row0", "a_eq_t", "a_eq_pad", "raw_neg", "raw_gt1", "score0", "raw_eq1", "ordinary", "inside", "last")
VARIANTS = ("row0", "later")


@functools.lru_cache(maxsize=None)
def special_case(V, pad, variant):
    """float32 log-probs (rows, V), trg, sampled token a, score, n_row.  Targets and sampled tokens avoid each other and both
    pads (0 and 1) except where the row's name says otherwise; the raw amplitude score p(a) n_row is placed by the score."""
    assert V >= 7 and pad in (0, 1) and variant in VARIANTS
    g = torch.Generator().manual_seed(100 * V + 10 * pad + VARIANTS.index(variant))
    rows, half = len(SPECIAL_ROWS), (V - 2) // 2
    logp = torch.log_softmax(2 * torch.randn(rows, V, generator=g, dtype=torch.float64), -1).float()
    trg = torch.randint(2, 2 + half, (rows,), generator=g)
    a = torch.randint(2 + half, V, (rows,), generator=g)
    i = {n: k for k, n in enumerate(SPECIAL_ROWS)}
    trg[i["t_pad_row0"]] = pad
    a[i["a_eq_t"]] = trg[i["a_eq_t"]]
    a[i["a_eq_pad"]] = pad
    if variant == "row0":
        a[i["t_pad_row0"]] = pad                                   # t == pad with a == pad, not zeroed
    else:
        trg[i["last"]] = pad
        a[i["last"]] = pad                                         # t == pad with a == pad, zeroed
    # raw == 1.0 exactly: p(a) = 2^0 -- the log-prob of the sampled token is 0.0, set by hand behind the softmax (the KL
    # kernels take logp as given), the rest of the row 40 nats down -- times score 0.25 times n_row 4
    r1 = i["raw_eq1"]
    logp[r1] -= 40.0
    logp[r1, a[r1]] = 0.0
    n_row = torch.randint(3, 9, (rows,), generator=g).float()
    n_row[r1] = 4.0
    p_a = torch.exp(torch.gather(logp.double(), 1, a[:, None]).squeeze(1))
    want_raw = torch.full((rows,), 0.4, dtype=torch.float64)       # inside (0, 1) unless the name says otherwise
    want_raw[i["raw_neg"]] = -0.5
    want_raw[i["raw_gt1"]] = 3.0
    score = (want_raw / (p_a * n_row.double())).float()
    score[i["score0"]] = 0.0
    score[r1] = 0.25
    score[i["ordinary"]] = float(torch.rand((), generator=g))       # a reward in (0, 1): a small amplitude
    return dict(V=V, pad=pad, variant=variant, logp=logp, trg=trg, a=a, score=score, n_row=n_row, index=i)


# ---- the sampler: 64 rows of log_softmax(2 randn).  SAMPLER_SEEDS[(V, row_offset)] is the effective seed (seed + the device
# word), chosen so that at least 90 % of the rows are decided (tests/loss_reference.py sampler_rows)
SAMPLER_V = (9, 256, 257, 1000, 10172)
SAMPLER_ROWS = 64
SAMPLER_DEV_WORD = 77777
SAMPLER_SEEDS = {(V, off): 100000 for V in (9, 256, 257, 1000) for off in (0, 1000)}
SAMPLER_SEEDS.update({(1000, 1000): 100001, (10172, 0): 112087, (10172, 1000): 106917})   # (about 80 % at a seed taken blindly)


@functools.lru_cache(maxsize=None)
def sampler_logp(V):
    g = torch.Generator().manual_seed(V)
    return torch.log_softmax(2 * torch.randn(SAMPLER_ROWS, V, generator=g, dtype=torch.float64), -1).float()


@functools.lru_cache(maxsize=None)
def sampler_case(V, row_offset):
    """-> float32 logp (64, V), effective seed, the rows of loss_reference.sampler_rows"""
    lp = sampler_logp(V)
    seed = SAMPLER_SEEDS[(V, row_offset)]
    return lp, seed, R.sampler_rows(lp.double(), seed, row_offset)


def greedy_logp(V):
    """rows with duplicated maxima: in two different threads' chunks, inside one chunk, in the last column and the first, and a
    row of equal entries; 256 threads own ceil(V / 256) consecutive columns each"""
    g = torch.Generator().manual_seed(3 * V)
    chunk = (V + 255) // 256
    lp = torch.randn(6, V, generator=g) - 5.0
    first, other = 1 * chunk, min(V - 1, 5 * chunk)                # first columns of two different chunks
    lp[0, other] = lp[0, first] = 1.0
    lp[1, first + chunk - 1] = lp[1, first] = 1.0                  # both in one chunk (the same column when chunk == 1)
    lp[2, V - 1] = 1.0
    lp[3, V - 1] = lp[3, 0] = 1.0
    lp[4] = -2.0
    want = [first, first, V - 1, 0, 0, int(lp[5].argmax())]
    return lp, want, chunk


# ---- REINFORCE: p(a) below the clamp, on its lower bound, inside, on its upper bound and above
def reinforce_case(V=9, rows=7):
    g = torch.Generator().manual_seed(17)
    probs = torch.softmax(torch.randn(rows, V, generator=g), -1)
    action = torch.randint(0, V, (rows,), generator=g)
    lo, hi = torch.tensor(1e-5, dtype=torch.float32), torch.tensor(1.0, dtype=torch.float32) - torch.tensor(1e-5, dtype=torch.float32)
    placed = {0: 1e-6, 1: float(lo), 2: 0.3, 3: float(hi), 4: 1.0 - 1e-6}
    for r, v in placed.items():
        probs[r, action[r]] = v
    value = torch.rand(rows, generator=g)
    critic = torch.rand(rows, generator=g)
    return dict(V=V, rows=rows, probs=probs, action=action, value=value, critic=critic, below=0, lower=1, inside=2, upper=3, above=4)
