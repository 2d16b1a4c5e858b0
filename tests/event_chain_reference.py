"""The restatement bmhrl_proposal_chain and proposal_utils.event_chain are tested against: numpy
float32, a loop over the levels and the positions with a first-maximum argmax per (level, position), no torch and none of
the package's code.

`chain_select` is the definition for a batch, `link_tables` the fp32 tIoU / link tables of one video that the exhaustive
check of tests/test_event_chain_cpu.py enumerates over.  `cases()` are the inputs the CPU and the GPU tests share,
`expected(name)` a case's restated result (computed once).
"""
import functools

import numpy as np

f = np.float32
NEG = f(-np.inf)


def tiou_with(s1, e1, s2, e2):
    inter = np.maximum(np.minimum(e1, e2) - np.maximum(s1, s2), f(0))
    union = (e1 - s1) + (e2 - s2) - inter
    union = np.minimum(np.maximum(e1, e2) - np.minimum(s1, s2), union)
    return inter / (union + f(1e-8))


def eligible_in_order(rows, count, event_cost, min_length):
    """the eligible rows' indices in (start, end, index) order, and their gains"""
    rows = np.asarray(rows, dtype=np.float32)
    s, e, score = rows[:, 0], rows[:, 1], rows[:, 2]
    with np.errstate(invalid="ignore"):
        g = score - f(event_cost)
        ok = (np.arange(len(rows)) < count) & ((e - s) > f(min_length)) & (score == score) & (g > f(0))
    idx = np.nonzero(ok)[0]
    idx = idx[np.lexsort((idx, e[idx], s[idx]))]            # the last key is the primary one; float comparisons
    return idx, g[idx]


def link_tables(rows, idx, max_tiou):
    """(t, allowed) over the positions: t[i, j] the fp32 tIoU, allowed[i, j] the link i -> j"""
    s, e = rows[idx, 0], rows[idx, 1]
    n = len(idx)
    with np.errstate(invalid="ignore"):
        t = tiou_with(s[:, None], e[:, None], s[None, :], e[None, :])
        allowed = (np.arange(n)[:, None] < np.arange(n)[None, :]) & (e[:, None] <= e[None, :]) & (t <= f(max_tiou))
    assert t.dtype == np.float32
    return t, allowed


def chain_of(rows, count, L, max_tiou, overlap_weight, event_cost, min_length):
    """one video: (chosen row indices in time order, value)"""
    rows = np.asarray(rows, dtype=np.float32)
    idx, g = eligible_in_order(rows, count, event_cost, min_length)
    n = len(idx)
    if n == 0:
        return [], f(0)
    t, allowed = link_tables(rows, idx, max_tiou)
    lam = f(overlap_weight)
    V = np.full((L + 1, n), NEG, dtype=np.float32)          # -inf: undefined
    parent = np.full((L + 1, n), -1, dtype=np.int64)
    V[1] = g
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(2, L + 1):
            for j in range(1, n):
                cand = (V[l - 1, :j] - (lam * t[:j, j])) + g[j]
                assert cand.dtype == np.float32
                cand = np.where(allowed[:j, j] & (V[l - 1, :j] > NEG) & (cand > NEG), cand, NEG)    # (NaN > -inf is False)
                i = int(np.argmax(cand))                    # the first of the maxima
                if cand[i] > NEG:
                    V[l, j], parent[l, j] = cand[i], i
            if not (V[l] > NEG).any():
                break
    best = V[1:].max()
    l, j = [(int(a) + 1, int(b)) for a, b in zip(*np.nonzero(V[1:] == best))][0]      # row-major: smaller l, then earlier j
    value, picked = V[l, j], []
    while l >= 1:
        picked.append(int(idx[j]))
        j, l = parent[l, j], l - 1
    return picked[::-1], value


def chain_select(props, count, L, max_tiou=0.0, overlap_weight=0.0, event_cost=0.0, min_length=0.2):
    """props (B, P, 3) float32, count (B) or None.  Returns events (B, L, 3) float32, chain (B, L) int32, length (B) int32
    and value (B) float32."""
    props = np.asarray(props, dtype=np.float32)
    B, P, _ = props.shape
    events = np.zeros((B, L, 3), dtype=np.float32)
    chain = np.full((B, L), -1, dtype=np.int32)
    length = np.zeros(B, dtype=np.int32)
    value = np.zeros(B, dtype=np.float32)
    for b in range(B):
        cnt = P if count is None else min(max(int(count[b]), 0), P)
        picked, value[b] = chain_of(props[b], cnt, L, max_tiou, overlap_weight, event_cost, min_length)
        length[b] = len(picked)
        chain[b, :len(picked)] = picked
        events[b, :len(picked)] = props[b, picked]
    return events, chain, length, value


# ------------------------------------------------------------------------------------------------ the shared cases
def random_props(rng, B, P, dur=60.0, longest=12.0, grid=None):
    """(B, P, 3) rows (start, end, score): lengths from 0.05 s (some below min_length) to `longest`, scores in (0, 1); with
    `grid` the times are multiples of it (exact ties of starts and ends)"""
    start = rng.uniform(0.0, dur - 1.0, (B, P))
    length = rng.uniform(0.05, longest, (B, P))
    if grid:
        start, length = np.round(start / grid) * grid, np.maximum(np.round(length / grid), 1) * grid
    props = np.stack([start, np.minimum(start + length, dur), rng.uniform(0.01, 1.0, (B, P))], axis=2)
    return props.astype(np.float32)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(props, count, L, max_tiou, overlap_weight, event_cost, min_length): the smallest shapes at which each
    mechanism of the kernel can break (see tests/test_event_chain_gpu.py)"""
    rng = np.random.default_rng(2036)
    out = {}

    def add(name, props, count, L, tau=0.0, lam=0.0, cost=0.0, min_length=0.2):
        assert name not in out
        out[name] = dict(props=np.ascontiguousarray(props, dtype=np.float32),
                         count=None if count is None else np.asarray(count, dtype=np.int32), L=L, max_tiou=tau,
                         overlap_weight=lam, event_cost=cost, min_length=min_length)

    for P in (1, 2, 3):
        add(f"P={P}", random_props(rng, 2, P, dur=20.0, longest=4.0), None, 4, tau=0.3, lam=0.2)
    for P in (64, 65):                                      # the wave edge
        add(f"P={P} tau 0.5 lambda 0.3", random_props(rng, 2, P), None, 10, tau=0.5, lam=0.3, cost=0.05)
        add(f"P={P} tau 0", random_props(rng, 2, P), None, 10)
    for P in (512, 513):                                    # a thread's second row
        add(f"P={P}", random_props(rng, 2, P, dur=120.0), None, 12, tau=0.1, lam=0.5, cost=0.05)
    p = random_props(rng, 1, 1023, dur=200.0)
    add("P=1023 L=32", p, None, 32, tau=0.2, lam=0.4, cost=0.3)
    p = random_props(rng, 2, 1024, dur=200.0)
    add("P=1024 L=32", p, None, 32, tau=0.5, lam=0.3, cost=0.1)
    add("P=1024 L=1", p, None, 1)
    p = random_props(rng, 3, 100)
    add("count 0", p, [0, 0, 0], 5)
    garbage = p.copy()
    garbage[:, 40:] = rng.uniform(-5.0, 90.0, (3, 60, 3)).astype(np.float32)
    garbage[:, 40:, :][:, ::3, 2] = np.nan
    garbage[:, 41::7, 0] = np.nan
    add("garbage and NaN behind count", garbage, [40, 40, 40], 8, tau=0.1, lam=0.5)
    add("count NULL", p, None, 10, tau=0.1, lam=0.5, cost=0.05)
    per_video = p.copy()
    per_video[1, :, 2] = 0.04                               # nothing eligible in the second video: every score below the cost
    add("per-video counts", per_video, [100, 57, 3], 10, tau=0.1, lam=0.5, cost=0.05)
    add("counts outside [0, P]", p, [-7, 1000, 50], 6, tau=0.1)
    add("L above the eligible rows", random_props(rng, 2, 6, dur=100.0, longest=3.0), None, 32, tau=0.5)
    q = random_props(rng, 2, 80)
    q[:, :, 2] = 0.25
    add("equal scores", q, None, 8, tau=0.1, lam=0.5)
    q = random_props(rng, 2, 30)
    add("exact duplicates", np.repeat(q, 3, axis=1), None, 10, tau=0.1, lam=0.5)
    add("exact duplicates tau 1", np.repeat(q, 3, axis=1), None, 10, tau=1.0)
    g = random_props(rng, 2, 120, dur=30.0, longest=6.0, grid=0.5)
    add("equal starts, different ends", g, None, 10, tau=0.2, lam=0.25)
    add("equal starts, scores on a grid", np.concatenate([g[:, :, :2], np.round(g[:, :, 2:] * 8) / 8 + 0.125], axis=2), None, 10,
        tau=0.2)
    touch = np.zeros((2, 40, 3), dtype=np.float32)          # back-to-back segments on a 1.5 s grid, each in two copies
    edges = (np.arange(21) * 1.5).astype(np.float32)
    touch[:, :, 0] = np.repeat(edges[:20], 2)[rng.permutation(40)]
    touch[:, :, 1] = touch[:, :, 0] + np.float32(1.5)
    touch[:, :, 2] = rng.uniform(0.1, 1.0, (2, 40))
    add("tau 0, touching segments", touch, None, 32)
    nested = np.zeros((1, 12, 3), dtype=np.float32)         # row i = [i, 30 - i]: every later start has an earlier end
    nested[0, :, 0] = np.arange(12)
    nested[0, :, 1] = 30 - np.arange(12)
    nested[0, :, 2] = rng.uniform(0.2, 0.9, 12)
    add("nested segments never link", nested, None, 5, tau=1.0)
    add("cost above every score", p, None, 10, tau=0.1, cost=1.5)
    nan_score = p.copy()
    nan_score[:, ::2, 2] = np.nan
    add("NaN scores", nan_score, None, 10, tau=0.1, lam=0.5)
    add("every row shorter than min_length", p, None, 10, tau=0.1, min_length=20.0)
    add("min_length 0", p, None, 10, tau=0.1, lam=0.5, min_length=0.0)
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """(events, chain, length, value) of case `name`"""
    c = cases()[name]
    return chain_select(c["props"], c["count"], c["L"], c["max_tiou"], c["overlap_weight"], c["event_cost"], c["min_length"])
