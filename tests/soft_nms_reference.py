"""The restatement bmhrl_proposal_select_soft and proposal_utils.soft_nms are tested against: numpy
float32 and math.exp, a loop over the picks, no torch and none of the package's code.

Besides the outputs a run reports `well_conditioned`: every Gaussian weight w (a float64) it used rounds to the same float32
as w * (1 + 2^-50) and w * (1 - 2^-50).  exp on the host and on the device are both within 1 ulp (2^-52 relative) of the true
value, so under this condition they cannot round to different float32 weights and equal bits can be demanded of both.  It
is a condition on the inputs of a case, not a tolerance; the cases below all satisfy it (asserted in
tests/test_soft_nms_cpu.py).

`cases()` are the inputs the CPU and the GPU tests share, `expected(name)` a case's restated result (computed once).
"""
import functools
import math

import numpy as np

f = np.float32
METHODS = ("hard", "linear", "gaussian")
EPS = 2.0 ** -50


def order_image(x):
    """float32 array -> int64 whose order is the floats' (negative below positive, -0.0 below +0.0)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.int64)
    return np.where(u >= 0x80000000, 0xFFFFFFFF - u, u + 0x80000000)


def pool_of(pred_b, dur, m):
    """the m rows of highest confidence, ties to the smaller row: (rows, start, end, score), corners trimmed in fp32"""
    n = pred_b.shape[0]
    order = np.lexsort((np.arange(n), -order_image(pred_b[:, 2])))[:m]
    centre, length = pred_b[order, 0], pred_b[order, 1]
    start, end = centre - length / f(2), centre + length / f(2)
    start = np.minimum(np.maximum(start, f(0)), dur)
    end = np.minimum(end, dur)
    return order, start, end, pred_b[order, 2].copy()


def tiou_with(s1, e1, s2, e2):
    inter = np.maximum(np.minimum(e1, e2) - np.maximum(s1, s2), f(0))
    union = (e1 - s1) + (e2 - s2) - inter
    union = np.minimum(np.maximum(e1, e2) - np.minimum(s1, s2), union)
    return inter / (union + f(1e-8))


@functools.lru_cache(maxsize=None)
def gaussian_weight(t, sigma):
    """(float32 weight, well conditioned) for one fp32 tIoU t and the fp32 sigma, both given as Python floats"""
    w = math.exp(-(t * t) / sigma)
    w32 = f(w)
    return w32, bool(f(w * (1 + EPS)) == w32 and f(w * (1 - EPS)) == w32)


def soft_select(pred, durations, m, k, method, tiou_thresh=0.0, sigma=0.5, min_score=None):
    """pred (B, N, 3) float32, durations (B).  Returns props (B, k, 3) float32, rows (B, k) int32, count (B) int32 and
    well_conditioned (bool)."""
    assert method in METHODS
    pred = np.asarray(pred, dtype=np.float32)
    B, N, _ = pred.shape
    props = np.zeros((B, k, 3), dtype=np.float32)
    rows = np.full((B, k), -1, dtype=np.int32)
    count = np.zeros(B, dtype=np.int32)
    thr = f(tiou_thresh)
    well = True
    for b in range(B):
        order, start, end, score = pool_of(pred[b], f(durations[b]), min(m, N))
        assert score.dtype == start.dtype == end.dtype == np.float32
        alive = np.ones(len(order), dtype=bool)
        for _ in range(k):
            if not alive.any():
                break
            image = np.where(alive, order_image(score), -1)
            i = int(np.argmax(image))                       # the first of the maxima: the smaller rank
            if min_score is not None and score[i] < f(min_score):
                break
            props[b, count[b]] = (start[i], end[i], score[i])
            rows[b, count[b]] = order[i]
            count[b] += 1
            alive[i] = False
            t = tiou_with(start[i], end[i], start, end)
            assert t.dtype == np.float32
            hit = alive & ~(t < thr)
            if method == "hard":
                alive &= ~hit
            elif method == "linear":
                score = np.where(hit, score * (f(1) - t), score)
            else:
                used = [gaussian_weight(x, float(f(sigma))) for x in t[hit].tolist()]
                well = well and all(ok for _, ok in used)
                score[hit] = score[hit] * np.array([w32 for w32, _ in used], dtype=np.float32)
    return props, rows, count, well


# ------------------------------------------------------------------------------------------------ the shared cases
D3 = [50.0, 31.7, 3.0]                  # the third so short that most trimmed segments are empty (start == end == duration)


def random_pred(rng, B, N, dur=50.0, conf=(0.0, 1.0)):
    pred = np.empty((B, N, 3), dtype=np.float32)
    pred[:, :, 0] = rng.uniform(-2.0, dur + 2.0, (B, N))
    pred[:, :, 1] = rng.uniform(0.1, dur / 3, (B, N))
    pred[:, :, 2] = rng.uniform(conf[0], conf[1], (B, N))
    return pred


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(pred, durations, m, k, method, tiou_thresh, sigma, min_score): the smallest shapes at which each
    mechanism of the kernel can break (see tests/test_soft_nms_gpu.py), every method, thresholds 0 and 0.5"""
    rng = np.random.default_rng(2017)
    out = {}

    def add(name, pred, m, k, method, thr, sigma=0.5, min_score=1e-3):
        assert name not in out
        out[name] = dict(pred=pred, durations=D3[:pred.shape[0]], m=m, k=k, method=method, tiou_thresh=thr, sigma=sigma,
                         min_score=min_score)

    p = random_pred(rng, 1, 1)
    for method in METHODS:
        add(f"N=1 {method}", p, 1, 1, method, 0.0)
    p = random_pred(rng, 3, 3)
    add("N=3 gaussian thr 0", p, 3, 3, "gaussian", 0.0)
    add("N=3 linear thr 0.5", p, 3, 2, "linear", 0.5)
    add("N=3 hard thr 0.5", p, 3, 3, "hard", 0.5, min_score=None)
    for N in (64, 65):                                      # the wave edge of the pool
        p = random_pred(rng, 2, N)
        add(f"N={N} gaussian thr 0", p, N, N, "gaussian", 0.0)
        add(f"N={N} linear thr 0.5", p, N, N, "linear", 0.5)
    for N in (4096, 4097):                                  # the chunk edge: 4097 is the first case with a pass
        p = random_pred(rng, 2, N)
        add(f"N={N} gaussian thr 0", p, 256, 100, "gaussian", 0.0)
        add(f"N={N} linear thr 0", p, 256, 100, "linear", 0.0)
    p = random_pred(rng, 2, 2 * 4096 + 5)                   # passes that keep more than 128 keys per chunk
    add("N=8197 m=1024 gaussian thr 0", p, 1024, 128, "gaussian", 0.0)
    add("N=8197 m=1024 linear thr 0.5", p, 1024, 128, "linear", 0.5)
    add("N=8197 m=1024 hard thr 0.5", p, 1024, 128, "hard", 0.5, min_score=None)
    p = random_pred(rng, 3, 1500)                           # a ragged second row per thread; three durations
    add("m=513 gaussian thr 0.5 sigma 0.3", p, 513, 100, "gaussian", 0.5, sigma=0.3)
    add("m=1023 linear thr 0", p, 1023, 100, "linear", 0.0)
    add("m=1023 gaussian thr 0", p, 1023, 60, "gaussian", 0.0)
    p = random_pred(rng, 2, 300)
    add("k < count", p, 200, 10, "hard", 0.5, min_score=None)
    add("k > survivors", p, 200, 200, "hard", 0.3, min_score=None)
    add("no floor", p, 100, 100, "gaussian", 0.0, min_score=None)
    add("all below the floor", random_pred(rng, 3, 300, conf=(0.0, 0.5)), 200, 50, "linear", 0.5, min_score=0.75)
    add("negative confidences, no floor", random_pred(rng, 2, 300, conf=(-1.0, 1.0)), 128, 128, "linear", 0.5, min_score=None)
    p = random_pred(rng, 2, 300)
    p[:, :, 2] = 0.25
    add("equal confidences gaussian thr 0.5", p, 200, 50, "gaussian", 0.5)
    add("equal confidences linear thr 0", p, 200, 50, "linear", 0.0)
    q = random_pred(rng, 2, 40)
    q[:, :, 0] = rng.uniform(5.0, 25.0, (2, 40))            # inside every duration but the 3 s one is not used: B = 2
    q[:, :, 1] = rng.uniform(1.0, 8.0, (2, 40))             # lengths >= 1 s: tIoU of a segment with its copy is exactly 1
    add("exact duplicates linear", np.repeat(q, 4, axis=1), 160, 160, "linear", 0.5)
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """(props, rows, count, well_conditioned) of case `name`"""
    c = cases()[name]
    return soft_select(c["pred"], c["durations"], c["m"], c["k"], c["method"], c["tiou_thresh"], c["sigma"], c["min_score"])
