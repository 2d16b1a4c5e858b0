"""The bootstrap's definition (B1-B4 of bmhrl_bootstrap_ratios, include/bmhrl_hip.h) in plain numpy
loops, written to be read: one resample, one column, one lane at a time, Python floats (IEEE doubles, one rounding per
operation).  Also the cases the CPU and GPU tests share; expected(name) computes a case's statistics once and keeps them."""
import numpy as np

MASK = (1 << 64) - 1


def hash_u32(seed, idx):
    """csrc/common.h's hash_u32 on Python integers"""
    z = (idx * 0x9E3779B97F4A7C15 + seed) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    z = z ^ (z >> 31)
    return z >> 32


def counts(N, r, seed):
    """B1: the counts of row r, a list of N integers"""
    if r == 0:
        return [1] * N
    c = [0] * N
    for j in range(N):
        h = hash_u32(seed, (r << 32) | j)
        c[(h * N) >> 32] += 1
    return c


def lane_sum(c, x):
    """B2 and B3: the 64 lane sums in ascending order of the videos, then the xor butterfly; every lane's final value"""
    N = len(c)
    p = [0.0] * 64
    for t in range(64):
        for i in range(t, N, 64):
            p[t] = p[t] + (float(c[i]) * x[i])
    for s in (32, 16, 8, 4, 2, 1):
        p = [p[t] + p[t ^ s] for t in range(64)]
    return p


def bootstrap_ratios(values, weights, resamples, seed):
    """stats (resamples + 1, M) fp64 of values (M, N), weights (M, N) or None"""
    values = np.asarray(values, dtype=np.float64)
    M, N = values.shape
    stats = np.empty((resamples + 1, M), dtype=np.float64)
    cols = [values[m].tolist() for m in range(M)]
    wcols = None if weights is None else [np.asarray(weights, dtype=np.float64)[m].tolist() for m in range(M)]
    for r in range(resamples + 1):
        c = counts(N, r, seed)
        assert sum(c) == N
        for m in range(M):
            lanes = lane_sum(c, cols[m])
            assert all(np.float64(v).tobytes() == np.float64(lanes[0]).tobytes() for v in lanes)      # B3: equal bits
            if wcols is None:
                stats[r, m] = lanes[0] / float(N)                                                       # B4
            else:
                den = lane_sum(c, wcols[m])[0]
                stats[r, m] = 0.0 if den == 0.0 else lanes[0] / den
    return stats


def case(N, M, R, seed=0, weights=None, rng_seed=0):
    """values of mixed sign; weights None, "some" (positive, a few zeros) or "zero_column" (column M // 2 all zero)"""
    rng = np.random.RandomState(1000 + 7 * N + 3 * M + rng_seed)
    values = rng.standard_normal((M, N)) * np.exp(rng.uniform(-3.0, 3.0, (M, 1)))
    w = None
    if weights is not None:
        w = rng.uniform(0.5, 2.0, (M, N)) * (rng.uniform(size=(M, N)) > 0.2)
        if weights == "zero_column":
            w[M // 2] = 0.0
    return dict(values=np.ascontiguousarray(values), weights=w, R=R, seed=seed)


BIG_SEED = (1 << 40) + 12345                  # above 2^32
COLUMN_BLOCK = 128                            # csrc/bootstrap.hip's kColBlock: the columns of one workgroup


def cases():
    out = {}
    # N at the stride edges, the rows-per-workgroup thresholds of the entry point (2560 / 5120) and the limit; R = 1, 2, 300;
    # M = 1, 3, 4, 5 (a wave per column, four waves) and one above the column block
    for N, M, R, seed, weights in [
            (1, 1, 2, 0, None), (2, 3, 1, BIG_SEED, "some"), (63, 4, 2, 0, "zero_column"), (64, 5, 300, BIG_SEED, None),
            (65, 3, 300, 0, "some"), (255, 1, 2, BIG_SEED, "zero_column"), (256, 4, 1, 0, None), (257, 5, 2, 0, "some"),
            (65, COLUMN_BLOCK + 2, 2, BIG_SEED, "zero_column"), (2560, 3, 5, 0, None), (2561, 3, 5, 0, "some"),
            (4097, 1, 2, BIG_SEED, "some"), (5121, 2, 2, 0, None), (16384, 2, 2, 0, "zero_column"), (16384, 3, 1, BIG_SEED, None)]:
        out[f"N{N}_M{M}_R{R}_{'big' if seed else 'zero'}seed_{weights or 'noweights'}"] = case(N, M, R, seed, weights)
    return out


CASES = cases()
_EXPECTED = {}


def expected(name):
    if name not in _EXPECTED:
        c = CASES[name]
        stats = bootstrap_ratios(c["values"], c["weights"], c["R"], c["seed"])
        stats.setflags(write=False)
        _EXPECTED[name] = stats
    return _EXPECTED[name]
