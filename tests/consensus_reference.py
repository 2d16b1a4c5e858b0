"""The consensus rules of bmhrl_amd/decode.py (consensus section, R1-R7) restated with Python loops and numpy float64: the
reference of tests/test_consensus_cpu.py and tests/test_consensus_gpu.py.  It shares no code with decode.py: grams are rows of
an integer array, a clip's distinct grams are numbered by np.unique, a hypothesis' counts come from np.bincount and its
first-occurrence order from the positions np.unique reports.  Every floating-point value is an np.float64 scalar and every sum
an explicit loop in the prescribed order (one product, then one add), so comparisons against it are equalities."""
import numpy as np

F = np.float64
MAX_G = 4


def words(row, end_idx):
    """R1: the tokens of columns 1 .. m before the first end_idx"""
    out = []
    for v in row[1:]:
        if int(v) == end_idx:
            break
        out.append(int(v))
    return out


def gram_weight(gram, w32):
    """R2: fp32 weights widened, added in token order, the division last; ids outside [0, V) weigh 0"""
    if w32 is None:
        return F(1.0)
    V = len(w32)
    s = None
    for v in gram:
        x = F(w32[v]) if 0 <= v < V else F(0.0)
        s = x if s is None else s + x
    return s / F(len(gram))


def clip_terms(clip, end_idx, w32=None):
    """t[g - 1, i, j] = M_g(i, j) / max(W_i^g, W_j^g) (0 where the maximum is 0, and on the diagonal) for g = 1 .. 4 of one
    clip's hypotheses (K, m + 1): R2-R5 up to the sum over g"""
    K = len(clip)
    ws = [words(r, end_idx) for r in clip]
    t = np.zeros((MAX_G, K, K), dtype=F)
    for g in range(1, MAX_G + 1):
        rows = [np.array([w[p:p + g] for p in range(len(w) - g + 1)], dtype=np.int64).reshape(-1, g) for w in ws]
        every = np.concatenate(rows, 0)
        if every.shape[0] == 0:
            continue
        uniq, inv = np.unique(every, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        weight = [gram_weight([int(v) for v in u], w32) for u in uniq]
        counts, firsts, mass, at = [], [], [], 0
        for r in rows:
            ids = inv[at:at + r.shape[0]]
            at += r.shape[0]
            c = np.bincount(ids, minlength=len(uniq))
            seen, pos = np.unique(ids, return_index=True)
            order = [int(s) for s in seen[np.argsort(pos, kind="stable")]]       # distinct grams, first occurrence first
            W = F(0.0)
            for y in order:
                W = W + weight[y] * F(c[y])                                       # R3
            counts.append(c)
            firsts.append(order)
            mass.append(W)
        for i in range(K):
            for j in range(K):
                if i == j:
                    continue
                M = F(0.0)
                for y in firsts[i]:
                    M = M + weight[y] * F(min(counts[i][y], counts[j][y]))        # R4
                mx = max(mass[i], mass[j])
                t[g - 1, i, j] = M / mx if mx > 0 else F(0.0)
    return t


def terms(toks, end_idx, w32=None):
    """clip_terms of every clip of toks (B, K, m + 1): (B, 4, K, K).  Compute once per set of hypotheses; utilities() of any
    N reads it."""
    toks = np.asarray(toks)
    return np.stack([clip_terms(c, end_idx, w32) for c in toks.tolist()]) if len(toks) else np.zeros((0, MAX_G, 0, 0))


def utilities(t, N):
    """R5-R6 from terms(): (U (B, K), u (B, K, K) with a zero diagonal)"""
    B, _, K, _ = t.shape
    u = np.zeros((B, K, K), dtype=F)
    U = np.zeros((B, K), dtype=F)
    for b in range(B):
        for i in range(K):
            total = F(0.0)
            for j in range(K):
                if j == i:
                    continue
                s = F(0.0)
                for g in range(N):
                    s = s + t[b, g, i, j]
                u[b, i, j] = s / F(N)
                total = total + u[b, i, j]
            U[b, i] = total / F(K - 1) if K > 1 else F(0.0)
    return U, u


def choose(U_row, order):
    """R7: the hypothesis of the largest U, ties to the earlier one of `order` (the hypotheses' indices, best first)"""
    best = None
    for k in order:
        if best is None or U_row[k] > U_row[best]:
            best = int(k)
    return best


def logp_order(scores_row):
    """sampling rule 7 / beam rule 5 with length_penalty = 0: the largest score first, ties to the lower index"""
    return sorted(range(len(scores_row)), key=lambda k: (-float(scores_row[k]), k))


def caption(row, end_idx):
    """start token + the words + the end token when there is one: what a returned caption holds before its padding"""
    w = words(row, end_idx)
    return [int(row[0])] + w + ([end_idx] if len(w) < len(row) - 1 else [])
