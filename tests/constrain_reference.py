"""The constraint rules of bmhrl_amd/decode.py (constraints section, rules 1-3) restated in numpy with plain Python loops:
the reference of tests/test_constrain_cpu.py and tests/test_constrain_gpu.py.  The results are bit-exact (-inf stores and one
fp32 multiply per id), so every comparison against it is an equality."""
import numpy as np


def apply_rules(lp, hist, t, ngram, min_len, penalty, end_idx, pad_idx):
    """lp (R, V) float32, hist (R, >= t + 1) integer sequences -> the adjusted copy of lp"""
    lp = np.array(lp, dtype=np.float32, copy=True)
    R, V = lp.shape
    theta = np.float32(penalty)
    for r in range(R):
        s = [int(v) for v in hist[r][:t + 1]]
        if theta != np.float32(1):
            for v in sorted(set(s)):
                if v != pad_idx:
                    lp[r, v] = np.float32(lp[r, v]) * theta
        if ngram >= 1 and t + 1 >= ngram:
            last = s[t - ngram + 2:t + 1]
            for j in range(0, t + 1 - ngram + 1):
                if s[j:j + ngram - 1] == last:
                    lp[r, s[j + ngram - 1]] = -np.inf
        if t < min_len:
            lp[r, end_idx] = -np.inf
    return lp


def repeats_ngram(tokens, n):
    """does the token list contain the same n-gram twice?"""
    seen = set()
    for j in range(len(tokens) - n + 1):
        g = tuple(tokens[j:j + n])
        if g in seen:
            return True
        seen.add(g)
    return False


def upto_end(row, end_idx):
    """the tokens of a hypothesis (start token included) up to and including its first end_idx"""
    row = [int(v) for v in row]
    return row[:row.index(end_idx, 1) + 1] if end_idx in row[1:] else row


def case_table():
    """(name, hist rows, t, ngram, min_len, penalty) over vocabulary 7 with pad 1 and end 6: histories with many repeats"""
    rng = np.random.RandomState(0)
    cases = []
    for t in range(12):
        hist = rng.randint(0, 7, size=(3, 12))
        hist[:, 0] = 2
        for n in (0, 1, 2, 3, 4):                         # t + 1 < n, == n and > n all occur over t = 0 .. 11
            for theta in (1.0, 1.3, 0.7):
                cases.append((f"random t={t} n={n} theta={theta}", hist, t, n, 0, theta))
    # the same bigram / trigram several times with different followers, and a follower that is also penalised
    h = np.array([[2, 3, 4, 5, 3, 4, 0, 3, 4, 3, 4, 6], [2, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5, 5], [2, 3, 4, 2, 3, 5, 2, 3, 0, 2, 3, 4]])
    for t in (8, 10, 11):
        for n in (2, 3):
            for theta in (1.0, 1.3):
                cases.append((f"followers t={t} n={n} theta={theta}", h, t, n, 0, theta))
    # pad in the history is not penalised (but takes part in the n-grams)
    h = np.array([[2, 3, 6, 1, 1, 1, 1, 1, 1, 1, 1, 1], [2, 1, 3, 1, 3, 1, 3, 1, 3, 1, 3, 1], [2, 4, 4, 6, 1, 1, 1, 1, 1, 1, 1, 1]])
    for t in (3, 5, 9):
        for n in (0, 2):
            cases.append((f"pad t={t} n={n}", h, t, n, 0, 1.3))
    # minimum length at t = m - 1 (banned) and t = m (free), alone and with the other rules
    for m, t in ((1, 0), (1, 1), (5, 4), (5, 5), (11, 10), (11, 11)):
        cases.append((f"min_len m={m} t={t}", h, t, 0, m, 1.0))
        cases.append((f"min_len m={m} t={t} with n=2 theta=0.7", h, t, 2, m, 0.7))
    return cases
