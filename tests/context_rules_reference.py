"""The context rules of bmhrl_amd/decode.py (constraints section, rules C1-C3) restated in numpy with plain Python loops, on
top of tests/constrain_reference.py's rules 1-3: the reference of tests/test_context_rules_cpu.py and
tests/test_context_rules_gpu.py.  The results are bit-exact (-inf stores and at most two fp32 multiplies per entry in a fixed
order), so every comparison against it is an equality on the uint32 view."""
import numpy as np

from tests.constrain_reference import apply_rules

PAD, START, END = 1, 2, 6
V37 = 37


def is_word(v, V, pad_idx):
    return 0 <= v < V and v != pad_idx


def apply_context_rules(lp, hist, t, ngram, min_len, penalty, end_idx, pad_idx, ctx, rows_per_ctx, ctx_ngram, ctx_penalty):
    """lp (R, V) float32, hist (R, >= t + 1) sequences, ctx (R / rows_per_ctx, C) contexts -> the adjusted copy of lp: rules
    1, C1, 2, C2, 3 in this order"""
    lp = apply_rules(lp, hist, t, 0, 0, penalty, end_idx, pad_idx)                      # rule 1
    R, V = lp.shape
    theta_c = np.float32(ctx_penalty)
    rows = [[int(v) for v in ctx[r // rows_per_ctx]] for r in range(R)]
    if theta_c != np.float32(1):                                                        # C1
        for r in range(R):
            for v in sorted(set(rows[r])):
                if is_word(v, V, pad_idx):
                    lp[r, v] = np.float32(lp[r, v]) * theta_c
    lp = apply_rules(lp, hist, t, ngram, 0, 1.0, end_idx, pad_idx)                      # rule 2
    n_c = ctx_ngram
    if n_c >= 1 and t >= n_c - 1:                                                       # C2
        for r in range(R):
            c = rows[r]
            tail = [int(v) for v in hist[r][t - n_c + 2:t + 1]]
            assert len(tail) == n_c - 1
            for j in range(0, len(c) - n_c + 1):
                window = c[j:j + n_c]
                if all(is_word(v, V, pad_idx) for v in window) and window[:n_c - 1] == tail:
                    lp[r, window[-1]] = -np.inf
    return apply_rules(lp, hist, t, 0, min_len, 1.0, end_idx, pad_idx)                  # rule 3


def paragraphs_share_ngram(sentences, n):
    """does a sentence of the paragraph (a list of token lists) contain an n-gram of an EARLIER sentence?"""
    seen = set()
    for sent in sentences:
        grams = {tuple(sent[j:j + n]) for j in range(len(sent) - n + 1)}
        if grams & seen:
            return True
        seen |= grams
    return False


def shares_ngram(tokens, context, n, V, pad_idx):
    """does the token list contain an n-gram of the context's sentences (the runs of words between its gaps)?"""
    grams = set()
    c = [int(v) for v in context]
    for j in range(len(c) - n + 1):
        if all(is_word(v, V, pad_idx) for v in c[j:j + n]):
            grams.add(tuple(c[j:j + n]))
    return any(tuple(tokens[j:j + n]) in grams for j in range(len(tokens) - n + 1))


def case_logp(case, seed=0):
    """the case's fp32 log-probs (R, V): a log-softmax with one -inf entry (row 0, id 5)"""
    R, V = case["hist"].shape[0], case["V"]
    x = np.random.RandomState(seed).randn(R, V) * 2
    lp = (x - np.log(np.exp(x).sum(1, keepdims=True))).astype(np.float32)
    lp[0, 5] = -np.inf
    return lp


def want(case, lp):
    c = case
    return apply_context_rules(lp, c["hist"], c["t"], c["n"], c["m"], c["theta"], c["end"], c["pad"], c["ctx"], c["rpc"],
                               c["n_c"], c["theta_c"])


def _case(name, hist, t, ctx, rpc, n_c, theta_c, n=0, m=0, theta=1.0, V=V37, end=END, pad=PAD):
    hist, ctx = np.asarray(hist, dtype=np.int64), np.asarray(ctx, dtype=np.int64)
    assert hist.shape[0] == ctx.shape[0] * rpc and ctx.ndim == 2
    return dict(name=name, hist=hist, t=t, ctx=ctx, rpc=rpc, n_c=n_c, theta_c=theta_c, n=n, m=m, theta=theta, V=V, end=end, pad=pad)


def case_table():
    """cases (dicts: name, hist (R, L), t, n, m, theta, V, end, pad, ctx (R / rpc, C), rpc, n_c, theta_c).  R = 6 and V = 37
    unless a case says otherwise; histories and contexts draw from the ids 0 .. 6, so that tails match often."""
    rng = np.random.RandomState(0)
    R = 6
    cases = []
    combos = [(tc, th, n, rpc) for rpc in (1, 3) for tc in (1.0, 1.3, 0.7) for th in (1.0, 1.3) for n in (0, 3)]
    k = 0
    for n_c in range(5):
        sizes = sorted({C for C in (1, n_c - 1, n_c, 63, 64, 65, 1024) if C >= 1})
        steps = sorted({t for t in (0, n_c - 2, n_c - 1, 11) if t >= 0})
        for C in sizes:
            for t in steps:
                # two combinations per (n_c, C, t), walking through all 24 of (theta_c, theta, n, rows_per_ctx)
                for _ in range(2):
                    tc, th, n, rpc = combos[k % len(combos)]
                    k += 1
                    hist = rng.randint(0, 7, size=(R, 12))
                    hist[:, 0] = START
                    ctx = rng.randint(0, 7, size=(R // rpc, C))
                    gaps = rng.rand(R // rpc, C) < 0.1
                    ctx[gaps] = rng.choice([PAD, -1, V37], size=int(gaps.sum()))
                    m = 12 if k % 5 == 0 else 0
                    cases.append(_case(f"random n_c={n_c} C={C} t={t} theta_c={tc} theta={th} n={n} rpc={rpc} m={m}", hist, t, ctx,
                                       rpc, n_c, tc, n, m, th))
    # every (theta_c, theta, n) with both rows_per_ctx at a size where everything is live
    for tc, th, n, rpc in combos:
        hist = rng.randint(0, 7, size=(R, 12))
        hist[:, 0] = START
        ctx = rng.randint(0, 7, size=(R // rpc, 65))
        cases.append(_case(f"cross theta_c={tc} theta={th} n={n} rpc={rpc}", hist, 11, ctx, rpc, 3, tc, n, 0, th))
    # a fixed tail (3, 4) at t = 11 for the hand-made windows below
    hist = rng.randint(7, 12, size=(R, 12))
    hist[:, 0] = START
    hist[:, 10:] = (3, 4)
    hist[:, 5] = 4                                           # id 4 is in s (twice) and in the contexts
    fill = [20, PAD, 21, PAD]                                # matches nothing
    for gap in (PAD, -1, V37, 2 ** 40):
        for p in range(3):
            w = [3, 4, 8]
            w[p] = gap
            cases.append(_case(f"gap {gap} at position {p} of a matching window", hist, 11, [fill + w + fill] * R, 1, 3, 1.3))
    cases.append(_case("the window without a gap", hist, 11, [fill + [3, 4, 8] + fill] * R, 1, 3, 1.3))
    cases.append(_case("a separator between tail and follower", hist, 11, [[3, 4, PAD, 8, 3, PAD, 4, 9]] * R, 1, 3, 1.0))
    for C in (6, 64, 65, 1024):
        ctx = [[3, 4, 8] + [fill[i % 4] for i in range(C - 6)] + [3, 4, 9]] * 2
        cases.append(_case(f"matches at j = 0 and j = C - n_c, C = {C}", hist, 11, ctx, 3, 3, 0.7, theta=1.3))
    ctx = [[3, 4, 8, PAD, 3, 4, 9, 3, 4, 10, PAD, 7, 3, 4, 11, 3, 4, 8, 4, 4, 3, 4]] * R
    for n_c in (1, 2, 3, 4):
        cases.append(_case(f"several followers of one tail, n_c = {n_c}", hist, 11, ctx, 1, n_c, 1.3, n=3, theta=1.3, m=12))
    # the same id at positions 63 and 64 and 20 more times: one multiply
    row = [fill[i % 4] for i in range(128)]
    for j in [63, 64] + list(range(0, 60, 3)):
        row[j] = 9
    assert row.count(9) == 22
    cases.append(_case("one id 22 times, at 63 and 64 among them", hist, 11, [row] * 2, 3, 0, 1.3))
    cases.append(_case("one id 22 times, theta_c < 1", hist, 11, [row] * 2, 3, 2, 0.7, theta=1.3))
    # an id in both s and the context (4), and the -inf entry (row 0, id 5) under C1
    cases.append(_case("ids in s and in the context", hist, 11, [[4, 5, 3, START, 8]] * R, 1, 0, 0.7, theta=1.3))
    cases.append(_case("ids in s and in the context, theta_c only", hist, 11, [[4, 5, 3, START, 8]] * R, 1, 0, 1.3))
    cases.append(_case("a context of gaps only", hist, 11, [[PAD, -1, V37, 2 ** 40, PAD, -5]] * R, 1, 2, 1.3, n=2, theta=1.3))
    cases.append(_case("ids -1, V and 2^40 among words", hist, 11, [[4, -1, 3, 4, V37, 3, 4, 2 ** 40, 3, 4, 36, 0]] * R, 1, 3, 1.3))
    # bitmap word edges
    h65 = rng.randint(0, 7, size=(R, 12))
    h65[:, 0] = START
    h65[:, 10:] = (31, 32)
    cases.append(_case("V = 65: ids at the bitmap's word edges", h65, 11, [[31, 32, 33, 63, 64, 31, 32, 64, 0, 63, 64]] * R, 1, 3,
                       1.3, V=65, theta=0.7))
    # the flagship vocabulary with a full history and a full context
    V = 10172
    ids = np.array([0, 31, 32, 63, 64, 5000, 10170, V - 1])
    hbig = ids[rng.randint(0, len(ids), size=(4, 256))]
    hbig[:, 0] = START
    cbig = ids[rng.randint(0, len(ids), size=(2, 1024))]
    cbig[rng.rand(2, 1024) < 0.05] = PAD
    cases.append(_case("V = 10172, t = 255, C = 1024", hbig, 255, cbig, 2, 3, 1.2, n=2, m=300, theta=1.2, V=V, end=V - 1))
    return cases
