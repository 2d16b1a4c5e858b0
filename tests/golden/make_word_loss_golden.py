"""Runs the reference's own HungarianMatcher (loss/hungarian_matcher.py) and loss_labels
(epoch_loops/captioning_bmrl_loops.py) on small cases, on the CPU, and writes tests/golden/word_loss.npz: per case the
logits, the captions, the reference's matches as padded arrays, the class map they imply, the loss and d loss / d logits.
captioning_bmrl_loops imports nltk at module level without using it here: make_golden.py's empty stand-in modules let it
import.  The archive is written with fixed zip timestamps, so a rerun reproduces it byte for byte.

Cases: Q = 100 queries, B = 3, L = 12, logits 3 * randn rounded to fp16-representable values (stored in two bytes each,
exact as fp32), C in {41, 173}; the captions hold trailing pads, interspersed pads, a duplicated word, an all-pad row and
a full row.  A case is written only if its class map is stable: each of 16 random perturbations of the probabilities within
+-1e-5 is re-matched with scipy and must give the same map -- a case whose optimum hinges on fp32 rounding pins nothing.
usage: make_word_loss_golden.py REFERENCE_CHECKOUT"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "word_loss.npz")
Q, B, L, PAD = 100, 3, 12, 1
MARGIN, TRIALS = 1e-5, 16

# (C, seed, captions): ids in [0, C - 2], 1 is the pad
CASES = [
    (41, 11, [[2, 7, 9, 7, 30, 3, 1, 1, 1, 1, 1, 1],          # trailing pads, word 7 twice
              [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1],           # all pads
              [2, 4, 5, 6, 8, 10, 12, 39, 0, 22, 23, 3]]),    # full row (first and last word ids of the range)
    (173, 12, [[1, 2, 1, 50, 171, 1, 1, 60, 3, 1, 1, 90],     # interspersed pads, leading pad, word after the last pad
               [2, 15, 16, 3, 1, 1, 1, 1, 1, 1, 1, 1],        # trailing pads
               [2, 100, 101, 100, 102, 100, 5, 6, 7, 8, 9, 3]]),   # full row, word 100 three times
]


def class_map_of(cap, matches, C):
    cls = np.full((B, Q), C - 1, dtype=np.int32)
    for b, (i, j) in enumerate(matches):
        words = cap[b][cap[b] != PAD]
        cls[b, i.numpy()] = words[j.numpy()]
    return cls


def stable(logits, cap, cls, C, seed):
    from scipy.optimize import linear_sum_assignment
    x = logits.astype(np.float64)
    p = np.exp(x - x.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    rng = np.random.default_rng(seed)
    for _ in range(TRIALS):
        for b in range(B):
            words = cap[b][cap[b] != PAD]
            cost = -(p[b][:, words] + rng.uniform(-MARGIN, MARGIN, size=(Q, len(words))))
            again = np.full(Q, C - 1, dtype=np.int32)
            if len(words):
                i, j = linear_sum_assignment(cost)
                again[i] = words[j]
            if not np.array_equal(again, cls[b]):
                return False
    return True


def main(ref):
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.abspath(ref))
    import torch
    from make_golden import import_reference_loops
    from make_reward_golden import save
    loops, _ = import_reference_loops()
    from loss.hungarian_matcher import HungarianMatcher
    out = {"n_cases": np.array(0)}
    n = 0
    for C, seed, captions in CASES:
        g = torch.Generator().manual_seed(seed)
        logits = (3 * torch.randn(B, Q, C, generator=g)).half()
        x = logits.float().requires_grad_(True)
        cap = torch.tensor(captions, dtype=torch.int64)
        assert cap.shape == (B, L) and int(cap.max()) <= C - 2 and int(cap.min()) >= 0
        matches = HungarianMatcher()(x.detach(), cap)
        loss = loops.loss_labels(x, cap, matches)
        loss.backward()
        cls = class_map_of(cap.numpy(), matches, C)
        if not stable(logits.float().numpy(), cap.numpy(), cls, C, seed):
            print(f"case C={C} seed={seed}: class map not stable under +-{MARGIN}, skipped")
            continue
        mi = np.full((B, L), -1, dtype=np.int64)
        mj = np.full((B, L), -1, dtype=np.int64)
        mn = np.zeros(B, dtype=np.int64)
        for b, (i, j) in enumerate(matches):
            mn[b] = len(i)
            mi[b, :len(i)], mj[b, :len(j)] = i.numpy(), j.numpy()
        out[f"c{n}_logits"] = logits.numpy()                      # float16, exact
        out[f"c{n}_captions"] = cap.numpy()
        out[f"c{n}_match_i"], out[f"c{n}_match_j"], out[f"c{n}_match_n"] = mi, mj, mn
        out[f"c{n}_class_map"] = cls
        out[f"c{n}_loss"] = loss.detach().numpy()
        out[f"c{n}_grad"] = x.grad.numpy()
        n += 1
    out["n_cases"] = np.array(n)
    out["pad_eos"] = np.array([PAD, 0.1])
    save(OUT, out)
    print(OUT, os.path.getsize(OUT), "bytes,", n, "cases")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
