"""Rules G1-G4 of the group beam search section of bmhrl_amd/decode.py, restated for one token step in numpy.  Shares no code
with decode.py: the candidates of a group are listed in the order of their flat index k*V + v and sorted by a stable argsort
of -a.  All arithmetic is IEEE fp32: the add s = score_k + lp(k, v) is numpy's elementwise float32 add over a beam's row (one
fp32 add per entry), the penalty of an entry with c > 0 is one np.float32 multiply, then one np.float32 subtract."""
import numpy as np


def initial_state(B, K, G):
    """rule G1 -> (scores (B, K) float32, finished (B, K) bool)"""
    Kp = K // G
    scores = np.full((B, K), -np.inf, dtype=np.float32)
    finished = np.ones((B, K), dtype=bool)
    scores[:, ::Kp] = 0.0
    finished[:, ::Kp] = False
    return scores, finished


def group_beam_step(logp, scores, finished, G, penalty, end_idx, pad_idx, gaps=False):
    """logp (B, K, V) float32, scores (B, K) float32, finished (B, K) bool -> new scores (B, K) float32, finished (B, K) bool,
    parents (B, K) (the beam index 0..K-1 within the sample) and tokens (B, K) int64.  gaps=True: also (B, G) float64, per
    group the difference of its K'-th and (K'+1)-th selection values (inf where the group has no (K'+1)-th candidate; NaN
    where both are -inf)."""
    logp = np.asarray(logp, dtype=np.float32)
    scores = np.asarray(scores, dtype=np.float32)
    finished = np.asarray(finished).astype(bool)
    B, K, V = logp.shape
    assert K % G == 0
    Kp = K // G
    lam = np.float32(penalty)
    new_scores = np.empty((B, K), dtype=np.float32)
    new_finished = np.empty((B, K), dtype=bool)
    parents = np.empty((B, K), dtype=np.int64)
    tokens = np.empty((B, K), dtype=np.int64)
    gap = np.full((B, G), np.inf, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(B):
            count = np.zeros(V, dtype=np.int64)                    # c_g(v) of rule G2
            for g in range(G):
                flat, s_all, a_all = [], [], []
                for k in range(g * Kp, (g + 1) * Kp):
                    if finished[b, k]:                             # the single candidate (k, pad), never penalised
                        flat.append(np.array([k * V + pad_idx], dtype=np.int64))
                        s_all.append(scores[b, k:k + 1])
                        a_all.append(scores[b, k:k + 1])
                        continue
                    s = scores[b, k] + logp[b, k]                  # float32 + float32 row: one fp32 add per entry
                    assert s.dtype == np.float32
                    a = s.copy()
                    for v in np.nonzero(count)[0]:
                        a[v] = s[v] - lam * np.float32(count[v])   # np.float32 scalars: multiply, then subtract
                    flat.append(k * V + np.arange(V, dtype=np.int64))
                    s_all.append(s)
                    a_all.append(a)
                flat, s_all, a_all = np.concatenate(flat), np.concatenate(s_all), np.concatenate(a_all)
                order = np.argsort(-a_all, kind="stable")
                if len(order) > Kp:
                    gap[b, g] = np.float64(a_all[order[Kp - 1]]) - np.float64(a_all[order[Kp]])
                for j, o in enumerate(order[:Kp]):
                    p, v = divmod(int(flat[o]), V)
                    r = g * Kp + j
                    new_scores[b, r] = s_all[o]                    # s, not a (rule G4)
                    new_finished[b, r] = finished[b, p] or v == end_idx
                    parents[b, r] = p
                    tokens[b, r] = v
                    if not finished[b, p]:
                        count[v] += 1
    out = (new_scores, new_finished, parents, tokens)
    return out + (gap,) if gaps else out
