"""Restatements of what csrc/policy_loss.hip computes (include/bmhrl_hip.h, the section on the self-critical policy gradient):

  advantage()     rules R1-R7 of bmhrl_rollout_advantage in numpy float64, every sum in the order the rules fix -- the device
                  performs the same IEEE operations, so tests/test_policy_loss_gpu.py compares for equality of every word;
  policy_loss()   the row losses, row entropies and the closed-form gradient of bmhrl_policy_loss_fwd / _bwd in torch, in
                  the dtype of the log-probs: float64 is the reference, float32 on the device the yardstick.

tests/test_policy_reference_cpu.py proves both against brute-force loops and torch.autograd of the plain expressions."""
import numpy as np
import torch

NONE, LEAVE_ONE_OUT, GIVEN = 0, 1, 2


def _ordered_sum(x):
    """x[0] + x[1] + ... from 0.0, one add after the other (np.sum adds pairwise; a cumulative sum does not)"""
    return np.cumsum(np.concatenate([np.zeros(1), np.asarray(x, dtype=np.float64)]))[-1]


def advantage(toks, n, m, end_idx, scores, mode, base=None):
    """toks (B * n, >= m + 1) int64, scores (B * n, >= m) float64 -> dict(len int32, reward, adv float64, weight (B * n, m)
    float32, stats (4,) float64)"""
    toks = np.asarray(toks)[:, 1:m + 1]
    scores = np.asarray(scores, dtype=np.float64)[:, :m]
    rows = toks.shape[0]
    B = rows // n
    is_end = toks == end_idx
    ln = np.where(is_end.any(1), is_end.argmax(1) + 1, m).astype(np.int32)                        # R1
    r = scores[np.arange(rows), ln - 1].copy()                                                    # R2
    if mode == LEAVE_ONE_OUT:                                                                     # R3
        rc = r.reshape(B, n)
        s = np.zeros((B, n))
        for j in range(n):                      # j ascending; the own rollout adds +0.0, which changes no bit of a sum from +0.0
            s = s + np.where(np.arange(n)[None, :] != j, rc[:, j:j + 1], 0.0)
        b = (s / np.float64(n - 1)).reshape(rows)
    elif mode == GIVEN:
        b = np.repeat(np.asarray(base, dtype=np.float64), n)
    else:
        b = np.zeros(rows)
    adv = r - b                                                                                   # R4
    N = int(ln.astype(np.int64).sum())                                                            # R5
    w = (adv / np.float64(N)).astype(np.float32)                                                  # R6
    weight = np.where(np.arange(m)[None, :] < ln[:, None], w[:, None], np.float32(0.0)).astype(np.float32)
    stats = np.array([_ordered_sum(r) / np.float64(rows), _ordered_sum(b) / np.float64(rows), np.float64(N) / np.float64(rows),
                      np.float64(N)])                                                             # R7
    return dict(len=ln, reward=r, adv=adv, weight=weight, stats=stats)


def policy_loss(logp, action, weight, logq=None, clip=0.0, ent_weight=None, gscale=1.0, drow=None):
    """logp (rows, V); action (rows,) int64; weight, logq, ent_weight, drow (rows,) in logp's dtype (or None)
    -> (row_loss (rows,), row_entropy (rows,), grad (rows, V) = d sum_i drow_i row_loss_i / d logp * gscale)"""
    rows, V = logp.shape
    dt = logp.dtype
    neg_inf = float("-inf")
    live = (action >= 0) & (action < V)
    a = action.clamp(0, V - 1)
    idx = torch.arange(rows, device=logp.device)
    lpa = logp[idx, a]
    w = weight.to(dt)
    if logq is None:
        pol, gpol = -w * lpa, -w
    else:
        rho = torch.exp(lpa - logq.to(dt))
        un, cl = rho * w, rho.clamp(1.0 - clip, 1.0 + clip) * w
        unclipped = un <= cl
        pol = -torch.where(unclipped, un, cl)
        gpol = torch.where(unclipped, -un, torch.zeros_like(un))
    grad = torch.zeros_like(logp)
    H = torch.zeros(rows, dtype=dt, device=logp.device)
    loss = pol
    if ent_weight is not None:
        beta = ent_weight.to(dt)
        finite = logp != neg_inf
        lp0 = torch.where(finite, logp, torch.zeros_like(logp))
        p = torch.where(finite, torch.exp(logp), torch.zeros_like(logp))
        H = -(p * lp0).sum(1)
        loss = pol - beta * H
        grad = beta[:, None] * (p * (1.0 + lp0))
    grad[idx, a] += gpol
    loss = torch.where(live, loss, torch.zeros_like(loss))
    grad = torch.where(live[:, None], grad, torch.zeros_like(grad))
    scale = torch.ones(rows, dtype=dt, device=logp.device) if drow is None else drow.to(dt)
    return loss, H, grad * (scale * gscale)[:, None]
