"""tests/policy_reference.py (the float64 restatements the GPU tests of csrc/policy_loss.hip compare against) proven against
brute-force Python loops (rules R1-R7 of the advantages) and float64 torch.autograd of the plain expressions (gather,
torch.min / clamp, -(p * logp).sum()), plus the argument validation of bmhrl_amd/scst.py.  No GPU."""
import numpy as np
import pytest
import torch

from tests import policy_reference as P

END, PAD = 5, 1


def make_rollouts(B, n, m, seed, ldt=None):
    """toks (B * n, ldt) with the three row kinds in front: a row that ends at step 1, one that never ends, one that ends at
    step m; the rest end at random steps or never.  pad after the end; -7 in the slack columns"""
    g = np.random.Generator(np.random.PCG64(seed))
    rows = B * n
    ldt = ldt or m + 1
    toks = np.full((rows, ldt), -7, dtype=np.int64)
    toks[:, 0] = 2
    body = g.integers(6, 50, size=(rows, m))
    ends = g.integers(1, m + 2, size=rows)            # m + 1: never ends
    kinds = [1, m + 1, m]
    for i in range(rows):
        e = kinds[i] if i < len(kinds) else int(ends[i])
        if e <= m:
            body[i, e - 1] = END
            body[i, e:] = PAD
    toks[:, 1:m + 1] = body
    return toks


def brute_advantage(toks, n, m, end_idx, scores, mode, base):
    rows = len(toks)
    ln, r = [], []
    for i in range(rows):
        l = m
        for t in range(m):
            if toks[i][1 + t] == end_idx:
                l = t + 1
                break
        ln.append(l)
        r.append(float(scores[i][l - 1]))
    b = []
    for i in range(rows):
        c = i // n
        if mode == P.LEAVE_ONE_OUT:
            s = 0.0
            for j in range(n):
                if c * n + j != i:
                    s = s + r[c * n + j]
            b.append(s / float(n - 1))
        elif mode == P.GIVEN:
            b.append(float(base[c]))
        else:
            b.append(0.0)
    adv = [r[i] - b[i] for i in range(rows)]
    N = sum(ln)
    weight = [[float(np.float32(adv[i] / float(N))) if t < ln[i] else 0.0 for t in range(m)] for i in range(rows)]
    sr = sb = 0.0
    for i in range(rows):
        sr = sr + r[i]
        sb = sb + b[i]
    return ln, r, adv, weight, [sr / float(rows), sb / float(rows), float(N) / float(rows), float(N)]


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64 if np.asarray(x).dtype == np.float64 else np.uint32)


# (leave-one-out needs two rollouts per clip: n = 1 is refused by the kernel and by scst.check_args)
ADV_CASES = [(B, n, m, mode) for B, n, m in [(1, 2, 1), (2, 4, 7), (3, 16, 30), (300, 1, 30)]
             for mode in (P.NONE, P.LEAVE_ONE_OUT, P.GIVEN) if not (mode == P.LEAVE_ONE_OUT and n == 1)]


@pytest.mark.parametrize("B,n,m,mode", ADV_CASES)
def test_advantage_restatement_equals_brute_force(B, n, m, mode):
    g = np.random.Generator(np.random.PCG64(B * 1000 + n * 50 + m))
    toks = make_rollouts(B, n, m, seed=B + n + m, ldt=m + 3)
    scores = g.standard_normal((B * n, m + 2)) * 3
    base = g.standard_normal(B)
    got = P.advantage(toks, n, m, END, scores, mode, base)
    ln, r, adv, weight, stats = brute_advantage(toks.tolist(), n, m, END, scores.tolist(), mode, base.tolist())
    assert got["len"].dtype == np.int32 and got["len"].tolist() == ln
    assert np.array_equal(bits(got["reward"]), bits(np.array(r)))
    assert np.array_equal(bits(got["adv"]), bits(np.array(adv)))
    assert got["weight"].dtype == np.float32 and np.array_equal(bits(got["weight"]), bits(np.array(weight, dtype=np.float32)))
    assert np.array_equal(bits(got["stats"]), bits(np.array(stats)))
    # the three row kinds: ends at step 1, never ends, ends at step m (as many of them as the case has rows)
    assert ln[:3] == [1, m, m][:B * n]
    # the weight is +0.0 (the sign bit too) from len_i on, and the advantage over the token count before
    for i in range(B * n):
        assert not bits(got["weight"][i, ln[i]:]).any()
        assert (got["weight"][i, :ln[i]] == np.float32(got["adv"][i] / stats[3])).all()
    if mode == P.LEAVE_ONE_OUT:
        # leave-one-out advantages of a clip sum to 0 within one rounding of the terms that were added: n r_i and n b_i
        # carry n - 1 roundings each at the size of the clip's rewards
        a, rc = got["adv"].reshape(B, n), got["reward"].reshape(B, n)
        assert (np.abs(a.sum(1)) <= 4 * n * np.finfo(np.float64).eps * np.abs(rc).sum(1)).all()
    if mode == P.NONE:
        assert np.array_equal(bits(got["adv"]), bits(got["reward"])) and stats[1] == 0.0


def test_constant_scores_give_zero_leave_one_out_advantages():
    toks = make_rollouts(4, 3, 6, seed=1)
    got = P.advantage(toks, 3, 6, END, np.full((12, 6), 0.3), P.LEAVE_ONE_OUT)
    assert not got["adv"].any() and not bits(got["weight"]).any()


def plain_loss(logp, action, weight, logq, clip, ent_weight):
    """the plain expressions, for torch.autograd; rows with an action out of range are left out by the caller"""
    lpa = logp.gather(1, action[:, None])[:, 0]
    if logq is None:
        pol = -weight * lpa
    else:
        rho = torch.exp(lpa - logq)
        pol = -torch.min(rho * weight, torch.clamp(rho, 1 - clip, 1 + clip) * weight)
    if ent_weight is None:
        return pol, torch.zeros_like(pol)
    p = torch.exp(logp)
    plogp = torch.where(torch.isinf(logp), torch.zeros_like(logp), p * logp.clamp_min(-1e300))
    H = -plogp.sum(1)
    return pol - ent_weight * H, H


def table(V, rows, seed):
    g = torch.Generator().manual_seed(seed)
    logp = torch.log_softmax(torch.randn(rows, V, generator=g, dtype=torch.float64) * 3, -1)
    action = torch.randint(0, V, (rows,), generator=g)
    action[0], action[1] = 0, V - 1
    weight = torch.randn(rows, dtype=torch.float64, generator=g)
    weight[2] = 0.0
    if V > 3:
        logp[3, (int(action[3]) + 1) % V] = float("-inf")       # a -inf column away from the action
    return logp, action, weight


@pytest.mark.parametrize("V", [4, 51, 1028])
@pytest.mark.parametrize("clip", [0.0, 0.2])
@pytest.mark.parametrize("ent", [False, True])
def test_loss_restatement_equals_autograd(V, clip, ent):
    rows = 12
    logp, action, weight = table(V, rows, seed=V)
    g = torch.Generator().manual_seed(V + 1)
    logq = None
    if clip > 0:
        ratios = torch.tensor([0.5, 0.95, 1.0, 1.05, 1.5, 0.5, 0.95, 1.0, 1.05, 1.5, 0.7, 1.3], dtype=torch.float64)
        weight = torch.cat([torch.full((5,), 0.7), torch.full((5,), -0.7), torch.tensor([0.0, 0.3])]).double()
        logq = logp[torch.arange(rows), action] - torch.log(ratios)
    beta = torch.rand(rows, dtype=torch.float64, generator=g) if ent else None
    drow = torch.randn(rows, dtype=torch.float64, generator=g)
    x = logp.clone().requires_grad_(True)
    loss, H = plain_loss(x, action, weight, logq, clip, beta)
    (loss * drow).sum().mul(1.7).backward()
    got_loss, got_H, got_grad = P.policy_loss(logp, action, weight, logq, clip, beta, gscale=1.7, drow=drow)
    assert torch.allclose(got_loss, loss.detach(), rtol=1e-14, atol=1e-15)
    assert torch.allclose(got_H, H.detach(), rtol=1e-14, atol=1e-15)
    assert torch.isfinite(got_grad).all() and torch.isfinite(got_loss).all()
    assert torch.allclose(got_grad, x.grad, rtol=1e-13, atol=1e-15)
    if clip > 0:
        # the clipped branch is taken (zero gradient at the action) exactly where the ratio leaves [1 - eps, 1 + eps] on the
        # side the advantage's sign rewards; the ratio 1.0 is a tie of the two branches and keeps the gradient
        ga = got_grad[torch.arange(rows), action] - (0 if beta is None else
                                                     (beta * torch.exp(logp[torch.arange(rows), action]) *
                                                      (1 + logp[torch.arange(rows), action]) * drow * 1.7))
        want_zero = [False, False, False, False, True, True, False, False, False, False, True, True]
        assert [abs(float(v)) < 1e-12 for v in ga] == want_zero
    # an action out of range: the row contributes nothing
    bad = action.clone()
    bad[4], bad[5] = -1, V
    l2, _, g2 = P.policy_loss(logp, bad, weight, logq, clip, beta, gscale=1.7, drow=drow)
    assert float(l2[4]) == 0.0 and float(l2[5]) == 0.0 and not g2[4].any() and not g2[5].any()
    keep = torch.ones(rows, dtype=torch.bool)
    keep[4] = keep[5] = False
    assert torch.equal(l2[keep], got_loss[keep]) and torch.equal(g2[keep], got_grad[keep])


def test_scst_argument_validation():
    from bmhrl_amd import scst
    scst.check_args("mean", 4, 0.0, 0.0)
    scst.check_args("none", 1, 0.2, 0.01)
    scst.check_args("greedy", 16, 0.0, 0.0)
    for bad in (dict(baseline="mean", n=1), dict(baseline="median"), dict(clip=-0.1), dict(entropy=-1e-3), dict(n=17), dict(n=0),
                dict(clip=float("nan")), dict(entropy=float("nan"))):
        with pytest.raises(ValueError):
            scst.check_args(**bad)
    # self_critical_loss refuses the same arguments before it touches a tensor (no GPU, no library here)
    ro = scst.Rollouts(torch.zeros(4, 3, dtype=torch.int64), torch.zeros(4, 2), torch.zeros(4, 2), 2, 1, END)
    pred = torch.zeros(4, 2, 7)
    for kw in (dict(baseline="mean"), dict(baseline="x"), dict(clip=-1.0), dict(entropy=-1.0)):
        with pytest.raises(ValueError):
            scst.self_critical_loss(pred, ro, torch.zeros(4, 2, dtype=torch.float64), **{"baseline": "none", **kw})
    with pytest.raises(ValueError):
        scst.self_critical_loss(pred, ro._replace(n=17), torch.zeros(4, 2, dtype=torch.float64), baseline="none")
    with pytest.raises(ValueError):
        scst.self_critical_loss(pred, ro, torch.zeros(4, 2, dtype=torch.float64), baseline="greedy")     # no greedy_scores
    with pytest.raises(ValueError):
        scst.rollout(None, {}, 10, 2, END, PAD, "audio_video", n=17)
    with pytest.raises(ValueError):
        scst.prefix_scores(None, torch.zeros(4, 3, dtype=torch.int64), ["a", "b", "c"])               # 4 rows, 3 clips
    # the loop refuses before the first batch
    from types import SimpleNamespace
    from bmhrl_amd.epoch_loops.captioning_scst_loops import train_bmhrl_scst
    for kw in (dict(scst_samples=1), dict(scst_baseline="x"), dict(scst_clip=-1.0), dict(scst_entropy=-1.0), dict(scst_samples=17)):
        with pytest.raises(ValueError):
            train_bmhrl_scst(SimpleNamespace(**kw), {}, None, None, 0, "t", None)
