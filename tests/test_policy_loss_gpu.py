"""csrc/policy_loss.hip on the GPU against tests/policy_reference.py (which tests/test_policy_reference_cpu.py proves against
brute-force loops and torch.autograd).

bmhrl_rollout_advantage: rules R1-R7 fix every operation and its order, so every output word is compared for EQUALITY.

bmhrl_policy_loss_fwd / _bwd: against float64 under the bound the module docstring of tests/test_loss_paths_gpu.py defines --
the yardstick is the same formulas (policy_reference.policy_loss) in float32 torch on the device on the same inputs; a kernel
result may err against float64 by twice the yardstick's error or by 2^-22 of the quantity's largest magnitude, whichever is
larger.  Every case asserts the path it is meant to reach, computed from the dispatcher's conditions in include/bmhrl_hip.h,
and prints its figures before it asserts them (pytest -s)."""
import numpy as np
import pytest
import torch

from tests import policy_reference as P
from tests.test_loss_paths_gpu import WORST, check, rows_buf, slack_untouched
from tests.test_policy_reference_cpu import ADV_CASES, END, make_rollouts

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT = -512.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bmhrl_amd import _lib
    _lib.load()
    yield torch.device("cuda:0")
    print("\nworst figures per kernel: err / yardstick (yardstick floored at 2^-23 of the magnitude), err / bound")
    for k in sorted(k for k in WORST if k.startswith("policy_loss")):
        print(f"  {k:34s} {WORST[k][0]:8.3f} {WORST[k][1]:8.3f}")


# ------------------------------------------------------------------------------------------------ the advantage kernel
def _bits(t):
    return t.cpu().contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


@pytest.mark.parametrize("B,n,m,mode", ADV_CASES)
def test_rollout_advantage_equals_the_restatement(dev, B, n, m, mode):
    """every output word, for the three row kinds (ends at step 1, never ends, ends at step m: the first rows of
    make_rollouts), with strides larger than the widths: the slack of toks holds END (never read), the slack of scores NaN,
    the slack of weight a sentinel that stays"""
    from bmhrl_amd import ops
    rows = B * n
    g = np.random.Generator(np.random.PCG64(B * 1000 + n * 50 + m))
    toks = make_rollouts(B, n, m, seed=B + n + m, ldt=m + 3)
    toks[:, m + 1:] = END
    scores = g.standard_normal((rows, m + 2)) * 3
    scores[:, m:] = np.nan
    base = g.standard_normal(B)
    want = P.advantage(toks, n, m, END, scores, mode, base)
    assert want["len"][:3].tolist() == [1, m, m][:rows]
    t, s, b = torch.from_numpy(toks).to(dev), torch.from_numpy(scores).to(dev), torch.from_numpy(base).to(dev)
    runs = []
    for _ in range(2):
        wbuf = torch.full((rows, m + 5), SENT, device=dev)
        out = (torch.full((rows,), -9, dtype=torch.int32, device=dev), torch.full((rows,), NAN, dtype=torch.float64, device=dev),
               torch.full((rows,), NAN, dtype=torch.float64, device=dev), wbuf,
               torch.full((4,), NAN, dtype=torch.float64, device=dev))
        ln, r, adv, w, stats = ops.rollout_advantage(t, n, m, END, s, mode, b if mode == P.GIVEN else None, out=out)
        assert w.shape == (rows, m) and w.data_ptr() == wbuf.data_ptr() and bool((wbuf[:, m:] == SENT).all())
        runs.append((ln, r, adv, w.contiguous(), stats))
    ln, r, adv, w, stats = runs[0]
    assert torch.equal(ln.cpu(), torch.from_numpy(want["len"]))
    for name, got in (("reward", r), ("adv", adv), ("weight", w), ("stats", stats)):
        assert torch.equal(_bits(got), _bits(torch.from_numpy(want[name]))), name
    assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(runs[0][1:], runs[1][1:])) and torch.equal(runs[0][0], runs[1][0])
    live = torch.arange(m).unsqueeze(0) < ln.cpu().unsqueeze(1)
    assert not bool(_bits(w)[~live].any()), "the weight is +0.0 from len_i on"


def test_rollout_advantage_refuses_bad_arguments(dev):
    from bmhrl_amd import _lib, ops
    lib = _lib.load()
    B, n, m = 2, 3, 4
    rows = B * n
    t = torch.zeros(rows, m + 1, dtype=torch.int64, device=dev)
    s = torch.zeros(rows, m, dtype=torch.float64, device=dev)
    base = torch.zeros(B, dtype=torch.float64, device=dev)
    ln = torch.zeros(rows, dtype=torch.int32, device=dev)
    r, a = torch.zeros(rows, dtype=torch.float64, device=dev), torch.zeros(rows, dtype=torch.float64, device=dev)
    w = torch.zeros(rows, m, device=dev)
    st = torch.zeros(4, dtype=torch.float64, device=dev)
    ptrs = dict(toks=t.data_ptr(), scores=s.data_ptr(), base=base.data_ptr(), len=ln.data_ptr(), reward=r.data_ptr(),
                adv=a.data_ptr(), weight=w.data_ptr(), stats=st.data_ptr())

    def call(**kw):
        k = dict(ptrs, ldt=m + 1, B=B, n=n, m=m, lds=m, mode=1, ldw=m)
        k.update(kw)
        return lib.bmhrl_rollout_advantage(k["toks"], k["ldt"], k["B"], k["n"], k["m"], END, k["scores"], k["lds"], k["mode"],
                                           k["base"], k["len"], k["reward"], k["adv"], k["weight"], k["ldw"], k["stats"],
                                           ops.stream())
    assert call() == 0 and call(mode=0, base=None) == 0 and call(mode=2) == 0
    bad = [dict(toks=None), dict(scores=None), dict(len=None), dict(reward=None), dict(adv=None), dict(weight=None),
           dict(stats=None), dict(n=0), dict(n=17), dict(m=0), dict(m=ops.REWARDS_MAX_L + 1), dict(B=0), dict(B=-1),
           dict(mode=1, n=1), dict(mode=2, base=None), dict(mode=3), dict(mode=-1), dict(ldt=m), dict(lds=m - 1), dict(ldw=m - 1)]
    for kw in bad:
        assert call(**kw) == -22, kw
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.rollout_advantage(t, 4, m, END, s)                 # 6 rows do not divide into clips of 4
    with pytest.raises(ValueError):
        ops.rollout_advantage(t, n, m, END, s, ops.BASELINE_GIVEN)


# ------------------------------------------------------------------------------------------------ the loss kernels
EPS = 0.2
RATIOS = [0.5, 0.95, 1.0, 1.05, 1.5]


def loss_rows(V, rows, seed, clip):
    """the row table.  clip off: action at column 0 (row 0) and V - 1 (row 1), actions out of range (rows 2 and 5: V and
    -1), w = 0 (row 3), > 0, < 0, a -inf column away from the action (row 4).  clip on: the target ratios with both signs of
    w (rows 0-9, logq built from the ratio); further rows are random."""
    g = torch.Generator().manual_seed(seed)
    logp = torch.log_softmax(torch.randn(rows, V, generator=g) * 3, -1)
    action = torch.randint(0, V, (rows,), generator=g)
    w = torch.randn(rows, generator=g)
    logq = None
    action[0], action[1] = 0, V - 1
    w[0], w[1] = abs(float(w[0])) + 0.1, -abs(float(w[1])) - 0.1
    logp[4, (int(action[4]) + 1) % V] = float("-inf")
    if clip:
        assert rows >= 10
        ratio = torch.tensor((RATIOS + RATIOS + [0.7, 1.3] * rows)[:rows], dtype=torch.float64)
        w[:10] = torch.tensor([0.7] * 5 + [-0.7] * 5)
        lpa = logp[torch.arange(rows), action].double()
        logq = (lpa - torch.log(ratio)).float()
        rho = torch.exp(lpa - logq.double())
        assert bool(((rho - (1 - EPS)).abs() > 1e-3).all() and ((rho - (1 + EPS)).abs() > 1e-3).all()), "a row at a clip boundary"
    else:
        action[2], action[5] = V, -1
        w[3] = 0.0
    beta = torch.rand(rows, generator=g) * 0.05
    drow = torch.randn(rows, generator=g)
    return logp, action, w, logq, beta, drow


def expected_vec(V, lds, ptrs):
    """the 16-byte path, from the conditions include/bmhrl_hip.h states for the dispatchers"""
    return V % 4 == 0 and all(ld % 4 == 0 for ld in lds) and all(p % 16 == 0 for p in ptrs)


# V, ld, offset of the base pointers in floats, whether the case is for the 16-byte path
LOSS_CASES = [(V, V + d, off, V % 4 == 0 and d % 4 == 0 and off == 0)
              for V in (4, 51, 52, 1028, 10172, 12292) for d, off in ((0, 0), (4, 0), (3, 0), (0, 1))]


@pytest.mark.parametrize("clip", [0.0, EPS])
@pytest.mark.parametrize("V,ld,off,want_vec", LOSS_CASES)
def test_policy_loss_paths(dev, V, ld, off, want_vec, clip):
    """forward (the gather without beta, the row reduction with it) and the one-pass dense backward, beta null and given; the
    outputs start NaN-filled and are fully overwritten, the slack columns V .. ld and the tails stay untouched, two runs give
    equal bits"""
    from bmhrl_amd import ops
    rows = 10 if clip else 7
    logp, action, w, logq, beta, drow = loss_rows(V, rows, V + ld + off, clip)
    buf, lp = rows_buf(dev, logp, ld, off)
    assert expected_vec(V, [ld], [lp.data_ptr()]) == want_vec, "this case no longer reaches the path it is for"
    a, wd, bd, dr = action.to(dev), w.to(dev), beta.to(dev), drow.to(dev)
    lq = logq.to(dev) if clip else None
    gscale = torch.tensor([1.7], device=dev)
    k17 = float(torch.tensor(1.7, dtype=torch.float32))
    lp64 = logp.double()
    for ent in (False, True):
        ref = P.policy_loss(lp64, action, w.double(), logq.double() if clip else None, clip, beta.double() if ent else None,
                            k17, drow.double())
        yard = P.policy_loss(logp.to(dev), a, wd, lq, clip, bd if ent else None, k17, dr)
        path = ("vec" if want_vec else "scalar") if ent else "gather"
        what = f"V={V} ld={ld} off={off} clip={clip} beta={'given' if ent else 'null'}"
        got = []
        for _ in range(2):
            rl, re = torch.full((rows,), NAN, device=dev), torch.full((rows,), NAN, device=dev)
            ops.policy_loss_fwd(lp, ld, a, wd, lq, clip, bd if ent else None, rl, re, rows, V)
            gbuf, g = rows_buf(dev, torch.full((rows, V), NAN), ld, off, SENT)
            assert expected_vec(V, [ld, ld], [lp.data_ptr(), g.data_ptr()]) == want_vec
            ops.policy_loss_bwd(lp, ld, a, wd, lq, clip, bd if ent else None, gscale, dr, g, ld, rows, V)
            assert slack_untouched(gbuf, g, ld, off, SENT), "the gradient's slack columns were written"
            got.append((rl, re, g.contiguous()))
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(*got)), "two runs differ"
        rl, re, g = got[0]
        assert bool(torch.isfinite(rl).all() and torch.isfinite(re).all() and torch.isfinite(g).all())
        check(f"policy_loss_fwd {path}", what + " row_loss", rl, ref[0], yard[0])
        if ent:
            check(f"policy_loss_fwd {path}", what + " row_entropy", re, ref[1], yard[1])
        else:
            assert not bool(re.view(torch.int32).any()), "row_entropy is +0.0 without beta"
        check(f"policy_loss_bwd {'vec' if want_vec else 'scalar'} beta {'given' if ent else 'null'}", what, g, ref[2], yard[2])
        if not ent:
            # zeros and one entry per row: exactly -w gscale drow (clip off) at the action, nothing anywhere else
            nz = (g != 0).sum(1).cpu()
            assert bool((nz <= 1).all())
        if not clip:
            for r in (2, 5):
                assert float(rl[r]) == 0.0 and not bool(g[r].view(torch.int32).any()), "an action out of range contributes nothing"
            assert ent or float(rl[3]) == 0.0
    assert slack_untouched(buf, lp, ld, off)


def test_policy_loss_gather_path_300_rows_and_mixed_alignment(dev):
    """300 rows through the entropy-less forward (one thread per row, two blocks) and the backward of the same rows; then a
    backward whose log-probs qualify for the 16-byte path and whose gradient buffer does not (the scalar path)"""
    from bmhrl_amd import ops
    V, rows = 52, 300
    logp, action, w, _, beta, drow = loss_rows(V, rows, 5, 0.0)
    lp, a, wd, dr = logp.to(dev), action.to(dev), w.to(dev), drow.to(dev)
    one = torch.ones(1, device=dev)
    ref = P.policy_loss(logp.double(), action, w.double(), drow=drow.double())
    yard = P.policy_loss(lp, a, wd, drow=dr)
    rl, re = torch.full((rows,), NAN, device=dev), torch.full((rows,), NAN, device=dev)
    ops.policy_loss_fwd(lp, V, a, wd, None, 0.0, None, rl, re, rows, V)
    check("policy_loss_fwd gather", "300 rows", rl, ref[0], yard[0])
    assert not bool(re.view(torch.int32).any())
    for off, want_vec in ((0, True), (1, False)):
        gbuf, g = rows_buf(dev, torch.full((rows, V), NAN), V, off, SENT)
        assert expected_vec(V, [V, V], [lp.data_ptr(), g.data_ptr()]) == want_vec
        ops.policy_loss_bwd(lp, V, a, wd, None, 0.0, None, one, dr, g, V, rows, V)
        check(f"policy_loss_bwd {'vec' if want_vec else 'scalar'} beta null", f"300 rows off={off}", g, ref[2], yard[2])
        assert slack_untouched(gbuf, g, V, off, SENT)


def test_policy_loss_refuses_bad_arguments(dev):
    from bmhrl_amd import _lib, ops
    lib = _lib.load()
    rows, V = 3, 8
    lp = torch.zeros(rows, V, device=dev)
    a = torch.zeros(rows, dtype=torch.int64, device=dev)
    f = lambda: torch.zeros(rows, device=dev)                                     # noqa: E731
    w, lq, rl, re, dr, one = f(), f(), f(), f(), f(), torch.ones(1, device=dev)
    g = torch.zeros(rows, V, device=dev)
    p = lambda t: None if t is None else t.data_ptr()                             # noqa: E731

    def fwd(**k):
        return lib.bmhrl_policy_loss_fwd(p(k.get("lp", lp)), k.get("ld", V), p(k.get("a", a)), p(k.get("w", w)), p(k.get("lq")),
                                         k.get("clip", 0.0), None, p(k.get("rl", rl)), p(k.get("re", re)), k.get("rows", rows),
                                         k.get("V", V), ops.stream())

    def bwd(**k):
        return lib.bmhrl_policy_loss_bwd(p(k.get("lp", lp)), k.get("ld", V), p(a), p(w), p(k.get("lq")), k.get("clip", 0.0), None,
                                         p(k.get("gs", one)), p(k.get("dr", dr)), p(k.get("g", g)), k.get("ldg", V),
                                         k.get("rows", rows), k.get("V", V), ops.stream())
    assert fwd() == 0 and bwd() == 0 and fwd(clip=0.2, lq=lq) == 0 and bwd(clip=0.2, lq=lq) == 0
    for kw in (dict(clip=0.2), dict(lq=lq), dict(clip=-0.1, lq=lq), dict(clip=float("nan"), lq=lq), dict(lp=None), dict(rows=0),
               dict(V=0), dict(ld=V - 1)):
        assert fwd(**kw) == -22 and bwd(**kw) == -22, kw
    for kw in (dict(a=None), dict(w=None), dict(rl=None), dict(re=None)):
        assert fwd(**kw) == -22, kw
    for kw in (dict(gs=None), dict(dr=None), dict(g=None), dict(ldg=V - 1)):
        assert bwd(**kw) == -22, kw
    torch.cuda.synchronize()


def test_policy_loss_node(dev):
    """functional.PolicyLossFn: values and d logp through autograd, with and without clip and entropy; row_entropy is not
    differentiable and nothing but logp gets a gradient"""
    from bmhrl_amd.functional import PolicyLossFn
    R, m, V = 2, 5, 52
    rows = R * m
    for clip in (0.0, EPS):
        logp, action, w, logq, beta, drow = loss_rows(V, rows, 11, clip)
        for ent in (False, True):
            x = logp.to(dev).view(R, m, V).clone().requires_grad_(True)
            wt = w.to(dev).view(R, m).clone().requires_grad_(True)
            rl, re = PolicyLossFn.apply(x, action.to(dev).view(R, m), wt, logq.to(dev).view(R, m) if clip else None, clip,
                                        beta.to(dev).view(R, m) if ent else None)
            assert rl.shape == (rows,) and re.shape == (rows,) and not re.requires_grad
            (rl * drow.to(dev)).sum().backward()
            assert wt.grad is None
            ref = P.policy_loss(logp.double(), action, w.double(), logq.double() if clip else None, clip,
                                beta.double() if ent else None, 1.0, drow.double())
            yard = P.policy_loss(logp.to(dev), action.to(dev), w.to(dev), logq.to(dev) if clip else None, clip,
                                 beta.to(dev) if ent else None, 1.0, drow.to(dev))
            what = f"clip={clip} beta={'given' if ent else 'null'}"
            check("policy_loss node", what + " row_loss", rl, ref[0], yard[0])
            check("policy_loss node", what + " d logp", x.grad.view(rows, V), ref[2], yard[2])
    with pytest.raises(ValueError):
        PolicyLossFn.apply(x, action.to(dev).view(R, m), wt, None, 0.2, None)
