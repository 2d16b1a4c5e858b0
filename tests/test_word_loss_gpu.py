"""The DETR word loss on the device (csrc/word_loss.hip) against the float64 restatement
(tests/word_loss_reference.py), scipy's optimum and the fixture recorded from the reference (tests/golden/word_loss.npz).

Tolerances are not fixed numbers.  Cost pass: the yardstick is ops.log_softmax_ on the same rows -- lse and cost may err
by twice its worst log-prob error or by 2^-22 |lse| (|d exp(y)| <= |dy| for y <= 0).  Loss and gradient: torch's own fp32
F.cross_entropy forward and backward on the device with the same class map -- twice its error against float64, or 2^-22
relative; the gradient's error is relative to its largest entry.  Every figure is printed before it is asserted."""
import os

import numpy as np
import pytest
import torch

from tests import word_loss_reference as ref

pytestmark = pytest.mark.gpu

PAD = 1
QL = [(1, 1), (5, 1), (100, 1), (100, 7), (100, 64), (128, 1), (128, 7), (128, 64)]      # Q in {1,5,100,128} x L in {1,7,64}, L <= Q
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "word_loss.npz")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bmhrl_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def make_logits(B, Q, C, seed, scale=3.0):
    return (scale * torch.randn(B, Q, C, generator=torch.Generator().manual_seed(seed))).contiguous()


def make_captions(B, L, C, seed, p_pad=0.3):
    """ids in [0, C - 2] without the pad, pads anywhere; with B = 3 one row is all pads and one is full"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.tensor([v for v in range(C - 1) if v != PAD])
    cap = ids[torch.randint(0, len(ids), (B, L), generator=g)]
    cap[torch.rand(B, L, generator=g) < p_pad] = PAD
    if B == 3:
        cap[1] = PAD
        cap[2] = ids[torch.randint(0, len(ids), (L,), generator=g)]
    return cap


def in_padded_buffer(x, extra, dev, fill=float("nan")):
    """x (B, Q, C) as a view of the first C columns of a (B, Q, C + extra) device buffer filled with `fill`"""
    B, Q, C = x.shape
    buf = torch.full((B, Q, C + extra), fill, device=dev)
    buf[:, :, :C] = x.to(dev)
    return buf, (buf[:, :, :C] if extra else buf)


def yardstick_lse_tol(x, lse64, dev):
    """per-row bound on |lse - lse64| and |cost - cost64|: twice the worst log-prob error of ops.log_softmax_ on these rows, or
    2^-22 |lse|"""
    from bmhrl_amd import ops
    B, Q, C = x.shape
    lp = x.reshape(B * Q, C).to(dev).contiguous()
    ops.log_softmax_(lp, C, B * Q, C)
    lp64 = x.double().numpy().reshape(B * Q, C) - lse64.reshape(B * Q, 1)
    err = float(np.abs(lp.cpu().double().numpy() - lp64).max())
    return np.maximum(2 * err, 2.0 ** -22 * np.abs(lse64)), err


def check_cost_pass(x, cap, extra, dev, cost_scale=1.0):
    from bmhrl_amd import ops
    B, Q, C = x.shape
    _, xv = in_padded_buffer(x, extra, dev)
    words, n, lse, x_none, gathered, cost = ops.word_cost(xv, cap.to(dev), PAD, cost_scale)
    torch.cuda.synchronize()
    w64, n64, lse64, none64, g64, c64 = ref.cost_pass(x.numpy(), cap.numpy(), PAD, cost_scale)
    assert np.array_equal(words.cpu().numpy(), w64) and np.array_equal(n.cpu().numpy(), n64)
    assert torch.isfinite(lse).all() and torch.isfinite(cost).all()
    # the logits at the words and at "no word" are copies; behind the n_b words both arrays are 0
    assert np.array_equal(gathered.cpu().numpy(), g64.astype(np.float32))
    assert np.array_equal(x_none.cpu().numpy(), none64.astype(np.float32))
    tol, err_y = yardstick_lse_tol(x, lse64, dev)
    e_lse = np.abs(lse[0].cpu().double().numpy() - lse64)
    e_pair = np.abs(lse[0].cpu().double().numpy() + lse[1].cpu().double().numpy() - lse64)
    e_cost = np.abs(cost.cpu().double().numpy() - c64)
    print(f"cost pass B={B} Q={Q} L={cap.shape[1]} C={C} ld=C+{extra}: log_softmax err {err_y:.3e}  lse err {e_lse.max():.3e} "
          f"(pair {e_pair.max():.3e})  cost err {e_cost.max():.3e}  bound {tol.min():.3e}")
    assert (e_lse <= tol).all() and (e_pair <= tol).all()
    assert (e_cost <= abs(cost_scale) * tol[..., None]).all()
    for b in range(B):
        assert (cost[b, :, int(n64[b]):] == 0).all()
    return float(e_cost.max())


@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("C", [5, 41, 4099, 10173])
@pytest.mark.parametrize("B", [1, 3])
def test_cost_pass(dev, B, C, extra):
    for Q, L in QL:
        check_cost_pass(make_logits(B, Q, C, seed=Q * 7 + L), make_captions(B, L, C, seed=Q + L + C), extra, dev)


def test_cost_pass_extreme_logits_stay_finite(dev):
    x = make_logits(3, 100, 4099, seed=5)
    x[x > 3] = 80.0
    x[x < -3] = -80.0
    x[0, 0] = -80.0
    x[0, 1] = 80.0
    x[0, 2, :-1] = -80.0
    x[0, 2, -1] = 80.0
    check_cost_pass(x, make_captions(3, 7, 4099, seed=6), 3, dev, cost_scale=2.0)


def test_cost_pass_drops_ids_outside_the_classes(dev):
    from bmhrl_amd import ops
    C = 41
    cap = torch.tensor([[C - 1, 5, -1, C, 7, PAD, 2 ** 40, C - 2], [-7, PAD, C + 100, C - 1, PAD, PAD, -2 ** 40, C]])
    x = make_logits(2, 9, C, seed=8)
    check_cost_pass(x, cap, 3, dev)
    words, n = ops.word_cost(x.to(dev), cap.to(dev), PAD)[:2]
    assert words.cpu().tolist() == [[5, 7, C - 2, -1, -1, -1, -1, -1], [-1] * 8] and n.cpu().tolist() == [3, 0]


# ---------------------------------------------------------------------------------------------- the matcher alone

def matcher_cost(kind, Q, n, seed):
    g = np.random.default_rng(seed)
    if kind == "ties":
        return g.choice(np.array([0, -0.25, -0.5, -1], dtype=np.float32), size=(Q, n))
    if kind == "long_paths":
        return (-(np.arange(Q)[:, None] + 1.0) * (np.arange(n)[None] + 1.0) / (Q * n)).astype(np.float32)
    return g.random((Q, n), dtype=np.float32)


def check_matching(cost, n, qot):
    """one to one, covers every target, total cost (float64 over the fp32 entries) == scipy's optimum within 1e-12"""
    from scipy.optimize import linear_sum_assignment
    for b in range(cost.shape[0]):
        k = int(n[b])
        q = qot[b, :k]
        assert (qot[b, k:] == -1).all()
        assert (q >= 0).all() and (q < cost.shape[1]).all() and len(set(q.tolist())) == k
        if k:
            c64 = cost[b, :, :k].astype(np.float64)
            i, j = linear_sum_assignment(c64)
            assert abs(ref.matching_cost(cost[b], qot[b], k) - c64[i, j].sum()) <= 1e-12


@pytest.mark.parametrize("kind", ["ties", "long_paths", "uniform"])
@pytest.mark.parametrize("Q,n", [(1, 1), (5, 5), (64, 64), (65, 64), (100, 30), (128, 64)])
def test_matcher_is_optimal_and_repeatable(dev, kind, Q, n):
    from bmhrl_amd import ops
    B, L = 3, n
    cost = np.stack([matcher_cost(kind, Q, L, seed=Q * 31 + b) for b in range(B)])
    nn = np.array([n, 0, 1], dtype=np.int32)
    c, k = torch.from_numpy(cost).to(dev), torch.from_numpy(nn).to(dev)
    a = ops.lsa_match(c, k)
    b_ = ops.lsa_match(c, k)
    torch.cuda.synchronize()
    assert torch.equal(a, b_)
    check_matching(cost, nn, a.cpu().numpy())
    # a (B, L, Q) buffer read through strides gives the same matching
    ct = c.transpose(1, 2).contiguous().transpose(1, 2)
    assert ct.stride() != c.stride() or Q == 1 or L == 1
    assert torch.equal(ops.lsa_match(ct, k), a)


# ---------------------------------------------------------------------------------------------- the whole loss

def fixture_cases():
    z = np.load(GOLDEN)
    return [{k: z[f"c{c}_{k}"] for k in ("logits", "captions", "class_map", "loss", "grad", "match_i", "match_j", "match_n")}
            for c in range(int(z["n_cases"]))], float(z["pad_eos"][1])


def torch_yardstick(x, cls, eos, dev):
    """torch's fp32 F.cross_entropy forward and backward on the device with the class map `cls` (B, Q)"""
    C = x.shape[2]
    w = torch.ones(C, device=dev)
    w[-1] = eos
    xt = x.to(dev).clone().requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(xt.transpose(1, 2), torch.from_numpy(cls.astype(np.int64)).to(dev), w)
    loss.backward()
    return float(loss.detach()), xt.grad.cpu().double().numpy()


def check_loss(x, cap, dev, eos=0.1, extra=0, want_cls=None, indices=None):
    """forward + backward through loss_labels against float64 on the device's own class map; returns what it measured"""
    from bmhrl_amd.loss.hungarian_matcher import HungarianMatcher, loss_labels
    B, Q, C = x.shape
    _, xv = in_padded_buffer(x, extra, dev)
    xd = xv.detach().requires_grad_(True)
    loss = loss_labels(xd, cap.to(dev), indices, eos_coef=eos, pad_idx=PAD)
    loss.backward()
    cls, qot, n = (t.cpu().numpy() for t in HungarianMatcher(pad_idx=PAD).match(xv, cap.to(dev)))
    if want_cls is not None:
        assert np.array_equal(cls, want_cls)
    words64, n64 = ref.compact(cap.numpy(), PAD, C)
    assert np.array_equal(n, n64)
    if indices is None:
        assert np.array_equal(cls, ref.class_map(words64, n64, qot, Q, C))
    loss64, grad64 = ref.loss_and_grad(x.numpy(), cls, eos)
    ty_loss, ty_grad = torch_yardstick(x, cls, eos, dev)
    gmax = np.abs(grad64).max()
    tol_loss = max(2 * abs(ty_loss - loss64) / abs(loss64), 2.0 ** -22)
    tol_grad = max(2 * np.abs(ty_grad - grad64).max() / gmax, 2.0 ** -22)
    loss = loss.detach()
    e_loss = abs(float(loss) - loss64) / abs(loss64)
    e_grad = np.abs(xd.grad.cpu().double().numpy() - grad64).max() / gmax
    print(f"loss B={B} Q={Q} L={cap.shape[1]} C={C} ld=C+{extra}: loss err {e_loss:.3e} (torch {abs(ty_loss - loss64) / abs(loss64):.3e}, "
          f"bound {tol_loss:.3e})  grad err {e_grad:.3e} (torch {np.abs(ty_grad - grad64).max() / gmax:.3e}, bound {tol_grad:.3e})")
    assert e_loss <= tol_loss and e_grad <= tol_grad
    return float(loss), xd.grad, cls, (loss64, grad64, tol_loss, tol_grad)


def test_whole_loss_against_the_reference_fixture(dev):
    from bmhrl_amd.loss.hungarian_matcher import HungarianMatcher, loss_labels
    cases, eos = fixture_cases()
    assert len(cases) >= 2
    for c in cases:
        x, cap = torch.from_numpy(c["logits"].astype(np.float32)), torch.from_numpy(c["captions"])
        B, Q, C = x.shape
        loss, grad, cls, (loss64, grad64, tol_loss, tol_grad) = check_loss(x, cap, dev, eos, want_cls=c["class_map"])
        # against the fixture itself: our bound plus the fp32 reference's own distance from float64
        f_loss, f_grad = float(c["loss"]), c["grad"].astype(np.float64)
        gmax = np.abs(grad64).max()
        assert abs(loss - f_loss) / abs(loss64) <= tol_loss + abs(f_loss - loss64) / abs(loss64)
        assert np.abs(grad.cpu().double().numpy() - f_grad).max() / gmax <= tol_grad + np.abs(f_grad - grad64).max() / gmax
        # the all-pad sample: every query is "no word" and its rows carry weight eos
        b0 = int(np.nonzero(c["match_n"] == 0)[0][0]) if (c["match_n"] == 0).any() else None
        if b0 is not None:
            assert (cls[b0] == C - 1).all()
            p = torch.softmax(x[b0].double(), -1).numpy()
            p[:, -1] -= 1.0
            den = eos * (cls == C - 1).sum() + (cls != C - 1).sum()
            assert np.abs(grad[b0].cpu().double().numpy() - eos / den * p).max() / gmax <= tol_grad
        # the reference's tuples score to the same loss, bit for bit (the same class map through the same launches)
        idx = [(torch.from_numpy(c["match_i"][b, :k]), torch.from_numpy(c["match_j"][b, :k])) for b, k in enumerate(c["match_n"])]
        xd = x.to(dev)
        assert torch.equal(loss_labels(xd, cap.to(dev), idx, eos_coef=eos), loss_labels(xd, cap.to(dev), None, eos_coef=eos))
        # forward(): scipy's form -- ascending index_i, int64 CPU tensors -- and the fixture's class map
        got = HungarianMatcher()(xd, cap.to(dev))
        words64, n64 = ref.compact(c["captions"], PAD, C)
        again = np.full((B, Q), C - 1, dtype=np.int32)
        for b, (i, j) in enumerate(got):
            assert i.dtype == torch.int64 and j.dtype == torch.int64 and not i.is_cuda and len(i) == len(j) == n64[b]
            assert (i[1:] > i[:-1]).all()
            again[b, i.numpy()] = words64[b, j.numpy()]
        assert np.array_equal(again, c["class_map"])


@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("C", [5, 41, 4099, 10173])
@pytest.mark.parametrize("B", [1, 3])
def test_whole_loss_against_float64(dev, B, C, extra):
    for L in (1, 7, 64):
        check_loss(make_logits(B, 100, C, seed=L + C), make_captions(B, L, C, seed=3 * L + C + B), dev, extra=extra)


def test_two_runs_give_equal_bits_and_padding_columns_are_kept(dev):
    from bmhrl_amd import ops
    from bmhrl_amd.loss.hungarian_matcher import loss_labels
    B, Q, C, L = 3, 100, 4099, 7
    x, cap = make_logits(B, Q, C, seed=21), make_captions(B, L, C, seed=22).to(dev)
    _, xv = in_padded_buffer(x, 3, dev)
    runs = []
    for _ in range(2):
        xd = xv.detach().requires_grad_(True)
        loss = loss_labels(xd, cap)
        loss.backward()
        runs.append((loss.detach().clone(), xd.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    # the gradient written into a padded buffer: the padding columns keep their sentinel
    words, n, lse, x_none, gathered, cost = ops.word_cost(xv, cap, PAD)
    tgt, row_w, ls = ops.word_loss(words, n, ops.lsa_match(cost, n), lse, x_none, gathered, 0.1, C)
    obuf = torch.full((B, Q, C + 3), -7.5, device=dev)
    ops.word_loss_bwd(xv, lse, tgt, row_w, ls, None, out=obuf[:, :, :C])
    assert (obuf[:, :, C:] == -7.5).all() and torch.equal(obuf[:, :, :C], runs[0][1])
    # an incoming gradient scales it: g = 0.5 halves every entry exactly
    half = ops.word_loss_bwd(xv, lse, tgt, row_w, ls, torch.tensor([0.5], device=dev))
    assert torch.equal(half, runs[0][1] * 0.5)


# ---------------------------------------------------------------------------------------------- optimality under the device's rounding

@pytest.mark.parametrize("B,Q,L,C,seed", [(3, 100, 30, 41, 1), (3, 100, 30, 173, 2), (2, 128, 64, 4099, 3), (3, 5, 5, 5, 4),
                                         (2, 100, 12, 10173, 5)])
def test_matching_is_optimal_within_the_device_rounding(dev, B, Q, L, C, seed):
    from bmhrl_amd import ops
    from scipy.optimize import linear_sum_assignment
    x, cap = make_logits(B, Q, C, seed), make_captions(B, L, C, seed + 50, p_pad=0.15)
    words, n, lse, x_none, gathered, cost = ops.word_cost(x.to(dev), cap.to(dev), PAD)
    qot = ops.lsa_match(cost, n).cpu().numpy()
    c64 = ref.cost_pass(x.numpy(), cap.numpy(), PAD)[5]
    eps = float(np.abs(cost.cpu().double().numpy() - c64).max())
    n = n.cpu().numpy()
    check_matching(cost.cpu().numpy(), n, qot)
    for b in range(B):
        k = int(n[b])
        if k:
            i, j = linear_sum_assignment(c64[b, :, :k])
            got = ref.matching_cost(c64[b], qot[b], k)
            print(f"B={B} Q={Q} C={C} sample {b}: n={k} eps={eps:.3e} cost gap {got - c64[b, :, :k][i, j].sum():.3e}")
            assert got - c64[b, :, :k][i, j].sum() <= 2 * k * eps


# ---------------------------------------------------------------------------------------------- refusals

def test_refusals_return_22_and_launch_nothing(dev):
    from bmhrl_amd import _lib
    lib = _lib.load()
    B, Q, L, C = 2, 8, 4, 16
    S = -3.0
    x = torch.randn(B * Q, C, device=dev)
    cap = torch.randint(2, C - 1, (B, L), device=dev)
    words, nw, qot, tgt = (torch.full(s, -9, dtype=torch.int32, device=dev) for s in ((B, L), (B,), (B, L), (B, Q)))
    lse, lo, none, row_w = (torch.full((B, Q), S, device=dev) for _ in range(4))
    gath, cost = torch.full((B, Q, L), S, device=dev), torch.full((B, Q, L), S, device=dev)
    ls, dx = torch.full((2,), S, device=dev), torch.full((B * Q, C), S, device=dev)
    p = lambda t: t.data_ptr()                                                                # noqa: E731
    st = torch.cuda.current_stream().cuda_stream

    def cost_call(x_=p(x), ld=C, cap_=p(cap), ldc=L, B_=B, Q_=Q, L_=L, C_=C, words_=p(words), lse_=p(lse)):
        return lib.bmhrl_word_cost(x_, ld, cap_, ldc, PAD, 1.0, B_, Q_, L_, C_, words_, p(nw), lse_, p(lo), p(none), p(gath), p(cost), st)

    def match_call(c_=p(cost), n_=p(nw), B_=B, Q_=Q, L_=L, out_=p(qot)):
        return lib.bmhrl_lsa_match(c_, Q * L, L, 1, n_, B_, Q_, L_, out_, st)

    def loss_call(w_=p(words), B_=B, Q_=Q, L_=L, C_=C, ls_=p(ls)):
        return lib.bmhrl_word_loss(w_, p(nw), p(qot), p(lse), p(lo), p(none), p(gath), 0.1, B_, Q_, L_, C_, p(tgt), p(row_w), ls_, st)

    def bwd_call(x_=p(x), ld=C, ldd=C, B_=B, Q_=Q, C_=C, dx_=p(dx)):
        return lib.bmhrl_word_loss_bwd(x_, ld, p(lse), p(lo), p(tgt), p(row_w), p(ls), None, dx_, ldd, B_, Q_, C_, st)

    bad = [cost_call(x_=None), cost_call(cap_=None), cost_call(words_=None), cost_call(lse_=None), cost_call(B_=0), cost_call(Q_=0),
           cost_call(L_=0), cost_call(C_=0), cost_call(C_=1), cost_call(Q_=129), cost_call(L_=65, Q_=100), cost_call(L_=Q + 1),
           cost_call(ld=C - 1), cost_call(B_=-1),
           match_call(c_=None), match_call(n_=None), match_call(out_=None), match_call(B_=0), match_call(Q_=0), match_call(L_=0),
           match_call(Q_=129), match_call(L_=65, Q_=100), match_call(L_=Q + 1),
           loss_call(w_=None), loss_call(ls_=None), loss_call(B_=0), loss_call(Q_=0), loss_call(L_=0), loss_call(C_=1),
           loss_call(Q_=129), loss_call(L_=65, Q_=100), loss_call(L_=Q + 1),
           bwd_call(x_=None), bwd_call(dx_=None), bwd_call(B_=0), bwd_call(Q_=0), bwd_call(C_=1), bwd_call(Q_=129),
           bwd_call(ld=C - 1), bwd_call(ldd=C - 1)]
    torch.cuda.synchronize()
    assert bad == [-22] * len(bad)
    for t in (words, nw, qot, tgt):
        assert (t == -9).all()
    for t in (lse, lo, none, row_w, gath, cost, ls, dx):
        assert (t == S).all()
    assert cost_call() == 0 and match_call() == 0 and loss_call() == 0 and bwd_call() == 0          # the same calls, valid
    torch.cuda.synchronize()
    assert (dx != S).all() and torch.isfinite(ls).all()


# ---------------------------------------------------------------------------------------------- captured launches

def test_captured_launches_replay_on_new_contents(dev):
    """launches 1-4 in one graph, at the ops level under no_grad (no autograd graph is alive at capture: DESIGN.md section
    10); the logits and captions are overwritten in place between replays"""
    from bmhrl_amd import ops
    B, Q, C, L = 3, 100, 173, 12
    xs = [make_logits(B, Q, C, seed=s).to(dev) for s in (31, 32)]
    caps = [make_captions(B, L, C, seed=s).to(dev) for s in (33, 34)]

    def run(x, cap):
        words, n, lse, x_none, gathered, cost = ops.word_cost(x, cap, PAD)
        qot = ops.lsa_match(cost, n)
        tgt, row_w, ls = ops.word_loss(words, n, qot, lse, x_none, gathered, 0.1, C)
        return ls, ops.word_loss_bwd(x, lse, tgt, row_w, ls), tgt

    with torch.no_grad():
        eager = [tuple(t.clone() for t in run(x, c)) for x, c in zip(xs, caps)]
        assert not torch.equal(eager[0][2], eager[1][2])
        x, cap = xs[0].clone(), caps[0].clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            run(x, cap)                     # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = run(x, cap)
        for k in (1, 0, 1):
            x.copy_(xs[k])
            cap.copy_(caps[k])
            g.replay()
            torch.cuda.synchronize()
            for got, want in zip(out, eager[k]):
                assert torch.equal(got, want)
        del g


# ---------------------------------------------------------------------------------------------- through the agent

def tiny_detr_agent(dev):
    """the tiny DetrCaption of tests/test_detr_agent_gpu.py (same builder, random state), V = 41, in train mode, no dropout"""
    from types import SimpleNamespace
    from bmhrl_amd import synthetic as syn
    from bmhrl_amd.model.det_bmhrl_agent import DetrCaption
    cfg = syn.tiny_cfg(d_model=64, d_model_video=64, d_vid=64, d_model_caps=20, rl_att_heads=4, rl_goal_d=8, dout_p=0.0)
    cfg.pre_goal_attention = False
    cfg.device = str(dev)
    agent = DetrCaption(cfg, SimpleNamespace(trg_voc_size=41, train_vocab=SimpleNamespace(vectors=None)))
    shapes = {k: tuple(v.shape) for k, v in agent.state_dict().items()}
    sd = syn.fill_state_dict({k: s for k, s in shapes.items() if not k.startswith("critic.")}, seed=13)
    sd.update({"critic." + k: v for k, v in syn.synthetic_critic_state(20, seed=1).items()})
    for leaf in ("weight", "bias"):
        sd[f"worker_decoder.norm.{leaf}"] = sd[f"manager_decoder.norm.{leaf}"]
    agent.load_state_dict(sd)
    return agent.to(dev).train(), cfg


def test_loss_through_the_detr_agent(dev, golden):
    from bmhrl_amd.loss.hungarian_matcher import HungarianMatcher, loss_labels
    g = golden("detr_agent")
    agent, cfg = tiny_detr_agent(dev)
    x, mask = torch.from_numpy(g["x_video"]).to(dev)[:2], torch.from_numpy(g["V_mask"]).to(dev)[:2]
    B, L = x.shape[0], 7
    assert B == 2
    trg = torch.randint(4, 41, (B, L), generator=torch.Generator().manual_seed(3))
    trg[0, 5] = 3
    trg[0, 6:] = 1
    c_mask = ((trg != 1).unsqueeze(1) & torch.ones(L, L, dtype=torch.bool).tril().unsqueeze(0))
    out = agent((x, None), trg.to(dev), {"V_mask": mask, "C_mask": c_mask.to(dev)})
    logits = out[5]
    assert logits.shape == (B, 100, 42)
    logits.retain_grad()
    loss_labels(logits, trg.to(dev)).backward()
    for w in (agent.object_detector.class_embed.weight, agent.input_proj[0][0].weight):
        assert w.grad is not None and torch.isfinite(w.grad).all() and float(w.grad.abs().max()) > 0
    xl = logits.detach().float().cpu()
    cls = HungarianMatcher().match(logits, trg.to(dev))[0].cpu().numpy()
    loss64, grad64 = ref.loss_and_grad(xl.numpy(), cls, 0.1)
    _, ty_grad = torch_yardstick(xl, cls, 0.1, dev)
    gmax = np.abs(grad64).max()
    tol = max(2 * np.abs(ty_grad - grad64).max() / gmax, 2.0 ** -22)
    err = np.abs(logits.grad.cpu().double().numpy() - grad64).max() / gmax
    print(f"agent: grad err {err:.3e} (bound {tol:.3e})")
    assert err <= tol
