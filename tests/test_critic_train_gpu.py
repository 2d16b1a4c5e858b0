"""Training the segment critic on the device (csrc/critic_train.hip, functional.SegmentCriticFn, critic_train.CriticTrainer)
against the float64 CPU oracle of tests/critic_reference.py.  The yardstick E of a case is the worst relative gradient
error of the SAME oracle in float32 on the CPU; the device must stay within 8 E (three bits for the different summation
order: MFMA k slices, per-block partials, sums over the B*L rows)."""
import functools

import pytest
import torch

from bmhrl_amd import synthetic as syn

from tests import critic_reference as R

pytestmark = pytest.mark.gpu

PW = 3.0
PAD = 1
# (d_caps, B, L): real width with a partial unit tile and a partial batch tile; two batch tiles; no recurrence (every
# weight_hh gradient is exactly 0); full caption length
CASES = [(300, 3, 5), (300, 17, 2), (12, 17, 1), (12, 2, 30)]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _critic(d, state, dev):
    from bmhrl_amd.model.bm_hrl_agent import SegmentCritic
    c = SegmentCritic(syn.default_cfg(d_model_caps=d))
    c.load_state_dict(state)
    return c.to(dev).unfreeze()


def _device_run(d, state, emb, labels, mask, emb_grad=True):
    """(loss, score, {name: grad}) of the package on the device"""
    dev = _dev()
    c = _critic(d, state, dev)
    x = emb.to(dev).requires_grad_(emb_grad)
    loss, score = c.masked_bce(x, labels.to(dev), mask.to(dev), PW)
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in c.named_parameters()}
    if emb_grad:
        grads["emb"] = x.grad.detach().clone()
    return loss.detach(), score.detach(), grads


@functools.lru_cache(maxsize=None)
def _case(d, B, L, alpha=None):
    """inputs, the float64 oracle, the float32 yardstick and the device result of one case (computed once, shared)"""
    state = R.random_state(d, seed=d + B + L)
    if alpha is not None:
        # float64, so that each precision gets its own nearest value: at alpha = 0.99 the oracle sits ON the end of the clamp
        # in float64 as the float32 runs do in float32 (float32(0.99) widened to float64 would lie outside it)
        state["relu.alpha"] = torch.tensor([alpha], dtype=torch.float64)
        state["relu2.alpha"] = torch.tensor([alpha], dtype=torch.float64)
    emb, tokens, labels = R.random_case(d, B, L, seed=B * 100 + L, pad_idx=PAD)
    mask = tokens != PAD
    l64, s64, g64 = R.loss_and_grads(state, emb, labels, mask, PW, torch.float64, emb_grad=True)
    l32, s32, g32 = R.loss_and_grads(state, emb, labels, mask, PW, torch.float32, emb_grad=True)
    E = max(R.rel_err(g32[n], g64[n]) for n in g64)
    assert 0.0 < E < 1e-3, f"yardstick E = {E}: the float32 oracle disagrees with the float64 one"
    dev_out = _device_run(d, state, emb, labels, mask)
    return dict(state=state, emb=emb, tokens=tokens, labels=labels, mask=mask, l64=l64, s64=s64, g64=g64, E=E, dev=dev_out)


def _check_grads(c, what):
    _, _, g = c["dev"]
    errs = {n: R.rel_err(g[n], c["g64"][n]) for n in c["g64"]}
    worst = max(errs, key=errs.get)
    print(f"{what}: worst err {errs[worst]:.3e} ({worst}), E {c['E']:.3e}, err / E {errs[worst] / c['E']:.2f}")
    assert set(g) == set(R.PARAM_NAMES) | {"emb"} and len(R.PARAM_NAMES) == 30
    for n, e in errs.items():
        assert e <= 8 * c["E"], f"{n}: err {e:.3e} > 8 E = {8 * c['E']:.3e}"


@pytest.mark.parametrize("d,B,L", CASES)
def test_gradient_parity(d, B, L):
    """all 30 parameter gradients and the embedding gradient: max|g_dev - g_64| / max|g_64| <= 8 E"""
    c = _case(d, B, L)
    _check_grads(c, f"(d {d}, B {B}, L {L})")
    if L == 1:                                  # no recurrence: the oracle's weight_hh gradients are exactly 0
        for n in R.PARAM_NAMES:
            if "weight_hh" in n:
                assert float(c["g64"][n].abs().max()) == 0.0 and float(c["dev"][2][n].abs().max()) == 0.0, n


@pytest.mark.parametrize("d,B,L", CASES)
def test_forward_parity(d, B, L):
    dev = _dev()
    c = _case(d, B, L)
    loss, score, _ = c["dev"]
    crit = _critic(d, c["state"], dev)
    x = c["emb"].to(dev)
    s_fn = crit.score(x).detach()
    s_inf = crit.score_and_labels(x, 0.5)[0]
    assert torch.equal(s_fn, score)                                   # head + loss launch == plain head
    bound = max(1.0, float(s_inf.abs().max()))
    assert float((s_fn - s_inf).abs().max()) <= 1e-5 * bound          # the two forward schedules
    ref = c["s64"]
    d64 = float((s_fn.cpu().double() - ref).abs().max())
    assert d64 <= 2e-5 * max(1.0, float(ref.abs().max()))
    rel = abs(float(loss.cpu().double() - c["l64"])) / abs(float(c["l64"]))
    print(f"(d {d}, B {B}, L {L}): score err {d64:.3e}, loss rel err {rel:.3e}, E {c['E']:.3e}")
    assert rel <= 8 * c["E"]


def _same_bits(a, b):
    la, sa, ga = a
    lb, sb, gb = b
    assert torch.equal(la, lb) and torch.equal(sa, sb)
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n


def test_masked_positions_do_not_matter():
    """flipping the labels under the mask leaves the loss and every gradient bit-identical"""
    d, B, L = CASES[0]
    c = _case(d, B, L)
    assert int((~c["mask"]).sum()) > 0
    flipped = torch.where(c["mask"], c["labels"], 1.0 - c["labels"])
    _same_bits(c["dev"], _device_run(d, c["state"], c["emb"], flipped, c["mask"]))


@pytest.mark.parametrize("d,B,L", [CASES[1], CASES[3]])
def test_two_runs_agree_bit_for_bit(d, B, L):
    c = _case(d, B, L)
    _same_bits(c["dev"], _device_run(d, c["state"], c["emb"], c["labels"], c["mask"]))


def test_score_backward_through_autograd():
    """the score-only call (head backward from autograd's dscore) gives the gradients of the fused head + loss call"""
    dev = _dev()
    d, B, L = CASES[0]
    c = _case(d, B, L)
    crit = _critic(d, c["state"], dev)
    score = crit.score(c["emb"].to(dev))
    m = c["mask"].to(dev).float()
    l = torch.nn.functional.binary_cross_entropy_with_logits(score.squeeze(-1), c["labels"].to(dev), reduction="none",
                                                            pos_weight=torch.tensor(PW, device=dev))
    ((l * m).sum() / m.sum()).backward()
    for n, p in crit.named_parameters():
        assert R.rel_err(p.grad, c["g64"][n]) <= 8 * c["E"], n


def test_needs_input_grad_is_honoured():
    dev = _dev()
    d, B, L = 12, 3, 5
    c = _case(d, B, L)
    crit = _critic(d, c["state"], dev)
    crit.freeze()
    crit.lin.weight.requires_grad = True
    crit.gru.weight_hh_l0.requires_grad = True
    loss, _ = crit.masked_bce(c["emb"].to(dev), c["labels"].to(dev), c["mask"].to(dev), PW)
    loss.backward()
    got = {n for n, p in crit.named_parameters() if p.grad is not None}
    assert got == {"lin.weight", "gru.weight_hh_l0"}
    for n in got:
        assert torch.equal(dict(crit.named_parameters())[n].grad, c["dev"][2][n])


@pytest.mark.parametrize("alpha", [0.995, 0.99, 0.5])
def test_arelu_ends(alpha):
    """outside the clamp dalpha is exactly 0; at the end 0.99 torch's clamp passes the gradient, and so does the device"""
    c = _case(12, 2, 30, alpha)
    _check_grads(c, f"alpha {alpha}")
    for n in ("relu.alpha", "relu2.alpha"):
        g = float(c["dev"][2][n])
        if alpha > 0.99:
            assert g == 0.0 and float(c["g64"][n]) == 0.0
        else:
            assert g != 0.0 and float(c["g64"][n]) != 0.0


def _learning_problem(dev, seed=0):
    from bmhrl_amd.critic_train import CriticTrainer
    from bmhrl_amd.model.bm_hrl_agent import SegmentCritic
    torch.manual_seed(seed)
    crit = SegmentCritic(syn.default_cfg(d_model_caps=12)).to(dev)
    g = torch.Generator().manual_seed(seed)
    table = torch.randn(20, 12, generator=g).to(dev)
    tokens = torch.randint(2, 20, (8, 6), generator=g)
    tokens[5:, 4:] = PAD
    labels = torch.zeros(8, 6)
    labels[:, 2] = 1.0
    labels[:, 5] = 1.0
    tr = CriticTrainer(crit, lambda tok: table[tok], PAD, lr=1e-2, pos_weight=None)
    return tr, crit, table, tokens.to(dev), labels.to(dev)


def test_it_learns():
    """60 steps on 8 sequences of 6 tokens: loss < 0.05 and every valid label right at threshold 0.5 through evaluate()"""
    dev = _dev()
    tr, crit, _, tokens, labels = _learning_problem(dev)
    losses = [tr.step(tokens, labels) for _ in range(60)]
    assert losses[-1].dim() == 0 and losses[-1].is_cuda
    last = float(losses[-1])
    ev = tr.evaluate(tokens, labels, 0.5)
    print(f"first loss {float(losses[0]):.4f}, last loss {last:.3e}, evaluate {ev}")
    assert last < 0.05
    assert ev["precision"] == 1.0 and ev["recall"] == 1.0 and ev["f1"] == 1.0
    tr.close()
    assert not any(p.requires_grad for p in crit.parameters())


def test_checkpoint_round_trip(tmp_path):
    from bmhrl_amd.model.bm_hrl_agent import SegmentCritic
    dev = _dev()
    tr, crit, table, tokens, labels = _learning_problem(dev, seed=1)
    means = tr.fit(tokens, labels, epochs=2, batch_size=3, seed=5)
    assert len(means) == 2 and all(m == m for m in means)
    path = str(tmp_path / "critic.cp")
    tr.save(path)
    loaded = SegmentCritic(syn.default_cfg(d_model_caps=12, rl_critic_path=path)).to(dev)
    assert not any(p.requires_grad for p in loaded.parameters())
    assert list(loaded.state_dict()) == list(torch.load(path))
    emb = table[tokens]
    assert torch.equal(loaded.score_and_labels(emb, 0.5)[1], crit.score_and_labels(emb, 0.5)[1])
    assert torch.equal(loaded.score_and_labels(emb, 0.5)[0], crit.score_and_labels(emb, 0.5)[0])


def test_refusals():
    """every invalid-argument case of the new entry points returns -22"""
    from bmhrl_amd import _lib, ops
    dev = _dev()
    B, L, H = 2, 3, 8
    f = lambda *s: torch.zeros(*s, device=dev)
    xp4, xp3, w4, w3 = f(B * L, 4 * H), f(B * L, 3 * H), f(4 * H, H), f(3 * H, H)
    seq, carry, b3 = f(B * L, H), f(B, H), f(3 * H)

    def refused(fn, *a, **k):
        with pytest.raises(_lib.HipError, match="invalid argument -22"):
            fn(*a, **k)

    fwd4 = lambda **o: ops.rnn_step_train(4, *[o.get(k, v) for k, v in dict(xproj=xp4, whh=w4, bhh=None, h_seq=seq, hprev=seq.clone(), c_seq=seq.clone(),
                                          gate_seq=xp4.clone(), hn_seq=None, y_seq=None, a=None, b=None, B=B, L=L, H=H, t=0).items()])
    fwd4()                                                                       # (the valid call goes through)
    for bad in (dict(xproj=None), dict(whh=None), dict(h_seq=None), dict(hprev=None), dict(c_seq=None), dict(gate_seq=None), dict(B=0),
                dict(L=0), dict(H=0), dict(H=644), dict(H=6), dict(t=L), dict(a=f(1))):
        refused(fwd4, **bad)
    refused(ops.rnn_step_train, 3, xp3, w3, None, seq, seq.clone(), None, xp3.clone(), seq.clone(), None, None, None, B, L, H, 0)   # GRU: b_hh
    refused(ops.rnn_step_train, 3, xp3, w3, b3, seq, seq.clone(), None, xp3.clone(), None, None, None, None, B, L, H, 0)            # GRU: hn_seq
    refused(ops.rnn_step_train, 4, xp4, w4, None, seq, seq.clone(), seq.clone(), xp4.clone(), None, None, f(1), f(1), B, L, H, 0)   # AReLU: y_seq
    bwd4 = lambda **o: ops.rnn_bwd_step(4, *[o.get(k, v) for k, v in dict(whh=w4, dy=seq, h_seq=seq, c_seq=seq, gate_seq=xp4, hn_seq=None,
                                        carry=carry, dax=xp4.clone(), dah=None, a=None, b=None, B=B, L=L, H=H, t=L - 1).items()])
    bwd4()
    for bad in (dict(whh=None), dict(dy=None), dict(h_seq=None), dict(c_seq=None), dict(gate_seq=None), dict(carry=None), dict(dax=None),
                dict(B=0), dict(L=0), dict(H=0), dict(H=644), dict(H=6), dict(t=-1), dict(b=f(1))):
        refused(bwd4, **bad)
    refused(ops.rnn_bwd_step, 3, w3, seq, seq, None, xp3, None, carry, xp3.clone(), xp3.clone(), None, None, B, L, H, 0)  # GRU: hn_seq
    refused(ops.rnn_bwd_step, 3, w3, seq, seq, None, xp3, seq, carry, xp3.clone(), None, None, None, B, L, H, 0)          # GRU: dah
    A, Bm, Cm = f(8, 8), f(8, 8), f(8, 8)
    ops.gemm_f32_nn(A, Bm, Cm, 8, 8, 8)
    for bad in ((None, Bm, Cm, 8, 8, 8), (A, None, Cm, 8, 8, 8), (A, Bm, None, 8, 8, 8), (A, Bm, Cm, 0, 8, 8), (A, Bm, Cm, 8, 0, 8),
                (A, Bm, Cm, 8, 8, 0), (A, Bm, Cm, 8, 8, 6)):                   # (K = 6: an input width that is no multiple of 4)
        refused(ops.gemm_f32_nn, *bad)
    refused(ops.gemm_f32, f(4, 6), f(8, 6), None, None, f(4, 8), 4, 8, 6)        # the forward's input projection: width % 4
    refused(ops.rnn_bias_grad, None, None, b3, None, B * L, 3 * H)
    refused(ops.rnn_bias_grad, xp3, None, None, None, B * L, 3 * H)
    refused(ops.rnn_bias_grad, xp3, xp3, b3, None, B * L, 3 * H)
    refused(ops.rnn_bias_grad, xp3, None, b3, None, 0, 3 * H)
    refused(ops.arelu_grad, None, seq, f(1), f(1), f(1), f(1), B * L * H)
    refused(ops.arelu_grad, seq, seq, f(1), f(1), f(1), None, B * L * H)
    refused(ops.arelu_grad, seq, seq, f(1), f(1), f(1), f(1), 0)
    rows = B * L
    head = lambda **o: ops.critic_head_loss(*[o.get(k, v) for k, v in dict(
        y2=seq, w=f(1, H), b=f(1), labels=f(rows), mask=torch.ones(rows, dtype=torch.bool, device=dev), pw=1.0, ds_in=None, score=f(rows),
        loss=f(1), ds=f(rows), dy2=seq.clone(), dw=f(1, H), db=f(1), rows=rows, H=H).items()])
    head()
    for bad in (dict(y2=None), dict(w=None), dict(b=None), dict(mask=None), dict(loss=None), dict(ds=None), dict(dy2=None), dict(dw=None),
                dict(db=None), dict(rows=0), dict(H=0), dict(H=644), dict(labels=None)):   # (no labels and no ds_in)
        refused(head, **bad)
    torch.cuda.synchronize()
