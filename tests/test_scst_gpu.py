"""Self-critical training on sampled rollouts end to end (bmhrl_amd/scst.py, epoch_loops/captioning_scst_loops.py): the agent
of test_sample_decoder_against_teacher_forcing_and_rerun (dropout 0, V = 200, B = 3 clips of 64 video / 200 audio frames,
max_len 10) with n = 3 rollouts per clip.  The loss against torch's own expression on the same prediction tensor under the
bound of tests/test_loss_paths_gpu.py (float32 torch on the device is the yardstick: twice its error or 2^-22 of the largest
magnitude), the rollout's log-probs against the training forward, the decoders' weight shadows after an optimizer step, and
the loop over two capacity buckets."""
from types import SimpleNamespace

import pytest
import torch

from bmhrl_amd import synthetic as syn
from tests.test_decode_gpu import _agent
from tests.test_loss_paths_gpu import check
from tests.test_sample_gpu import END, PAD, START, _batch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
V, B, TV, TA, L, N = 200, 3, 64, 200, 10, 3


def _mk_agent():
    return _agent(torch.device(DEV), V, rl_critic_score_threshhold=0.5)


@pytest.fixture(scope="module")
def case():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bmhrl_amd import scst
    agent = _mk_agent()
    fs = _batch(B, TV, TA, V, 4)
    ro = scst.rollout(agent, fs, L, START, END, PAD, "audio_video", n=N, seed=77)
    assert ro.toks.shape == (B * N, ro.m + 1) and ro.step_logp.shape == (B * N, ro.m) and 1 <= ro.m <= L and ro.n == N
    assert not agent.training                               # the previous mode is restored
    return agent, fs, ro


def _live(ro):
    t = ro.toks[:, 1:]
    is_end = t == END
    return (is_end.cumsum(1) - is_end.long()) == 0


def _train_forward(agent, fs, ro):
    from bmhrl_amd.epoch_loops.captioning_scst_loops import rollout_forward
    agent.train()
    agent.teach_worker()
    agent.zero_grad(set_to_none=True)
    return rollout_forward(agent, fs, ro, "audio_video", PAD)


def test_constant_scores_with_the_mean_baseline_give_exactly_zero(case):
    from bmhrl_amd import scst
    from bmhrl_amd.epoch_loops.captioning_scst_loops import off_default_stream
    agent, fs, ro = case
    scores = torch.full((B * N, ro.m), 0.37, dtype=torch.float64, device=DEV)
    with off_default_stream(torch.device(DEV)):
        pred = _train_forward(agent, fs, ro)
        loss, stats = scst.self_critical_loss(pred, ro, scores, baseline="mean")
        loss.backward()
        assert float(loss.detach()) == 0.0
        st = stats.tolist()
        assert abs(st[0] - 0.37) < 1e-15 and abs(st[1] - 0.37) < 1e-15 and st[3] == float(_live(ro).sum())
        n_grads = 0
        for name, p in agent.named_parameters():
            if p.grad is not None:
                n_grads += 1
                assert not bool(p.grad.any()), name
        assert n_grads > 20
        del pred, loss
    agent.eval()


def test_unit_scores_without_baseline_equal_the_mean_log_prob(case):
    from bmhrl_amd import scst
    from bmhrl_amd.epoch_loops.captioning_scst_loops import off_default_stream
    agent, fs, ro = case
    scores = torch.ones(B * N, ro.m, dtype=torch.float64, device=DEV)
    live = _live(ro)
    n_tok = int(live.sum())
    a = ro.toks[:, 1:].unsqueeze(-1)
    with off_default_stream(torch.device(DEV)):
        pred = _train_forward(agent, fs, ro)
        pred.retain_grad()
        loss, stats = scst.self_critical_loss(pred, ro, scores, baseline="none", clip=0.0, entropy=0.0)
        loss.backward()
        assert stats.tolist() == [1.0, 0.0, n_tok / (B * N), float(n_tok)]
        out = {}
        for tag, dt in (("ref", torch.float64), ("yard", torch.float32)):
            x = pred.detach().to(dt).requires_grad_(True)
            l = -(x.gather(-1, a).squeeze(-1) * live.to(dt)).sum() / n_tok
            l.backward()
            out[tag] = (l.detach(), x.grad)
        check("scst", "loss, scores 1, no baseline", loss.detach(), out["ref"][0], out["yard"][0])
        check("scst", "d loss / d prediction", pred.grad, out["ref"][1], out["yard"][1])
        frozen = [p for m in agent.manager_modules for p in m.parameters()]
        assert frozen and all(p.grad is None for p in frozen)
        got = {k: p.grad for k, p in agent.named_parameters() if p.grad is not None}
        assert len(got) > 20 and all(bool(torch.isfinite(g).all()) for g in got.values())
        assert any(bool(g.any()) for g in got.values())
        # the trainable parameters: exactly those torch's own expression of the loss reaches on a second forward
        pred2 = _train_forward(agent, fs, ro)
        (-(pred2.gather(-1, a).squeeze(-1) * live.float()).sum() / n_tok).backward()
        want = {k for k, p in agent.named_parameters() if p.grad is not None}
        assert set(got) == want
        assert any(k.startswith("worker.") for k in want) and any(k.startswith("bm_enc.") for k in want)
        del pred, pred2, loss, out, x, l
    agent.zero_grad(set_to_none=True)
    agent.eval()


def test_eval_forward_reproduces_the_rollout_log_probs(case):
    """the clipped ratio starts at 1: |logp[a] - step_logp| < 1e-3 on live steps, the bound tests/test_sample_gpu.py asserts
    for the same quantity"""
    from bmhrl_amd.epoch_loops.captioning_scst_loops import rollout_forward
    agent, fs, ro = case
    agent.eval()
    agent.set_inference_mode(True)                          # exploration off
    with torch.no_grad():
        pred = rollout_forward(agent, fs, ro, "audio_video", PAD).float()
    lp = pred.gather(-1, ro.toks[:, 1:].unsqueeze(-1)).squeeze(-1)
    live = _live(ro)
    err = float(((lp - ro.step_logp).abs() * live).max())
    print(f"max |logp[a] - rollout step_logp| on {int(live.sum())} live steps: {err:.3e}")
    assert err < 1e-3, err
    assert bool((ro.step_logp[~live] == 0).all()) and bool((ro.toks[:, 1:][~live] == PAD).all())


def _score_fn(hyp, captions):
    """a synthetic per-prefix reward: the running share of tokens with an even id"""
    even = (hyp % 2 == 0).double().cumsum(1)
    return even / torch.arange(1, hyp.shape[1] + 1, device=hyp.device, dtype=torch.float64)


def test_rollout_after_an_optimizer_step_equals_a_fresh_agent(case):
    """the cached decoders re-cast their weight shadows when the parameters change: tokens and step log-probs of a seeded
    rollout after one step equal, bit for bit, those of a freshly built agent loaded with the updated state dict"""
    from bmhrl_amd import scst
    from bmhrl_amd.epoch_loops.captioning_scst_loops import off_default_stream
    _, fs, _ = case
    agent = _mk_agent()
    opt = torch.optim.Adam([p for p in agent.parameters()], lr=1e-3)
    ro = scst.rollout(agent, fs, L, START, END, PAD, "audio_video", n=N, seed=5)        # (the decoder exists before the step)
    with off_default_stream(torch.device(DEV)):
        pred = _train_forward(agent, fs, ro)
        loss, _ = scst.self_critical_loss(pred, ro, _score_fn(ro.toks[:, 1:], None), baseline="mean")
        loss.backward()
        opt.step()
        torch.cuda.current_stream().synchronize()
        del pred, loss
    agent.zero_grad(set_to_none=True)
    agent.eval()
    after = scst.rollout(agent, fs, L, START, END, PAD, "audio_video", n=N, seed=5)
    fresh = _mk_agent()
    fresh.load_state_dict(agent.state_dict())
    want = scst.rollout(fresh, fs, L, START, END, PAD, "audio_video", n=N, seed=5)
    assert after.m == want.m and torch.equal(after.toks, want.toks)
    assert torch.equal(after.step_logp.view(torch.int32), want.step_logp.view(torch.int32))
    assert not torch.equal(after.step_logp, ro.step_logp), "the step changed nothing the rollout sees"


class _Dataset:
    pad_idx, start_idx, end_idx, phase = PAD, START, END, "train"

    def __init__(self, batches):
        self.batches = batches

    def update_iterator(self):
        pass


class _Loader:
    def __init__(self, ds):
        self.dataset = ds

    def __iter__(self):
        return iter(self.dataset.batches)

    def __len__(self):
        return len(self.dataset.batches)


def test_loop_runs_over_two_capacity_buckets(case):
    """two batches whose clip lengths fall into different capacity buckets (Tv 64, then 128): the second batch's decoder is
    captured after the first batch's training step, in one process"""
    from bmhrl_amd.epoch_loops.captioning_scst_loops import train_bmhrl_scst
    agent = _mk_agent()
    batches = [{"feature_stacks": _batch(B, tv, TA, V, 6 + i), "captions": ["a b c"] * B} for i, tv in enumerate((TV, 128))]
    cfg = syn.default_cfg(dout_p=0.0, max_len=L, scst_samples=N, scst_seed=3, scst_score_fn=_score_fn, scst_baseline="mean",
                          scst_clip=0.2, scst_entropy=0.01, grad_clip=1.0)
    opt = torch.optim.Adam([p for p in agent.parameters()], lr=1e-4)
    w0 = agent.worker.core.projection.weight.detach().clone()
    m0 = agent.manager.linear.weight.detach().clone()
    seen = []
    board = SimpleNamespace(add_scalar=lambda *a: seen.append(a))
    loss = train_bmhrl_scst(cfg, {"captioning": (agent, opt, None)}, None, _Loader(_Dataset(batches)), 0, "t", board)
    assert loss == loss and abs(loss) < float("inf")
    assert len(agent.__dict__["_sample_decoders"]) == 2
    assert not torch.equal(w0, agent.worker.core.projection.weight) and torch.equal(m0, agent.manager.linear.weight)
    assert [s[0] for s in seen] == ['debug/train_loss_epoch', 'debug/scst_reward_epoch'] and 0.0 <= seen[1][1] <= 1.0
    cfg.scst_baseline = "greedy"
    loss = train_bmhrl_scst(cfg, {"captioning": (agent, opt, None)}, None, _Loader(_Dataset(batches)), 1, "t", None)
    assert loss == loss and abs(loss) < float("inf")


def test_prefix_scores_binds_every_clips_caption_for_its_rollouts():
    """scst.prefix_scores through the scorers' public prefix_scores (BLEU and METEOR): the fp64 table of the existing reward
    launch with each clip's caption repeated for its n rollouts, bit for bit"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bmhrl_amd import scst
    from bmhrl_amd.rewards import BleuScorer, MeteorScorer
    itos = ["<unk>", "<pad>", "<s>", "</s>"] + [f"w{i}" for i in range(26)]
    vocab = SimpleNamespace(itos=itos)
    caps = ["w1 w2 w3 w4", "w5 w6 w2 w1 w9"]
    n, m = 3, 6
    g = torch.Generator().manual_seed(0)
    toks = torch.cat([torch.full((2 * n, 1), START), torch.randint(4, 14, (2 * n, m), generator=g)], 1).to(DEV)
    rep = [c for c in caps for _ in range(n)]
    for scorer in (BleuScorer(vocab, DEV, 0.9, 0.7), MeteorScorer(vocab, DEV, 0.9, 0.7, stemmer=False, synonyms=False)):
        got = scst.prefix_scores(scorer, toks, caps)
        assert got.dtype == torch.float64 and got.shape == (2 * n, m)
        want = scorer._diff(toks[:, 1:].contiguous(), rep)[1]
        assert torch.equal(got.view(torch.int64), want.view(torch.int64)) and bool((got > 0).any())
        with pytest.raises(TypeError):
            scorer.prefix_scores(toks[:, 1:], "w1 w2")
    with pytest.raises(ValueError):
        scst.prefix_scores(None, toks, caps)
