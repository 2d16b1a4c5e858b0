"""The device caption rewards (csrc/rewards.hip through bmhrl_amd/rewards.py) on the GPU: the reference scorers' own
outputs (tests/golden/rewards.npz), random cases against the float64 restatement (tests/reward_reference.py), the shape
limits, a captured reward launch re-bound between replays, and the worker RL step with device rewards."""
import random
import types

import numpy as np
import pytest
import torch

from tests import reward_reference as rr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx(golden):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return golden("rewards")


def _scorers(fx, n, sigma):
    from bmhrl_amd.rewards import BleuScorer, CiderScorer
    vocab = types.SimpleNamespace(itos=[str(s) for s in fx["itos"]])
    g, gm = (float(x) for x in fx["gamma"])
    corpus = [c.split() for c in fx["corpus"]]
    return CiderScorer(vocab, iter(corpus), DEV, g, gm, n=n, sigma=sigma), BleuScorer(vocab, DEV, g, gm, n=n, sigma=sigma)


def test_fixture_cases_match_the_reference_scorers(fx):
    caps = [str(c) for c in fx["captions"]]
    for c, (n, sigma, one) in enumerate(fx["cases"]):
        cid, ble = _scorers(fx, int(n), float(sigma))
        pred = torch.from_numpy(fx["hyp1"] if one else fx["hyp"]).to(DEV)
        w, r = cid.delta_cider_worker(pred, caps)
        assert w.dtype == torch.float32 and r.dtype == torch.float64 and w.device == pred.device
        np.testing.assert_allclose(r.cpu().numpy(), fx[f"c{c}_cider_rewards"], rtol=1e-12, atol=0)
        np.testing.assert_allclose(w.cpu().numpy(), fx[f"c{c}_cider_worker"], rtol=0, atol=1e-6)
        w, r = ble.delta_bleu_worker(pred, caps)
        assert w.dtype == torch.float32 and r.dtype == torch.float32
        np.testing.assert_allclose(r.cpu().numpy(), fx[f"c{c}_bleu_rewards"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(w.cpu().numpy(), fx[f"c{c}_bleu_worker"], rtol=0, atol=1e-6)
        if not one:
            sec = torch.from_numpy(fx["sections_in"]).to(DEV)
            m, none = cid.delta_cider_manager(pred, caps, None, sec)
            assert none is None and m.dtype == torch.float32
            np.testing.assert_array_equal(sec.cpu().numpy(), fx[f"c{c}_cider_sections"])     # the in-place write
            # the manager sums segments and discounts them in another fp32 order than the reference's loops (rl_glue)
            np.testing.assert_allclose(m.cpu().numpy(), fx[f"c{c}_cider_manager"], rtol=1e-6, atol=1e-6)
            sec = torch.from_numpy(fx["sections_in"]).to(DEV)
            m, _ = ble.delta_bleu_manager(pred, caps, None, sec)
            np.testing.assert_array_equal(sec.cpu().numpy(), fx["sections_in"])                  # BLEU leaves it alone
            np.testing.assert_allclose(m.cpu().numpy(), fx[f"c{c}_bleu_manager"], rtol=1e-6, atol=1e-6)
        assert cid.type == "CIDER" and ble.type == "BLEU" and cid.counter == ble.counter == (2 if not one else 1)


def test_cider_manager_index_error_past_the_row(fx):
    cid, _ = _scorers(fx, 4, 6.0)
    pred = torch.from_numpy(fx["hyp"]).to(DEV)
    caps = [str(c) for c in fx["captions"]]
    caps[2] = " ".join(["w"] * pred.shape[1])
    sec = torch.from_numpy(fx["sections_in"]).to(DEV)
    with pytest.raises(IndexError):
        cid.delta_cider_manager(pred, caps, None, sec)
    expect = torch.from_numpy(fx["c0_cider_sections"])
    assert torch.equal(sec[:2].cpu(), expect[:2]) and torch.equal(sec[2:].cpu(), torch.from_numpy(fx["sections_in"][2:]))


def _random_case(seed, V=500, n_corpus=5000, B=64, L=30, R_max=80):
    rng = random.Random(seed)
    common = [f"w{i}" for i in range(40)]
    itos = ["<unk>", "<pad>", "<s>", "</s>", " ", ""] + [w.upper() if i % 37 == 0 else w for i, w in enumerate(
        common + [f"v{i}" for i in range(V - 6 - len(common))])]
    zipf = lambda: common[min(int(rng.paretovariate(1.2)) - 1, len(common) - 1)] if rng.random() < 0.7 else \
        itos[rng.randrange(6, V)].lower()                                                                # noqa: E731
    corpus = [[zipf() for _ in range(rng.randint(1, 15))] for _ in range(n_corpus)]
    caps = []
    for b in range(B):
        words = [zipf() if rng.random() < 0.8 else f"oov{rng.randrange(9)}" for _ in range(rng.randint(0, R_max))]
        caps.append(" ".join(w.upper() if rng.random() < 0.1 else w for w in words) + (" ." if b % 3 == 0 else ""))
    stoi = {s: i for i, s in enumerate(itos)}
    hyp = torch.empty(B, L, dtype=torch.int64)
    for b in range(B):
        for t in range(L):
            r = rng.random()
            hyp[b, t] = rng.choice([4, 5]) if r < 0.05 else (3 if r < 0.08 and b % 4 else stoi.get(zipf(), 6 + t))
        if b % 8 == 1:
            hyp[b, 0] = 3
    return itos, corpus, caps, hyp


def test_random_cases_match_the_restatement():
    from bmhrl_amd.rewards import BleuScorer, CiderScorer
    itos, corpus, caps, hyp = _random_case(3)
    df = rr.precook_corpus(corpus)
    vocab = types.SimpleNamespace(itos=itos)
    for n, sigma in ((4, 6.0), (2, 3.0)):
        cid = CiderScorer(vocab, iter(corpus), DEV, 0.9, 0.7, n=n, sigma=sigma)
        ble = BleuScorer(vocab, DEV, 0.9, 0.7, n=n, sigma=sigma)
        pred = hyp.to(DEV)
        d, r = cid._cider_diff(pred, caps)
        want = np.stack([rr.cider_scores(itos, row, caps[b], df, n, sigma) for b, row in enumerate(hyp.tolist())])
        np.testing.assert_allclose(r.cpu().numpy(), want, rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(d.cpu().numpy(), rr.delta_row(want), rtol=0, atol=1e-6)
        assert (want != 0).mean() > 0.5 and (want == np.float64(np.float32(-0.1))).any()
        d, r = ble._bleu_diff(pred, caps)
        want = np.stack([rr.bleu_scores(itos, row, caps[b], n) for b, row in enumerate(hyp.tolist())])
        np.testing.assert_allclose(r.cpu().numpy(), want, rtol=0, atol=1e-6)
        np.testing.assert_allclose(d.cpu().numpy(), rr.delta_row(want), rtol=0, atol=1e-6)


def test_limits_are_refused():
    from bmhrl_amd import _lib, ops
    from bmhrl_amd.rewards import CiderScorer
    itos, corpus, caps, hyp = _random_case(5, n_corpus=200, B=4, L=8)
    cid = CiderScorer(types.SimpleNamespace(itos=itos), iter(corpus), DEV, 0.9, 0.7)
    with pytest.raises(ValueError):
        cid.bind(["w1 " * (ops.REWARDS_MAX_R + 1)])
    cid.bind(caps)
    with pytest.raises(ValueError):
        cid._launch(torch.zeros(4, ops.REWARDS_MAX_L + 1, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        cid._launch(torch.zeros(5, 8, dtype=torch.int64, device=DEV))            # more samples than bound captions
    # the kernel's own checks: -22 above the limits
    R = ops.REWARDS_MAX_R
    L = ops.REWARDS_MAX_L + 1
    h = torch.zeros(1, L, dtype=torch.int64, device=DEV)
    ref = torch.zeros(1, R, dtype=torch.int32, device=DEV)
    rl = torch.zeros(1, dtype=torch.int32, device=DEV)
    s, d = torch.empty(1, L, dtype=torch.float64, device=DEV), torch.empty(1, L, device=DEV)
    with pytest.raises(_lib.HipError, match="-22"):
        ops.rewards(h, cid.vmap, cid.eos, ref, rl, cid.df_keys, cid.df_logs, ops.REWARD_CIDER, 4, 6.0, s, d)
    ref2 = torch.zeros(1, R + 1, dtype=torch.int32, device=DEV)
    s, d = s[:, :8].contiguous(), d[:, :8].contiguous()
    with pytest.raises(_lib.HipError, match="-22"):
        ops.rewards(h[:, :8].contiguous(), cid.vmap, cid.eos, ref2, rl, cid.df_keys, cid.df_logs, ops.REWARD_CIDER, 4, 6.0,
                    s, d)
    with pytest.raises(_lib.HipError, match="-22"):
        ops.rewards(h[:, :8].contiguous(), cid.vmap, cid.eos, ref, rl, cid.df_keys, cid.df_logs, ops.REWARD_CIDER, 5, 6.0,
                    s, d)


def test_captured_reward_rebinds_between_replays():
    from bmhrl_amd.rewards import CiderScorer, BleuScorer
    itos, corpus, caps, hyp = _random_case(11, n_corpus=1000, B=16, L=20)
    caps2 = list(reversed(caps))
    vocab = types.SimpleNamespace(itos=itos)
    for sc in (CiderScorer(vocab, iter(corpus), DEV, 0.9, 0.7), BleuScorer(vocab, DEV, 0.9, 0.7)):
        fn = sc.reward_fn()
        pred = hyp.to(DEV)
        e1, e2 = fn(pred, caps).clone(), fn(pred, caps2).clone()
        worker = sc.delta_cider_worker if sc.type == "CIDER" else sc.delta_bleu_worker
        assert torch.equal(e1, worker(pred, caps)[0])
        assert not torch.equal(e1, e2)
        sc.bind(caps)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            fn(pred, None)                  # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = fn(pred, None)
        for c, want in ((caps2, e2), (caps, e1), (caps2, e2)):
            sc.bind(c)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want)
        del g


def _trainer_case():
    from bmhrl_amd import synthetic as syn
    V, B = 80, 4
    cfg = syn.tiny_cfg(d_model=1024, rl_att_heads=4, dout_p=0.0)
    b = syn.synthetic_batch(B, 160, 200, 8, V, seed=10, d_vid=cfg.d_vid, d_aud=cfg.d_aud, min_len=3)
    itos = ["<unk>", "<pad>", "<s>", "</s>"] + [f"w{i % 20}" if i % 3 else f"W{i}" for i in range(V - 4)]
    itos = [s if itos.index(s) == i else f"u{i}" for i, s in enumerate(itos)]
    corpus = [[f"w{(i * 7 + j) % 20}" for j in range(2 + i % 9)] for i in range(300)]
    caps = ["w1 w8 w15 w2 w9", "W5 w3 w3 w3", "", "w7 w14 w1 w8 w15 w2 w9 w16"]
    return cfg, V, b, itos, corpus, caps


def test_worker_step_with_device_rewards_matches_the_restatement():
    """an eager worker RL step with reward_fn=scorer.reward_fn() == one whose reward_fn scores the same sampled tokens with
    the CPU restatement; the captured step == the eager step"""
    from bmhrl_amd import rl_glue
    from bmhrl_amd.rewards import CiderScorer
    from bmhrl_amd.train import CaptionTrainer
    cfg, V, b, itos, corpus, caps = _trainer_case()
    df = rr.precook_corpus(corpus)
    fs = {k: b[k].to(DEV) for k in ("rgb", "flow", "audio")}
    cap = b["captions"].to(DEV)
    scorer = CiderScorer(types.SimpleNamespace(itos=itos), iter(corpus), DEV, 0.9, 0.7)
    scorer.bind(caps)
    seen = []

    def host_fn(sampled, captions):
        rows = sampled.cpu().tolist()
        seen.append(rows)
        want = np.stack([rr.cider_scores(itos, r, caps[i], df) for i, r in enumerate(rows)])
        return rl_glue.discontinue_reward(torch.from_numpy(rr.delta_row(want)).to(DEV), 0.9)

    def mk(fn):
        t = CaptionTrainer(cfg, V, DEV, exploration=False, lr=1e-3, phase="worker", reward_fn=fn, value_lr=1e-3)
        t.agent.train()
        t.value_net.train()
        return t

    dev_fn = scorer.reward_fn()
    dev_seen = []

    def dev_logged(sampled, captions):
        out = dev_fn(sampled, captions)
        dev_seen.append((sampled.cpu().tolist(), out.cpu()))
        return out

    t1, t2 = mk(dev_logged), mk(host_fn)
    l1, v1, l2, v2 = [], [], [], []
    for _ in range(3):
        l1.append(float(t1.step(fs, cap)))
        v1.append(float(t1.last_value_loss))
        l2.append(float(t2.step(fs, cap)))
        v2.append(float(t2.last_value_loss))
    assert len(seen) == len(dev_seen) == 3 and any(any(x != 3 for x in r) for r in seen[0])
    # every step's device reward == the restatement's on the same sampled tokens
    for rows, got in dev_seen:
        want = np.stack([rr.cider_scores(itos, r, caps[i], df) for i, r in enumerate(rows)])
        ref = rl_glue.discontinue_reward(torch.from_numpy(rr.delta_row(want)).to(DEV), 0.9).cpu()
        assert torch.allclose(got, ref, rtol=0, atol=1e-6)
    # step 1 samples the same tokens in both trainers: same loss and value loss.  Later steps start from two trainers'
    # own Adam updates, which are not bitwise reproducible, so they sample other tokens (the rewards above still agree).
    assert seen[0] == dev_seen[0][0]
    assert abs(l1[0] - l2[0]) <= 1e-5 * abs(l1[0]) and abs(v1[0] - v2[0]) <= 1e-5 * abs(v1[0]) + 1e-7, (l1, l2, v1, v2)
    # the captured step: warm-up step 1 eager, then replays 2 and 3 == eager steps 2 and 3
    t3 = mk(dev_fn)
    t3.capture(fs, cap, warmup=1)
    lg = []
    for _ in range(2):
        scorer.bind(caps)
        lg.append(float(t3.replay()))
    assert all(abs(a - g) < 2e-3 * abs(a) for a, g in zip(l1[1:], lg)), (l1, lg)
