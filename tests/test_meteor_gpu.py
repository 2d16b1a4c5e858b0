"""The device METEOR rewards (csrc/meteor.hip through bmhrl_amd/rewards.py MeteorScorer) on the GPU against the plain-Python
restatement (tests/meteor_reference.py): nltk's documented values, random cases with every combination of stages and with
strided rows, the edge shapes and limits, the manager path, a captured reward launch re-bound between replays, and an
eager worker RL step.  Tolerances: the fp64 scores at rtol 1e-12 (room for pow's last place, as the fp64 CIDEr rows), the
fp32 rewards / differences at atol 1e-6 (the bound of the other reward rows)."""
import types

import numpy as np
import pytest
import torch

from tests import meteor_reference as mr
from tests.test_meteor_cpu import HYP1, REF1, always_forever

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ST = mr.DictStemmer()


def _scorer(itos, stem=True, syn=True, stemmer=ST, synonyms=mr.dict_synonyms):
    from bmhrl_amd.rewards import MeteorScorer
    return MeteorScorer(types.SimpleNamespace(itos=list(itos)), DEV, 0.9, 0.7, stemmer=stemmer if stem else False,
                        synonyms=synonyms if syn else False)


def _want(itos, hyp, caps, stem, syn, fn=mr.meteor_scores):
    return np.stack([fn(itos, row, caps[b], stem, syn) for b, row in enumerate(np.asarray(hyp).tolist())])


def _check(sc, hyp, caps, want):
    """the fp64 scores, the fp32 rewards and the differences of one launch against the restatement's rows"""
    pred = torch.as_tensor(hyp, dtype=torch.int64).to(DEV)
    d, s = sc._diff(pred, caps)
    assert s.dtype == torch.float64 and d.dtype == torch.float32 and s.shape == d.shape == pred.shape
    np.testing.assert_allclose(s.cpu().numpy(), want, rtol=1e-12, atol=0)
    d2, r = sc._meteor_diff(pred, caps, None)
    assert r.dtype == torch.float32 and torch.equal(d, d2)
    np.testing.assert_allclose(r.cpu().numpy(), mr.rewards_row(want), rtol=0, atol=1e-6)
    np.testing.assert_allclose(d.cpu().numpy(), mr.delta_row(want), rtol=0, atol=1e-6)
    return s


@pytest.fixture(scope="module")
def case():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    itos, caps, hyp = mr.random_case(3)
    want = {(a, b): _want(itos, hyp, caps, ST.stem if a else None, mr.dict_synonyms if b else None)
            for a in (False, True) for b in (False, True)}
    return itos, caps, hyp, want


def test_documented_values():
    from bmhrl_amd import rl_glue
    sents = [(HYP1, REF1), ("on the mat sat the cat", "the cat sat on the mat"), ("non matching hypothesis", "this is a cat"),
             (HYP1, "")]
    itos = ["<unk>", ""] + sorted({w for h, _ in sents for w in h.split()})
    stoi = {s: i for i, s in enumerate(itos)}
    L = max(len(h.split()) for h, _ in sents)
    hyp = np.array([[stoi[w] for w in h.split()] + [1] * (L - len(h.split())) for h, _ in sents])
    caps = [r for _, r in sents]
    ident = mr.DictStemmer({})
    sc = _scorer(itos, stemmer=ident, synonyms=always_forever)
    want = _want(itos, hyp, caps, ident.stem, always_forever)
    s = _check(sc, hyp, caps, want)[:, -1].cpu().numpy()
    np.testing.assert_allclose(s, [0.7398275988019579, 0.5, 0.0, 0.0], rtol=1e-12, atol=0)
    w, r = sc.delta_meteor_worker(torch.as_tensor(hyp).to(DEV), caps, None)
    assert w.dtype == r.dtype == torch.float32 and w.device.type == "cuda" and sc.type == "METEOR" and sc.counter == 3
    ref = rl_glue.discontinue_reward(torch.from_numpy(mr.delta_row(want)).to(DEV), 0.9)
    assert torch.allclose(w, ref, rtol=0, atol=1e-6)
    # the exact stage alone
    sc = _scorer(itos, stem=False, syn=False)
    s = _check(sc, hyp, caps, _want(itos, hyp, caps, None, None))[:, -1].cpu().numpy()
    np.testing.assert_allclose(s, [0.6944444444444445, 0.5, 0.0, 0.0], rtol=1e-12, atol=0)


@pytest.mark.parametrize("stem,syn", [(False, False), (True, False), (False, True), (True, True)])
def test_random_cases_match_the_restatement(case, stem, syn):
    itos, caps, hyp, want = case
    assert (want[(stem, syn)] != 0).mean() > 0.5
    if stem or syn:
        assert (want[(stem, syn)] != want[(False, False)]).any()
    _check(_scorer(itos, stem, syn), hyp, caps, want[(stem, syn)])


def test_strided_rows_and_untouched_padding(case):
    from bmhrl_amd import ops
    itos, caps, hyp, want = case
    sc = _scorer(itos)
    sc.bind(caps)
    B, L = hyp.shape
    big = torch.randint(6, len(itos), (B, L + 7), device=DEV)            # words behind the rows would change the scores
    big[:, :L] = torch.from_numpy(hyp).to(DEV)
    scores = torch.full((B, L + 3), -7.0, dtype=torch.float64, device=DEV)
    delta = torch.full((B, L + 5), -9.0, dtype=torch.float32, device=DEV)
    ref, ref_len = sc.bound()
    ops.meteor(big[:, :L], sc.vmap, sc.vstem, sc.syn_off, sc.syn_ids, ref[0], ref[1], ref_len, 0.9, 3.0, 0.5, scores[:, :L],
               delta[:, :L])
    np.testing.assert_allclose(scores[:, :L].cpu().numpy(), want[(True, True)], rtol=1e-12, atol=0)
    np.testing.assert_allclose(delta[:, :L].cpu().numpy(), mr.delta_row(want[(True, True)]), rtol=0, atol=1e-6)
    assert (scores[:, L:] == -7.0).all() and (delta[:, L:] == -9.0).all()
    # two runs agree bit for bit
    s2, d2 = torch.empty(B, L, dtype=torch.float64, device=DEV), torch.empty(B, L, device=DEV)
    ops.meteor(big[:, :L], sc.vmap, sc.vstem, sc.syn_off, sc.syn_ids, ref[0], ref[1], ref_len, 0.9, 3.0, 0.5, s2, d2)
    assert torch.equal(s2, scores[:, :L]) and torch.equal(d2, delta[:, :L])


def test_edge_rows():
    itos = mr.case_vocab()
    V = len(itos)
    sc = _scorer(itos)
    st, sy = ST.stem, mr.dict_synonyms
    # L = 1; an empty reference; a row of tokens without a word; ids outside the vocabulary
    hyp = np.array([[6], [4], [-1], [V], [25]])
    caps = ["a big dog", "a", "a", "a", ""]
    want = _want(itos, hyp, caps, st, sy)
    assert want[0, 0] > 0 and (want[1:] == 0).all()
    _check(sc, hyp, caps, want)
    hyp = np.array([[4, 5, 5, 4, 5, 4], [-1, 6, V, 7, V + 9, 6], [6, 7, 25, 10, 11, 12], [-5, 4, 5, V, 4, -1]])
    caps = ["a", "a the a", "", "a"]
    want = _want(itos, hyp, caps, st, sy)
    assert (want[0] == 0).all() and want[0].shape == (6,) and (want[2] == 0).all() and (want[3] == 0).all()
    assert want[1, 0] == 0 and want[1, 1] > 0 and want[1, 2] == want[1, 1] and want[1, 5] > want[1, 4] == want[1, 3]
    _check(sc, hyp, caps, want)


@pytest.mark.parametrize("L,R", [(65, 65), (65, 129), (256, 512)])
def test_past_a_wave_and_at_the_limits(L, R):
    """one past a wave of reference lanes (R = 65, 129) and of hypothesis slots (L = 65); the largest shape, one sample"""
    from bmhrl_amd import ops
    assert (ops.REWARDS_MAX_L, ops.REWARDS_MAX_R) == (256, 512)
    itos, caps, hyp = mr.random_case(L + R, B=2 if L < 256 else 1, L=L, R_max=R)
    rng = np.random.RandomState(R)
    pool = [s.lower() for s in itos[6:]] + ["walker", "great", "feline", "oov"]
    caps = [" ".join(pool[rng.randint(len(pool))] for _ in range(R)) for _ in caps]
    hyp[:, -1] = 25                                          # the last prefix holds every word
    assert (hyp[0] >= 6).sum() > 0.8 * L
    want = _want(itos, hyp, caps, ST.stem, mr.dict_synonyms, fn=mr.meteor_scores_reduced)
    assert (want[:, -1] > 0).all()
    _check(_scorer(itos), hyp, caps, want)


def test_refusals():
    from bmhrl_amd import _lib, ops
    itos, caps, hyp = mr.random_case(5, B=2, L=8)
    sc = _scorer(itos)
    with pytest.raises(ValueError):
        sc.bind(["a " * (ops.REWARDS_MAX_R + 1)])
    sc.bind(caps)
    with pytest.raises(ValueError):
        sc._launch(torch.zeros(2, ops.REWARDS_MAX_L + 1, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        sc._launch(torch.zeros(3, 8, dtype=torch.int64, device=DEV))             # more samples than bound captions
    ref, ref_len = sc.bound()
    R = ops.REWARDS_MAX_R
    lib = _lib.load()

    def call(L=8, R=R, ld=None, **null):
        """bmhrl_meteor on buffers large enough for L = MAX_L + 1, R = MAX_R + 1; null: pointers to pass as null"""
        ld = ld or ops.REWARDS_MAX_L + 1
        h = torch.zeros(2, ld, dtype=torch.int64, device=DEV)
        rf = torch.zeros(2, 2, R + 1, dtype=torch.int32, device=DEV)
        s, d = torch.zeros(2, ld, dtype=torch.float64, device=DEV), torch.zeros(2, ld, device=DEV)
        p = dict(hyp=h, vmap=sc.vmap, vstem=sc.vstem, syn_off=sc.syn_off, syn_ids=sc.syn_ids, ref=rf[0], ref_stem=rf[1],
                 ref_len=ref_len, scores=s, delta=d)
        a = {k: (None if null.get(k) else v.data_ptr()) for k, v in p.items()}
        return lib.bmhrl_meteor(a["hyp"], ld, a["vmap"], a["vstem"], sc.vmap.numel(), a["syn_off"], a["syn_ids"],
                                sc.syn_ids.numel(), a["ref"], a["ref_stem"], R + 1, a["ref_len"], 0.9, 3.0, 0.5, 2, L, R,
                                a["scores"], ld, a["delta"], ld, ops.stream())

    assert call() == 0 and call(L=ops.REWARDS_MAX_L) == 0
    assert call(L=ops.REWARDS_MAX_L + 1) == -22 and call(R=R + 1) == -22 and call(L=0) == -22 and call(R=0) == -22
    for name in ("hyp", "vmap", "ref", "ref_len", "scores", "delta"):
        assert call(**{name: True}) == -22, name
    assert call(syn_off=True) == -22 and call(syn_ids=True) == -22 and call(syn_off=True, syn_ids=True) == 0
    assert call(ref_stem=True) == -22 and call(vstem=True) == 0 and call(vstem=True, ref_stem=True) == 0
    assert call(L=9, ld=8) == -22
    torch.cuda.synchronize()
    # ops.meteor hands half a synonym table through to the kernel's check
    s, d = torch.empty(2, 8, dtype=torch.float64, device=DEV), torch.empty(2, 8, device=DEV)
    with pytest.raises(_lib.HipError, match="-22"):
        ops.meteor(torch.from_numpy(hyp).to(DEV), sc.vmap, sc.vstem, sc.syn_off, None, ref[0], ref[1], ref_len, 0.9, 3.0,
                   0.5, s, d)


def test_manager_path(case):
    from bmhrl_amd import rl_glue
    itos, caps, hyp, want = case
    sc = _scorer(itos)
    pred = torch.from_numpy(hyp).to(DEV)
    sections = (torch.rand(hyp.shape, generator=torch.Generator().manual_seed(1)) < 0.2).long().to(DEV)
    before = sections.clone()
    m, none = sc.delta_meteor_manager(pred, caps, None, sections)
    assert none is None and m.dtype == torch.float32 and torch.equal(sections, before)
    step = rl_glue.discontinue_reward(torch.from_numpy(mr.delta_row(want[(True, True)])).to(DEV), 0.9)
    ref = rl_glue.discontinue_reward(rl_glue.segment_reward(step, sections)[0], 0.9)
    assert torch.allclose(m, ref, rtol=1e-6, atol=1e-6)
    seg, idx = sc.delta_meteor_segment(step, sections, 0.9)
    assert torch.equal(seg, ref) and torch.equal(idx, torch.nonzero(sections))
    g = sc.get_meteor_gamma(0.9, 3, 5)
    assert g.shape == (3, 5, 5) and float(g[1, 0, 0]) == 1.0 and float(g[2, 3, 1]) == 0.0
    assert abs(float(g[0, 1, 4]) - 0.9 ** 3) < 1e-6


def test_captured_reward_rebinds_between_replays():
    itos, caps, hyp = mr.random_case(11, B=16, L=20)
    caps2 = list(reversed(caps))
    sc = _scorer(itos)
    fn = sc.reward_fn()
    pred = torch.from_numpy(hyp).to(DEV)
    e1, e2 = fn(pred, caps).clone(), fn(pred, caps2).clone()
    assert torch.equal(e1, sc.delta_meteor_worker(pred, caps, None)[0]) and not torch.equal(e1, e2)
    sc.bind(caps)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn(pred, None)                  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn(pred, None)
    from bmhrl_amd import rl_glue
    wants = {}
    for name, c in (("a", caps), ("b", caps2)):
        w = _want(itos, hyp, c, ST.stem, mr.dict_synonyms)
        wants[name] = rl_glue.discontinue_reward(torch.from_numpy(mr.delta_row(w)).to(DEV), 0.9)
    for c, eager, name in ((caps2, e2, "b"), (caps, e1, "a"), (caps2, e2, "b")):
        sc.bind(c)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
        assert torch.allclose(out, wants[name], rtol=0, atol=1e-6)
    del g


def test_worker_step_sees_the_restatements_reward():
    """one eager worker RL step with reward_fn=MeteorScorer(...).reward_fn(): the reward the loss saw is the restatement's
    on the tokens the step sampled"""
    from bmhrl_amd import rl_glue, synthetic as syn
    from bmhrl_amd.train import CaptionTrainer
    V, B = 80, 4
    cfg = syn.tiny_cfg(d_model=1024, rl_att_heads=4, dout_p=0.0)
    b = syn.synthetic_batch(B, 160, 200, 8, V, seed=10, d_vid=cfg.d_vid, d_aud=cfg.d_aud, min_len=3)
    itos = ["<unk>", "<pad>", "<s>", "</s>"] + [f"w{i % 20}" if i % 3 else f"W{i}" for i in range(V - 4)]
    itos = [s if itos.index(s) == i else f"u{i}" for i, s in enumerate(itos)]
    caps = ["w1 w8 w15 w2 w9", "W5 w3 w3 w3", "", "w7 w14 w1 w8 w15 w2 w9 w16"]
    stemmer = mr.DictStemmer({f"{c}{i}": f"s{i % 7}" for c in "wu" for i in range(V)})      # w1, w8, w15, u8, ... share a stem
    synonyms = lambda w: [f"w{(int(w[1:]) * 3) % 20}", "w3"] if w[1:].isdigit() else []                   # noqa: E731
    sc = _scorer(itos, stemmer=stemmer, synonyms=synonyms)
    sc.bind(caps)
    fn, seen = sc.reward_fn(), []

    def logged(sampled, captions):
        out = fn(sampled, captions)
        seen.append((sampled.cpu().numpy(), out.clone()))
        return out

    t = CaptionTrainer(cfg, V, DEV, exploration=False, lr=1e-3, phase="worker", reward_fn=logged, value_lr=1e-3)
    t.agent.train()
    t.value_net.train()
    loss = float(t.step({k: b[k].to(DEV) for k in ("rgb", "flow", "audio")}, b["captions"].to(DEV)))
    assert np.isfinite(loss) and len(seen) == 1
    rows, got = seen[0]
    want = _want(itos, rows, caps, stemmer.stem, synonyms)
    assert (want[0] != 0).any() and (want[2] == 0).all()
    ref = rl_glue.discontinue_reward(torch.from_numpy(mr.delta_row(want)).to(DEV), 0.9)
    assert got.dtype == torch.float32 and torch.allclose(got, ref, rtol=0, atol=1e-6)
