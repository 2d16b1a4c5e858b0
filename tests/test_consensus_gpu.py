"""Consensus choice on the GPU: bmhrl_consensus (csrc/consensus.hip) against the restatement of tests/consensus_reference.py --
equality of every utility and every pair entry -- and select="consensus" on the two incremental decoders of the small agent of
tests/test_constrain_gpu.py, with the captured graph and without."""
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import consensus_reference as ref

pytestmark = pytest.mark.gpu

PAD, START = 1, 2
DEV = "cuda:0"
AV = "audio_video"
V7, END7 = 7, 6
OUTSIDE = (-3, 9)                       # two ids outside [0, V7): they weigh 0 and compare by their ids
SENTINEL = 4                            # fills the columns behind `steps`: a frequent word, so reading it changes the grams
BS, KS, STEPS, NS = (1, 3), (1, 2, 3, 16), (0, 1, 5, 30, 256), (1, 2, 3, 4)


def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _hypotheses(B, K, S, seed):
    """(B, K, S + 4) int64: column 0 the start token, S generated tokens over ids 0 .. 5 (many repeated grams, pad_idx = 1
    among them), SENTINEL behind them.  Row (b, k) is of kind (b + k) % 6: 0 never ends; 1 ends at a random column; 2 repeats
    the row before it (an exact duplicate); 3 ends at column 1 (no word); 4 has at most two words (shorter than N = 3, 4);
    5 ends at a random column behind a pad word.  pad_idx follows every end."""
    rng = np.random.RandomState(seed)
    h = rng.randint(0, 6, size=(B, K, S + 4))
    h[:, :, 0] = START
    h[:, :, S + 1:] = SENTINEL
    for b, k in itertools.product(range(B), range(K)):
        kind = (b + k) % 6
        end = None                                              # the column of the end token
        if kind in (1, 5) and S >= 1:
            end = int(rng.randint(1, S + 1))
        elif kind == 2 and k >= 1:
            h[b, k] = h[b, k - 1]
        elif kind == 3 and S >= 1:
            end = 1
        elif kind == 4 and S >= 1:
            end = min(3, S)
        if end is not None:
            h[b, k, end] = END7
            h[b, k, end + 1:S + 1] = PAD
            if kind == 5 and end >= 2:
                h[b, k, 1] = PAD
    return h


@functools.lru_cache(None)
def _cases():
    """every (B, K, steps): the hypotheses, the same with some words replaced by the ids of OUTSIDE, random fp32 weights in
    [0.25, 4], and the restatement's terms of both -- computed once, read by every test below"""
    rng = np.random.RandomState(11)
    out = {}
    for n, (B, K, S) in enumerate(itertools.product(BS, KS, STEPS)):
        h = _hypotheses(B, K, S, 100 + n)
        odd = h.copy()
        swap = rng.rand(B, K, S) < 0.15
        ids = np.asarray(OUTSIDE)[rng.randint(0, 2, size=(B, K, S))]
        body = odd[:, :, 1:S + 1]
        body[swap & (body != END7)] = ids[swap & (body != END7)]
        w = rng.uniform(0.25, 4.0, size=V7).astype(np.float32)
        out[(B, K, S)] = dict(h=h, odd=odd, w=w, t=ref.terms(h[:, :, :S + 1], END7), t_odd=ref.terms(odd[:, :, :S + 1], END7, w))
    return out


def _launch(h, K, S, N, w=None):
    from bmhrl_amd import ops
    hist = torch.from_numpy(h).to(DEV).view(-1, h.shape[-1])
    return ops.consensus(hist, S, K, END7, N, None if w is None else torch.from_numpy(w).to(DEV), pair=True)


def test_kernel_matches_the_restatement():
    """B in {1, 3} x K in {1, 2, 3, 16} x steps in {0, 1, 5, 30, 256} x N in {1 .. 4}, rows of steps + 4 columns with the
    sentinel behind the steps, three ways: no weights, all-ones weights (the same bits), random weights over hypotheses that
    hold two ids outside [0, V).  Every launch is issued first, the results are read afterwards."""
    _needs_gpu()
    cases = _cases()
    ones = np.ones(V7, dtype=np.float32)
    runs = []
    for (B, K, S), c in cases.items():
        kinds = {(b + k) % 6 for b in range(B) for k in range(K)}
        assert c["h"].shape == (B, K, S + 4) and (K < 16 or kinds == set(range(6)))
        for N in NS:
            runs.append(((B, K, S, N), c, _launch(c["h"], K, S, N), _launch(c["h"], K, S, N, ones),
                         _launch(c["odd"], K, S, N, c["w"]), _launch(c["odd"], K, S, N, c["w"])))
    torch.cuda.synchronize()
    positive = 0
    for key, c, plain, one, odd, again in runs:
        N = key[3]
        U, u = ref.utilities(c["t"], N)
        assert np.array_equal(_bits(plain[0].cpu()), _bits(U)), key
        assert np.array_equal(_bits(plain[1].cpu()), _bits(u)), key
        assert torch.equal(one[0], plain[0]) and torch.equal(one[1], plain[1]), key
        Uw, uw = ref.utilities(c["t_odd"], N)
        assert np.array_equal(_bits(odd[0].cpu()), _bits(Uw)), key
        assert np.array_equal(_bits(odd[1].cpu()), _bits(uw)), key
        assert np.array_equal(_bits(again[0].cpu()), _bits(odd[0].cpu())) and np.array_equal(_bits(again[1].cpu()), _bits(odd[1].cpu()))
        if key[2] == 0 or key[1] == 1:
            assert not U.any() and not Uw.any()
        positive += int((U > 0).sum())
    assert len(runs) == 160 and positive > 400
    big = cases[(3, 16, 256)]
    assert any(v in big["odd"][:, :, 1:257] for v in OUTSIDE) and (big["h"][:, :, 1:257] == PAD).any()


def test_kernel_reads_the_decoder_layout():
    """a history wider than the steps with a row stride of its own (a view of a larger buffer), and ids beyond int32"""
    _needs_gpu()
    from bmhrl_amd import ops
    B, K, S = 2, 3, 9
    h = _hypotheses(B, K, S, 5)[:, :, :S + 1]
    h[0, 1, 2] = 2 ** 40 + 3                                        # compares by its 64-bit id: not equal to 3
    h[0, 2, 2] = 3
    big = torch.full((B * K, 40), SENTINEL, dtype=torch.int64, device=DEV)
    big[:, :S + 1] = torch.from_numpy(h).view(B * K, -1).to(DEV)
    U = ops.consensus(big[:, :S + 3], S, K, END7, 4)
    assert U.shape == (B, K) and U.dtype == torch.float64
    want = ref.utilities(ref.terms(h, END7), 4)[0]
    assert np.array_equal(_bits(U.cpu()), _bits(want))
    # fewer steps than the history holds: the columns behind them are not read
    U5 = ops.consensus(big, 5, K, END7, 2)
    assert np.array_equal(_bits(U5.cpu()), _bits(ref.utilities(ref.terms(h[:, :, :6], END7), 2)[0]))


def test_refusals_leave_the_output_alone():
    _needs_gpu()
    from bmhrl_amd import _lib, ops
    B, K, S, ld = 2, 3, 6, 10
    hist = torch.from_numpy(_hypotheses(B, K, S, 1)).to(DEV).view(B * K, ld)
    w = torch.ones(V7, device=DEV)
    util = torch.full((B, K), -7.0, dtype=torch.float64, device=DEV)
    pair = torch.full((B, K, K), -7.0, dtype=torch.float64, device=DEV)
    lib = _lib.load()

    def call(**kw):
        a = dict(hist=hist.data_ptr(), ld=ld, B=B, K=K, steps=S, end=END7, N=4, w=w.data_ptr(), V=V7, util=util.data_ptr(),
                 pair=pair.data_ptr())
        a.update(kw)
        return lib.bmhrl_consensus(a["hist"], a["ld"], a["B"], a["K"], a["steps"], a["end"], a["N"], a["w"], a["V"], a["util"],
                                   a["pair"], ops.stream())
    for bad in (dict(hist=None), dict(util=None), dict(B=0), dict(B=-1), dict(K=0), dict(K=-2), dict(steps=-1), dict(K=17),
                dict(steps=257), dict(N=0), dict(N=5), dict(N=-1), dict(V=-1), dict(V=0), dict(ld=S), dict(ld=0)):
        assert call(**bad) == -22, bad
    torch.cuda.synchronize()
    assert bool((util == -7.0).all()) and bool((pair == -7.0).all())                # refused before any launch
    assert call(w=None, V=0) == 0 and call(pair=None) == 0 and call(steps=0, ld=1) == 0
    torch.cuda.synchronize()
    assert bool((util == 0).all())                                                  # steps = 0: every utility is 0
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((util >= 0).all()) and bool((util > 0).any()) and bool((pair >= 0).all())
    for kw in (dict(K=0), dict(K=17), dict(K=4), dict(steps=-1), dict(steps=257), dict(steps=ld), dict(n=0), dict(n=5),
               dict(token_weight=w.double()), dict(token_weight=w.view(1, -1)), dict(token_weight=w.cpu().to(DEV)[::2]),
               dict(hist=hist.int()), dict(hist=hist.t()), dict(hist=hist.view(-1))):
        a = dict(hist=hist, steps=S, K=K, end_idx=END7)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.consensus(**a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.consensus(hist.cpu(), S, K, END7)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.consensus(hist, S, K, END7, token_weight=w.cpu())


# ----------------------------------------------------------------------------------------------------------- decoders
# The small agent and the clip batch (B = 2, V = 150, max_len = 10) of tests/test_constrain_gpu.py; min_len keeps the
# hypotheses from ending at once, so that there are words to agree on (asserted below).
N_HYP = 4
MIN_LEN = 4
_CACHES = ("_incremental_decoders", "_beam_decoders", "_sample_decoders")


def _setup():
    from tests.test_constrain_gpu import L, _setup as setup
    agent, fs, end = setup()
    return agent, fs, end, (agent, fs, L, START, end, PAD, AV)


def _caption_rows(hyps, picks, end):
    caps = [ref.caption(hyps[b, k].tolist(), end) for b, k in enumerate(picks)]
    n = max(len(c) for c in caps)
    return [c + [PAD] * (n - len(c)) for c in caps]


def _check_sample(args, end, **kw):
    from bmhrl_amd.decode import sample_decode
    kw = dict(n=N_HYP, seed=3, top_p=0.9, min_len=MIN_LEN, **kw)
    base = sample_decode(*args, return_samples=True, **kw)
    same = sample_decode(*args, return_samples=True, select="logp", **kw)
    assert len(base) == len(same) == 5 and all(torch.equal(a, b) for a, b in zip(base, same))
    got = sample_decode(*args, return_samples=True, select="consensus", **kw)
    assert len(got) == 6 and all(torch.equal(a, b) for a, b in zip(base[1:], got[1:5]))
    samples, sums, util = got[1].cpu(), got[2].cpu(), got[5].cpu()
    U = ref.utilities(ref.terms(samples.numpy(), end), 4)[0]
    assert np.array_equal(_bits(util), _bits(U))
    picks = [ref.choose(U[b], ref.logp_order(sums[b].tolist())) for b in range(U.shape[0])]
    assert got[0].tolist() == _caption_rows(samples, picks, end)
    assert torch.equal(sample_decode(*args, select="consensus", **kw), got[0])
    assert (U > 0).any(), samples
    return picks, samples


def _check_beam(args, end, **kw):
    from bmhrl_amd.decode import beam_decode
    kw = dict(beam_size=N_HYP, min_len=MIN_LEN, **kw)
    base = beam_decode(*args, return_scores=True, return_beams=True, **kw)
    same = beam_decode(*args, return_scores=True, return_beams=True, select="logp", **kw)
    assert len(base) == len(same) == 4 and all(torch.equal(a, b) for a, b in zip(base, same))
    got = beam_decode(*args, return_scores=True, return_beams=True, select="consensus", consensus_n=2, **kw)
    assert len(got) == 5 and torch.equal(got[2], base[2]) and torch.equal(got[3], base[3])
    beams, scores, util = got[2].cpu(), got[3].cpu(), got[4].cpu()
    U = ref.utilities(ref.terms(beams.numpy(), end), 2)[0]
    assert np.array_equal(_bits(util), _bits(U))
    picks = [ref.choose(U[b], range(N_HYP)) for b in range(U.shape[0])]                # the beams arrive in rule 5's order
    assert got[0].tolist() == _caption_rows(beams, picks, end)
    assert torch.equal(got[1].cpu(), scores[torch.arange(len(picks)), torch.tensor(picks)])
    assert (U > 0).any(), beams
    return picks, beams


def test_decoders_return_what_the_restatement_picks(monkeypatch):
    """both incremental decoders, with the captured graph and -- on fresh decoders -- without it: the utilities returned are
    the restatement's of the hypotheses the same call returns, bit for bit, and the caption is the one R7 picks from them"""
    _needs_gpu()
    from bmhrl_amd.decode import BeamDecoder, IncrementalDecoder, SampleDecoder
    agent, fs, end, args = _setup()
    L = args[2]
    with_graph = (_check_sample(args, end), _check_beam(args, end))
    assert SampleDecoder.for_batch(agent, fs, L, START, end, PAD, N_HYP).graph is not None
    assert BeamDecoder.for_batch(agent, fs, L, START, end, PAD, N_HYP).graph is not None
    kept = {c: agent.__dict__.pop(c) for c in _CACHES if c in agent.__dict__}       # put back below, with their graphs
    for cls in (IncrementalDecoder, SampleDecoder, BeamDecoder):                    # (a subclass may carry its own switch)
        monkeypatch.setattr(cls, "use_graph", False)
    try:
        eager = (_check_sample(args, end), _check_beam(args, end))
        assert SampleDecoder.for_batch(agent, fs, L, START, end, PAD, N_HYP).graph is None
        assert BeamDecoder.for_batch(agent, fs, L, START, end, PAD, N_HYP).graph is None
    finally:
        monkeypatch.undo()
        for c in _CACHES:
            agent.__dict__.pop(c, None)
        agent.__dict__.update(kept)
    print(f"consensus picks: sample {with_graph[0][0]} (eager {eager[0][0]}), beam {with_graph[1][0]} (eager {eager[1][0]}); "
          f"samples of clip 0: {with_graph[0][1][0].tolist()}")


def test_weights_and_n_reach_the_kernel():
    _needs_gpu()
    from bmhrl_amd.decode import idf_weights, sample_decode
    agent, fs, end, args = _setup()
    w = idf_weights(torch.arange(150) % 13 + 1).to(DEV)
    got = sample_decode(*args, n=N_HYP, seed=3, top_p=0.9, min_len=MIN_LEN, return_samples=True, select="consensus", consensus_n=3,
                        consensus_weight=w)
    U = ref.utilities(ref.terms(got[1].cpu().numpy(), end, w.cpu().numpy()), 3)[0]
    assert np.array_equal(_bits(got[5].cpu()), _bits(U))
    # the re-run path of the same call goes through the host implementation: its utilities of its own samples
    rerun = sample_decode(*args, n=N_HYP, seed=3, top_p=0.9, min_len=MIN_LEN, return_samples=True, select="consensus",
                          consensus_n=3, consensus_weight=w, incremental=False)
    U2 = ref.utilities(ref.terms(rerun[1].cpu().numpy(), end, w.cpu().numpy()), 3)[0]
    assert rerun[5].is_cuda and np.array_equal(_bits(rerun[5].cpu()), _bits(U2))


def test_the_default_never_reaches_the_op(monkeypatch):
    """ops.consensus replaced by one that raises before fresh decoders are built: with select left at its default (and with
    select="logp") both decoders decode what they decoded before; select="consensus" does reach the stub"""
    _needs_gpu()
    from bmhrl_amd import ops
    from bmhrl_amd.decode import beam_decode, sample_decode
    agent, fs, end, args = _setup()
    skw = dict(n=N_HYP, seed=3, top_p=0.9, return_samples=True)
    bkw = dict(beam_size=N_HYP, return_scores=True, return_beams=True)
    today = (sample_decode(*args, **skw), beam_decode(*args, **bkw))
    kept = {c: agent.__dict__.pop(c) for c in _CACHES if c in agent.__dict__}

    def boom(*a, **k):
        raise AssertionError("consensus reached")
    monkeypatch.setattr(ops, "consensus", boom)
    try:
        for extra in ({}, dict(select="logp", consensus_n=2)):
            under = (sample_decode(*args, **skw, **extra), beam_decode(*args, **bkw, **extra))
            for a, b in zip(today, under):
                assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))
        with pytest.raises(AssertionError, match="consensus reached"):
            sample_decode(*args, select="consensus", **skw)
        with pytest.raises(AssertionError, match="consensus reached"):
            beam_decode(*args, select="consensus", **bkw)
    finally:
        monkeypatch.undo()
        for c in _CACHES:
            agent.__dict__.pop(c, None)
        agent.__dict__.update(kept)


def test_consensus_decoder_drives_predict_1by1():
    _needs_gpu()
    from types import SimpleNamespace
    from bmhrl_amd.epoch_loops.captioning_bmrl_loops import sample_decoder
    from bmhrl_amd.epoch_loops.validation_loops import predict_1by1
    agent, fs, end, args = _setup()
    itos = [f"w{i}" for i in range(150)]
    itos[START], itos[end], itos[PAD] = "<s>", "</s>", "<blank>"
    ds = SimpleNamespace(start_idx=START, end_idx=end, pad_idx=PAD, train_vocab=SimpleNamespace(itos=itos))
    batch = {"feature_stacks": fs, "video_ids": ["v0", "v1"], "starts": torch.tensor([0.0, 1.0]), "ends": torch.tensor([1.0, 2.0])}

    class Loader(list):
        dataset = ds
    cfg = SimpleNamespace(max_len=args[2], modality=AV)
    pred = predict_1by1(cfg, agent, Loader([batch]), sample_decoder(4, select="consensus"))
    got = [seg["sentence"] for vid in ("v0", "v1") for seg in pred["results"][vid]]
    assert len(got) == 2 and all(isinstance(s, str) for s in got)
