"""Constrained decoding on the GPU: bmhrl_logit_rules (csrc/constrain.hip) against the numpy restatement of
tests/constrain_reference.py, bit-equal, and the three incremental decoders under rules against their re-run paths, compared
the way tests/test_decode_gpu.py, tests/test_beam_gpu.py and tests/test_sample_gpu.py compare those paths without rules."""
import functools
import itertools

import numpy as np
import pytest
import torch

from bmhrl_amd import synthetic as syn
from tests import constrain_reference as ref
from tests.test_decode_gpu import _agent

pytestmark = pytest.mark.gpu

PAD, START = 1, 2
DEV = "cuda:0"
AV = "audio_video"
V7, END7 = 7, 6


def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _word(t):
    return torch.tensor([t], dtype=torch.int64, device=DEV)


# ------------------------------------------------------------------------------------------------------------- kernel
def _padded(lp, ld):
    buf = torch.full((lp.shape[0], ld), float("nan"))
    buf[:, :lp.shape[1]] = lp
    return buf


def test_logit_rules_matches_the_restatement():
    """rows = 3, V = 37 in rows of 40 floats whose last three hold NaN: the case table of the CPU file (t = 0 .. 11; n = 0 .. 4
    with t + 1 <, == and > n; repeated n-grams with several followers; theta 1 / 1.3 / 0.7 over duplicate ids; pad in the
    history; m at t = m - 1 and t = m)"""
    _needs_gpu()
    from bmhrl_amd import ops
    R, V, ld = 3, 37, 40
    g = torch.Generator().manual_seed(5)
    cases = ref.case_table()
    got, want = [], []
    for name, hist, t, n, m, theta in cases:
        lp = torch.log_softmax(torch.randn(R, V, generator=g) * 2, -1)
        lp[0, 5] = float("-inf")
        want.append(ref.apply_rules(lp.numpy(), hist, t, n, m, theta, END7, PAD))
        d = _padded(lp, ld).to(DEV)
        ops.logit_rules(d, ld, R, V, torch.from_numpy(hist).long().to(DEV), _word(t), n, m, theta, END7, PAD)
        got.append(d)
    got = torch.stack(got).cpu().numpy()
    for (name, *_), g_, w_ in zip(cases, got, want):
        assert np.array_equal(_bits(g_[:, :V]), _bits(w_)), name
        assert np.isnan(g_[:, V:]).all(), name
    assert len(cases) > 200


def test_logit_rules_large_vocabulary_and_full_history():
    _needs_gpu()
    from bmhrl_amd import ops
    rng = np.random.RandomState(1)
    # V = 10172, rows = 2: 30 tokens drawn from six ids spread over the vocabulary, its last id included
    V, R, t = 10172, 2, 29
    ids = np.array([0, 63, 64, 5000, 10170, V - 1])
    hist = ids[rng.randint(0, len(ids), size=(R, 31))]
    hist[:, 0] = START
    lp = torch.log_softmax(torch.randn(R, V, generator=torch.Generator().manual_seed(2)), -1)
    d = _padded(lp, V + 4).to(DEV)
    ops.logit_rules(d, V + 4, R, V, torch.from_numpy(hist).long().to(DEV), _word(t), 2, 40, 1.2, V - 1, PAD)
    want = ref.apply_rules(lp.numpy(), hist, t, 2, 40, 1.2, V - 1, PAD)
    out = d.cpu().numpy()
    assert np.array_equal(_bits(out[:, :V]), _bits(want)) and np.isnan(out[:, V:]).all()
    assert np.isinf(want).sum() >= 3 and (want != lp.numpy()).sum() <= R * (t + 2)
    # the history at the capacity limit: 256 positions, all of them read (t = 255)
    cap = ops.LOGIT_RULES_MAX_HIST
    assert cap == 256
    V, R = 37, 3
    for n, m, theta, t in ((4, cap, 1.3, cap - 1), (3, 0, 0.7, cap - 2), (cap, 0, 1.0, cap - 1), (1, 0, 1.0, cap - 1)):
        hist = rng.randint(0, V7, size=(R, cap))
        if n == cap:
            hist[1:] = 3                                          # one n-gram as long as the history: equal tokens repeat it
        lp = torch.log_softmax(torch.randn(R, V, generator=torch.Generator().manual_seed(n)), -1)
        d = _padded(lp, 40).to(DEV)
        ops.logit_rules(d, 40, R, V, torch.from_numpy(hist).long().to(DEV), _word(t), n, m, theta, END7, PAD)
        want = ref.apply_rules(lp.numpy(), hist, t, n, m, theta, END7, PAD)
        out = d.cpu().numpy()
        assert np.array_equal(_bits(out[:, :V]), _bits(want)) and np.isnan(out[:, V:]).all(), (n, m, theta, t)


def test_logit_rules_off_and_out_of_range_positions_write_nothing():
    _needs_gpu()
    from bmhrl_amd import ops
    R, V, ld = 3, 37, 40
    lp = _padded(torch.log_softmax(torch.randn(R, V, generator=torch.Generator().manual_seed(9)), -1), ld)
    lp[1, 3] = float("-inf")
    hist = torch.randint(0, V7, (R, 12), generator=torch.Generator().manual_seed(1)).to(DEV)
    before = lp.numpy().view(np.uint32).copy()
    d = lp.to(DEV)
    ops.logit_rules(d, ld, R, V, hist, _word(7), 0, 0, 1.0, END7, PAD)              # every rule off
    assert np.array_equal(d.cpu().numpy().view(np.uint32), before)
    for t in (12, -1, 10 ** 12):                                                    # positions the history does not hold
        ops.logit_rules(d, ld, R, V, hist, _word(t), 2, 20, 1.3, END7, PAD)
    assert np.array_equal(d.cpu().numpy().view(np.uint32), before)


def test_logit_rules_refuses_bad_arguments():
    _needs_gpu()
    from bmhrl_amd import _lib, ops
    R, V = 2, 16
    lp0 = torch.log_softmax(torch.randn(R, V, generator=torch.Generator().manual_seed(4)), -1)
    lp = lp0.to(DEV)
    hist = torch.full((R, 8), 3, dtype=torch.int64, device=DEV)
    t = _word(4)
    lib = _lib.load()
    call = lambda **kw: lib.bmhrl_logit_rules(lp.data_ptr(), kw.get("ld", V), kw.get("rows", R), kw.get("V", V), hist.data_ptr(),
                                              kw.get("ld_hist", 8), t.data_ptr(), kw.get("n", 2), kw.get("m", 6),
                                              kw.get("theta", 1.3), kw.get("end", 5), kw.get("pad", PAD), ops.stream())
    for bad in (dict(ld=V - 1), dict(rows=0), dict(rows=-1), dict(V=0), dict(n=-1), dict(m=-1), dict(theta=0.0), dict(theta=-1.0),
                dict(theta=float("inf")), dict(theta=float("nan")), dict(end=V), dict(end=-1), dict(pad=V), dict(pad=-1),
                dict(ld_hist=0), dict(ld_hist=ops.LOGIT_RULES_MAX_HIST + 1)):
        assert call(**bad) == -22, bad
    torch.cuda.synchronize()
    assert torch.equal(lp.cpu(), lp0)                                               # refused before any launch
    assert call() == 0
    torch.cuda.synchronize()
    assert not torch.equal(lp.cpu(), lp0)
    for kw in (dict(ngram=-1), dict(min_len=-1), dict(penalty=0.0), dict(penalty=float("nan")), dict(end_idx=V), dict(pad_idx=-1)):
        args = dict(ngram=2, min_len=6, penalty=1.3, end_idx=5, pad_idx=PAD)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.logit_rules(lp, V, R, V, hist, t, **args)
    with pytest.raises(ValueError):
        ops.logit_rules(lp, V, R, V, torch.zeros(R, ops.LOGIT_RULES_MAX_HIST + 1, dtype=torch.int64, device=DEV), t, 2, 0, 1.0, 5, PAD)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.logit_rules(lp0, V, R, V, hist, t, 2, 0, 1.0, 5, PAD)


# ----------------------------------------------------------------------------------------------------------- decoders
# The small synthetic agent of the decode / beam / sample GPU tests, one clip batch of B = 2.  CLIP_SEED = 6 is the clip for
# which tests/test_beam_gpu.py's _common_end finds an end token and whose unconstrained greedy decode repeats a bigram or stops
# before MIN_LEN tokens (on an MI355X both clips end at once: [start, end]); DRAW_SEED = 3 is the one sampler seed of 1 .. 5
# whose free samples of that clip repeat a bigram or stop early.  Both are asserted, not searched: a precondition that no
# longer holds fails the test.
V, B, L = 150, 2, 10
CLIP_SEED = 6
DRAW_SEED = 3
NGRAM, MIN_LEN, THETA = 2, 5, 1.2
RULES = dict(no_repeat_ngram=NGRAM, min_len=MIN_LEN, repetition_penalty=THETA)
OFF = dict(no_repeat_ngram=0, min_len=0, repetition_penalty=1.0)


@functools.lru_cache(None)
def _setup():
    from tests.test_beam_gpu import _common_end
    from bmhrl_amd.decode import greedy_decode
    agent = _agent(torch.device(DEV), V, rl_critic_score_threshhold=0.5)
    b = syn.synthetic_batch(B, 64, 96, 12, V, seed=CLIP_SEED)
    fs = {k: b[k].to(DEV) for k in ("rgb", "flow", "audio")}
    end = _common_end(agent, fs, L)
    assert end is not None, f"clip seed {CLIP_SEED}: no common end token"
    free = greedy_decode(agent, fs, L, START, end, PAD, AV, incremental=False)
    assert _loops_or_stops_early(_hyps(free, end), end), \
        f"clip seed {CLIP_SEED} neither loops nor stops early: the decoder tests would show nothing ({free.tolist()})"
    print(f"constrained decoders: clip seed {CLIP_SEED}, end token {end}")
    return agent, fs, end


def _hyps(toks, end):
    return [ref.upto_end(r, end) for r in toks.reshape(-1, toks.shape[-1]).tolist()]


def _loops_or_stops_early(hyps, end):
    return any(ref.repeats_ngram(h, NGRAM) for h in hyps) or any(h[-1] == end and len(h) - 1 <= MIN_LEN for h in hyps)


def _check_structure(hyps, end):
    for h in hyps:
        assert not ref.repeats_ngram(h, NGRAM), h
        assert h[-1] != end or len(h) - 1 >= MIN_LEN + 1, h


def _adjusted_teacher_forced(agent, fs, toks, end, rows_per_clip=1):
    """(rows, m + 1) tokens -> the full forward's log-probs of every position over the rows' own prefixes, adjusted by the
    restated rules: (rows, m, V) fp32"""
    from bmhrl_amd.model.masking import make_masks
    rep = {k: v.repeat_interleave(rows_per_clip, 0) for k, v in fs.items()}
    trg = toks[:, :-1].contiguous()
    with torch.no_grad():
        lp = agent.inference(((rep["rgb"], rep["flow"]), rep["audio"]), trg, make_masks(rep, trg, AV, PAD)).float().cpu().numpy()
    hist = toks.cpu().numpy()
    out = [ref.apply_rules(lp[:, t], hist, t, NGRAM, MIN_LEN, THETA, end, PAD) for t in range(lp.shape[1])]
    return torch.from_numpy(np.stack(out, 1)).to(DEV)


_CACHES = ("_incremental_decoders", "_beam_decoders", "_sample_decoders")


def test_rules_off_never_reach_the_kernel(monkeypatch):
    """With every rule off nothing of a decode reaches ops.logit_rules: the op is replaced by one that raises BEFORE the
    decoders exist, so that their eager token step, their graph capture (IncrementalDecoder.__init__) and -- for a decoder
    without a graph -- every single step run Python's _token_step under the stub.  The tokens, scores and log-probs equal
    those recorded before the stub went in."""
    _needs_gpu()
    from bmhrl_amd import ops
    from bmhrl_amd.decode import BeamDecoder, IncrementalDecoder, SampleDecoder, beam_decode, greedy_decode, sample_decode
    agent, fs, end = _setup()
    args = (agent, fs, L, START, end, PAD, AV)
    today = (greedy_decode(*args, return_first=True), beam_decode(*args, beam_size=3, return_scores=True, return_beams=True),
             sample_decode(*args, n=3, seed=11, top_p=0.9, return_samples=True))
    rerun = greedy_decode(*args, incremental=False)
    kept = {c: agent.__dict__.pop(c) for c in _CACHES}            # the cached decoders and their graphs, put back below
    steps = []

    def boom(*a, **k):
        raise AssertionError("logit_rules reached with every rule off")
    real_step = IncrementalDecoder._token_step

    def counted(self):
        steps.append(type(self).__name__)
        return real_step(self)
    monkeypatch.setattr(ops, "logit_rules", boom)
    monkeypatch.setattr(IncrementalDecoder, "_token_step", counted)
    try:
        # fresh decoders: the eager step and the capture of __init__ run under the stub, the decode replays that graph
        off = (greedy_decode(*args, return_first=True, **OFF),
               beam_decode(*args, beam_size=3, return_scores=True, return_beams=True, **OFF),
               sample_decode(*args, n=3, seed=11, top_p=0.9, return_samples=True, **OFF))
        for cls in (IncrementalDecoder, BeamDecoder, SampleDecoder):
            assert steps.count(cls.__name__) >= 2, steps          # the eager step and the capture of __init__
        assert all(len(agent.__dict__[c]) == 1 for c in _CACHES)
        for a, b in zip(today, off):
            assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))
        # without a graph every token is one Python _token_step under the stub
        for c in _CACHES:
            agent.__dict__.pop(c)
        monkeypatch.setattr(IncrementalDecoder, "use_graph", False)
        del steps[:]
        eager = (greedy_decode(*args, return_first=True, **OFF), greedy_decode(*args, return_first=True),
                 beam_decode(*args, beam_size=3, return_scores=True, return_beams=True, **OFF),
                 sample_decode(*args, n=3, seed=11, top_p=0.9, return_samples=True, **OFF))
        assert IncrementalDecoder.for_batch(agent, fs, L, START, end, PAD).graph is None
        for cls, toks in ((IncrementalDecoder, today[0][0]), (BeamDecoder, today[1][0]), (SampleDecoder, today[2][0])):
            assert steps.count(cls.__name__) >= 1 + toks.shape[1] - 1, steps        # __init__'s step + one per token
        for a, b in zip((today[0], today[0]) + today[1:], eager):
            assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))
        assert torch.equal(rerun, greedy_decode(*args, incremental=False, **OFF))
        # and the stub does catch a rule that is set
        with pytest.raises(AssertionError, match="logit_rules reached"):
            greedy_decode(*args, no_repeat_ngram=2)
    finally:
        monkeypatch.undo()
        agent.__dict__.update(kept)


def test_greedy_decoder_under_rules():
    _needs_gpu()
    from bmhrl_amd.decode import IncrementalDecoder, greedy_decode
    agent, fs, end = _setup()
    args = (agent, fs, L, START, end, PAD, AV)
    free = greedy_decode(*args)
    assert _loops_or_stops_early(_hyps(free, end), end), free
    dec = IncrementalDecoder.for_batch(agent, fs, L, START, end, PAD)
    assert dec.rules is None
    got, first = greedy_decode(*args, return_first=True, **RULES)
    assert dec.rules == (NGRAM, MIN_LEN, float(np.float32(THETA))) and dec.graph is not None
    _check_structure(_hyps(got, end), end)
    # against the full forward over its own prefixes, adjusted: the arg-max wherever the top-2 margin exceeds 1e-3, and the
    # re-run path's tokens up to the first step that is no such coin-flip (the criterion of tests/test_decode_gpu.py)
    adj = _adjusted_teacher_forced(agent, fs, got, end)
    assert torch.equal(torch.isinf(first), torch.isinf(adj[:, 0]))
    fin = torch.isfinite(first)
    assert float(((first - adj[:, 0])[fin].abs() / adj[:, 0][fin].abs().clamp_min(1.0)).max()) < 1e-3
    assert bool(torch.isinf(first[:, end]).all()) and bool(torch.isinf(first[:, START]).logical_not().all())
    top2 = adj.topk(2, -1).values
    sure = (top2[..., 0] - top2[..., 1]) > 1e-3
    assert torch.equal(got[:, 1:][sure], adj.argmax(-1)[sure])
    assert float(sure.float().mean()) > 0.8
    memo = greedy_decode(*args, incremental=False, **RULES)
    n_sure = int(sure.all(0).float().cumprod(0).sum())
    assert torch.equal(memo[:, :n_sure + 1], got[:, :n_sure + 1])
    _check_structure(_hyps(memo, end), end)
    # the rules are launch arguments of the captured step: off again, then on again, on the cached decoder
    assert torch.equal(greedy_decode(*args), free) and dec.rules is None
    assert torch.equal(greedy_decode(*args, **RULES), got)
    only_ban = greedy_decode(*args, no_repeat_ngram=1)
    for h in _hyps(only_ban, end):
        assert len(set(h)) == len(h), h                           # n = 1: no token twice
    assert IncrementalDecoder.for_batch(agent, fs, L, START, end, PAD) is dec
    print(f"greedy under rules: free {free.tolist()} -> {got.tolist()}, sure steps {n_sure}/{got.shape[1] - 1}")


def test_beam_decoder_under_rules():
    _needs_gpu()
    from bmhrl_amd.decode import BeamDecoder, beam_decode
    from tests.test_beam_gpu import _stable_order
    from bmhrl_amd.model.masking import make_masks
    agent, fs, end = _setup()
    K = 3
    args = (agent, fs, L, START, end, PAD, AV)
    free = beam_decode(*args, beam_size=K, return_beams=True)
    assert _loops_or_stops_early(_hyps(free[1], end), end), free[1]
    dec = BeamDecoder.for_batch(agent, fs, L, START, end, PAD, K)
    dec.set_rules(**RULES)
    with torch.no_grad():
        assert dec.begin(fs)
        steps = []
        for _ in range(L):
            dec.step()
            steps.append((dec.out[:, :dec.steps_run + 1].view(B, K, -1).clone(), dec.scores.view(B, K).clone()))
            if int(dec.last_live) < dec.steps_run:
                break
    toks, beams, scores = beam_decode(*args, beam_size=K, return_beams=True, **RULES)
    _check_structure(_hyps(beams, end), end)
    # the re-run path step by step under the restated rules; a step is sure for a sample when its K-th and (K+1)-th
    # candidates differ by at least 1e-3 (the criterion of tests/test_beam_gpu.py)
    rep = {k: v.repeat_interleave(K, 0) for k, v in fs.items()}
    x = ((rep["rgb"], rep["flow"]), rep["audio"])
    sc = torch.full((B, K), float("-inf"), device=DEV)
    sc[:, 0] = 0
    fin = torch.ones(B, K, dtype=torch.bool, device=DEV)
    fin[:, 0] = False
    hist = torch.full((B * K, 1), START, dtype=torch.long, device=DEV)
    snaps, sure = [], []
    with torch.no_grad():
        for i in range(L):
            lp = agent.inference(x, hist, make_masks(rep, hist, AV, PAD))[:, -1].float()
            lp = torch.from_numpy(ref.apply_rules(lp.cpu().numpy(), hist.cpu().numpy(), i, NGRAM, MIN_LEN, THETA, end, PAD)).to(DEV)
            cand = sc.unsqueeze(-1) + lp.view(B, K, V)
            only = torch.zeros_like(cand)
            only[..., PAD] = sc
            cand = torch.where(fin.unsqueeze(-1), only, cand).view(B, K * V)
            order = _stable_order(cand, fin, PAD)
            top = cand.gather(1, order[:, :K + 1])
            n_cand = (~fin).sum(1) * V + fin.sum(1)
            sure.append(~(top[:, K - 1] - top[:, K] < 1e-3) | (n_cand <= K))
            pick = order[:, :K]
            parent, tok = pick // V, pick % V
            sc = cand.gather(1, pick)
            fin = fin.gather(1, parent) | (tok == end)
            hist = hist.view(B, K, -1).gather(1, parent.unsqueeze(-1).expand(-1, -1, hist.shape[-1])).view(B * K, -1)
            hist = torch.cat([hist, tok.view(B * K, 1)], 1)
            snaps.append((hist.view(B, K, -1).clone(), sc.clone()))
            if bool(fin.all()):
                break
    sure = torch.stack(sure)
    assert float(sure.float().mean()) >= 0.8, sure
    for i in range(min(len(snaps), len(steps))):
        for s in range(B):
            if bool(sure[:i + 1, s].all()):
                assert torch.equal(steps[i][0][s], snaps[i][0][s]), (i, s)
                d = (steps[i][1][s].double() - snaps[i][1][s].double()).abs()
                d = d[torch.isfinite(snaps[i][1][s])]
                assert torch.equal(torch.isfinite(steps[i][1][s]), torch.isfinite(snaps[i][1][s]))
                assert d.numel() == 0 or float(d.max()) <= 1e-3 * max(1.0, float(snaps[i][1][s][torch.isfinite(snaps[i][1][s])].abs().max())) * (i + 1)
    forced = beam_decode(*args, beam_size=K, incremental=False, **RULES)
    if bool(sure.all()):
        assert torch.equal(forced, toks)
    _check_structure(_hyps(forced, end), end)
    # off again and on again on the cached decoder
    back = beam_decode(*args, beam_size=K, return_beams=True)
    assert dec.rules is None and all(torch.equal(a, b) for a, b in zip(back, free))
    again = beam_decode(*args, beam_size=K, return_beams=True, **RULES)
    assert torch.equal(again[1], beams) and torch.equal(again[2], scores)
    print(f"beam under rules: sure {float(sure.float().mean()):.2f}, best {toks.tolist()}")


def test_sample_decoder_under_rules():
    _needs_gpu()
    from bmhrl_amd.decode import SampleDecoder, _sample_choose, sample_decode, uniform01
    agent, fs, end = _setup()
    n = 3
    T, k, p = 1.0, 40, 0.9
    args = (agent, fs, L, START, end, PAD, AV)
    seed = DRAW_SEED
    kw = dict(n=n, temperature=T, top_k=k, top_p=p, seed=seed, return_samples=True)
    free = sample_decode(*args, **kw)
    assert _loops_or_stops_early(_hyps(free[1], end), end), (seed, free[1])
    toks, samples, sums, slp, slq = sample_decode(*args, **kw, **RULES)
    dec = SampleDecoder.for_batch(agent, fs, L, START, end, PAD, n)
    assert dec.rules is not None and dec.graph is not None
    _check_structure(_hyps(samples, end), end)
    m = slp.shape[-1]
    inc = samples.reshape(B * n, m + 1)
    # every step's recorded log-prob is the adjusted teacher-forced one of the sampled token
    adj = _adjusted_teacher_forced(agent, fs, inc, end, n)                          # (B*n, m, V)
    toks_n = inc[:, 1:]
    is_end = toks_n == end
    live = torch.ones_like(toks_n, dtype=torch.bool)
    live[:, 1:] = (is_end.cumsum(1) - is_end.long())[:, 1:] == 0
    lp_ref = adj.gather(-1, toks_n.unsqueeze(-1)).squeeze(-1)
    assert bool(torch.isfinite(lp_ref[live]).all())                                 # never a banned token
    err = float(((slp.reshape(B * n, m) - lp_ref).abs() * live)[live].max())
    assert err < 1e-3, err
    # the re-run path with the same seed: the same tokens up to a row's first low-margin step (tests/test_sample_gpu.py (c))
    forced = sample_decode(*args, incremental=False, **kw, **RULES)[1].reshape(B * n, -1)
    _check_structure(_hyps(forced, end), end)
    same_rows = 0
    for r in range(B * n):
        w = min(inc.shape[1], forced.shape[1])
        diff = (inc[r, :w] != forced[r, :w]).nonzero()
        if diff.numel() == 0:
            same_rows += 1
            continue
        s = int(diff[0]) - 1
        u = torch.from_numpy(uniform01(seed, [(r << 16) + s])).to(DEV)
        lp_s = adj[r, s].unsqueeze(0).double()
        top = torch.sort(lp_s[0], descending=True).values
        near = bool(top[k - 1] - top[k] < 2e-3)
        for du, dp in itertools.product((-1e-3, 0.0, 1e-3), (-1e-3, 0.0, 1e-3)):
            pk, _ = _sample_choose(lp_s, T, k, min(p + dp, 1.0), (u + du).clamp(0, 1 - 1e-9))
            near |= int(pk) != int(inc[r, s + 1]) or int(pk) != int(forced[r, s + 1])
        assert near, (r, s)
        # (the criterion above is tests/test_sample_gpu.py's and cannot fail at a step where the two paths differ; what does
        # carry weight: neither path drew a banned token there, and at least half the rows agree throughout)
        assert bool(torch.isfinite(adj[r, s, inc[r, s + 1]])) and bool(torch.isfinite(adj[r, s, forced[r, s + 1]])), (r, s)
    assert same_rows >= (B * n) // 2, same_rows
    # off again and on again on the cached decoder
    back = sample_decode(*args, **kw)
    assert dec.rules is None and all(torch.equal(a, b) for a, b in zip(back, free))
    again = sample_decode(*args, **kw, **RULES)
    assert torch.equal(again[1], samples) and torch.equal(again[2], sums) and torch.equal(again[3], slp)
    print(f"sample under rules: draw seed {seed}, step logp error {err:.2e}, rows equal to the re-run {same_rows}/{B * n}")
