"""Paragraph-aware decoding on the GPU: bmhrl_logit_rules_ctx (csrc/constrain.hip) against the numpy
restatement of tests/context_rules_reference.py, bit-equal; the off state; the incremental decoders under context rules against
their re-run paths, compared the way tests/test_constrain_gpu.py compares them under the plain rules; a cached decoder with a
second context; and predict.caption_segments(paragraph=True) end to end."""
import copy

import numpy as np
import pytest
import torch

from tests import context_rules_reference as ref
from tests.test_constrain_gpu import AV, B, DEV, L, PAD, START, V, _hyps, _setup
from tests.test_predict_gpu import setup  # noqa: F401  (the tiny whole-video configuration, as a fixture of this module)

pytestmark = pytest.mark.gpu

SENTINEL = 12345.5


def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _word(t):
    return torch.tensor([t], dtype=torch.int64, device=DEV)


# ------------------------------------------------------------------------------------------------------------- kernel
def _run_table(cases):
    """every case through ops.logit_rules_ctx on rows 1 .. R of an (R + 2)-row buffer of V + 3 columns -> the buffers"""
    from bmhrl_amd import ops
    out = []
    for i, c in enumerate(cases):
        R, Vc = c["hist"].shape[0], c["V"]
        ld = Vc + 3
        buf = torch.full((R + 2, ld), SENTINEL)
        buf[1:R + 1, :Vc] = torch.from_numpy(ref.case_logp(c, i))
        buf[1:R + 1, Vc:] = float("nan")
        d = buf.to(DEV)
        ops.logit_rules_ctx(d[1:R + 1], ld, R, Vc, torch.from_numpy(c["hist"]).to(DEV), _word(c["t"]), c["n"], c["m"], c["theta"],
                            c["end"], c["pad"], torch.from_numpy(c["ctx"]).to(DEV), c["rpc"], c["n_c"], c["theta_c"])
        out.append(d)
    return [d.cpu().numpy() for d in out]


def test_logit_rules_ctx_matches_the_restatement():
    """the case table of tests/context_rules_reference.py: R = 6, V = 37 in rows of 40 floats whose tail holds NaN, rows_per_ctx
    1 and 3, C in {1, n_c - 1, n_c, 63, 64, 65, 1024}, t in {0, n_c - 2, n_c - 1, 11}, n_c = 0 .. 4, theta_c x theta x n; gaps at
    every position of a matching window; matches at both ends; several followers; one id 22 times; ids in s and the context;
    -inf under C1; gaps only; ids -1, V, 2^40; V = 65; V = 10172 with 256 history and 1024 context tokens.  Twice: equal bits."""
    _needs_gpu()
    cases = ref.case_table()
    first = _run_table(cases)
    second = _run_table(cases)
    changed = 0
    for i, (c, got, again) in enumerate(zip(cases, first, second)):
        R, Vc = c["hist"].shape[0], c["V"]
        lp = ref.case_logp(c, i)
        want = ref.want(c, lp)
        assert np.array_equal(_bits(got[1:R + 1, :Vc]), _bits(want)), c["name"]
        assert np.isnan(got[1:R + 1, Vc:]).all(), c["name"]                       # columns V .. ld - 1
        assert (got[0] == SENTINEL).all() and (got[R + 1] == SENTINEL).all(), c["name"]   # other rows
        assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), c["name"]
        changed += not np.array_equal(_bits(want), _bits(lp))
    assert len(cases) > 200 and changed > len(cases) // 2


def test_logit_rules_ctx_out_of_range_positions_and_off_arguments_write_nothing():
    _needs_gpu()
    from bmhrl_amd import ops
    R, Vc, ld = 6, 37, 40
    lp = torch.full((R, ld), float("nan"))
    lp[:, :Vc] = torch.log_softmax(torch.randn(R, Vc, generator=torch.Generator().manual_seed(9)), -1)
    hist = torch.randint(0, 7, (R, 12), generator=torch.Generator().manual_seed(1)).to(DEV)
    ctx = torch.randint(0, 7, (2, 70), generator=torch.Generator().manual_seed(2)).to(DEV)
    before = lp.numpy().view(np.uint32).copy()
    d = lp.to(DEV)
    ops.logit_rules_ctx(d, ld, R, Vc, hist, _word(7), 0, 0, 1.0, ref.END, PAD, ctx, 3, 0, 1.0)       # every rule off
    assert np.array_equal(d.cpu().numpy().view(np.uint32), before)
    for t in (12, -1, 10 ** 12):                                                    # positions the history does not hold
        ops.logit_rules_ctx(d, ld, R, Vc, hist, _word(t), 2, 20, 1.3, ref.END, PAD, ctx, 3, 2, 1.3)
    assert np.array_equal(d.cpu().numpy().view(np.uint32), before)
    ops.logit_rules_ctx(d, ld, R, Vc, hist, _word(7), 0, 0, 1.0, ref.END, PAD, ctx, 3, 2, 1.3)
    assert not np.array_equal(d.cpu().numpy().view(np.uint32), before)


def test_logit_rules_ctx_refuses_bad_arguments():
    _needs_gpu()
    from bmhrl_amd import _lib, ops
    R, Vc = 4, 16
    lp0 = torch.log_softmax(torch.randn(R, Vc, generator=torch.Generator().manual_seed(4)), -1)
    lp = lp0.to(DEV)
    hist = torch.full((R, 8), 3, dtype=torch.int64, device=DEV)
    ctx = torch.full((2, 9), 3, dtype=torch.int64, device=DEV)
    t = _word(4)
    lib = _lib.load()

    def call(**kw):
        Vk = kw.get("V", Vc)
        return lib.bmhrl_logit_rules_ctx(lp.data_ptr(), kw.get("ld", Vk), kw.get("rows", R), Vk, hist.data_ptr(),
                                         kw.get("ld_hist", 8), t.data_ptr(), kw.get("n", 2), kw.get("m", 6), kw.get("theta", 1.3),
                                         kw.get("end", 5), kw.get("pad", PAD), kw.get("ctx", ctx.data_ptr()), kw.get("ld_ctx", 9),
                                         kw.get("rpc", 2), kw.get("n_c", 2), kw.get("theta_c", 1.3), ops.stream())
    inf, nan = float("inf"), float("nan")
    for bad in (dict(ld=Vc - 1), dict(rows=0), dict(rows=-1), dict(V=0), dict(n=-1), dict(m=-1), dict(theta=0.0), dict(theta=-1.0),
                dict(theta=inf), dict(theta=nan), dict(end=Vc), dict(end=-1), dict(pad=Vc), dict(pad=-1), dict(ld_hist=0),
                dict(ld_hist=ops.LOGIT_RULES_MAX_HIST + 1),                         # ... what bmhrl_logit_rules refuses, and:
                dict(ctx=None), dict(ld_ctx=0), dict(ld_ctx=-1), dict(ld_ctx=ops.LOGIT_RULES_MAX_CTX + 1), dict(rpc=0), dict(rpc=-2),
                dict(rpc=3), dict(rpc=8), dict(n_c=-1), dict(theta_c=0.0), dict(theta_c=-1.0), dict(theta_c=inf), dict(theta_c=nan),
                dict(V=ops.LOGIT_RULES_CTX_MAX_V + 1)):
        assert call(**bad) == -22, bad
    torch.cuda.synchronize()
    assert torch.equal(lp.cpu(), lp0)                                               # refused before any launch
    assert call() == 0 and call(rpc=1, ld_ctx=4) == 0 and call(rpc=4, ld_ctx=1) == 0
    torch.cuda.synchronize()
    assert not torch.equal(lp.cpu(), lp0)
    good = dict(ngram=2, min_len=6, penalty=1.3, end_idx=5, pad_idx=PAD, ctx=ctx, rows_per_ctx=2, ctx_ngram=2, ctx_penalty=1.3)
    for kw in (dict(ngram=-1), dict(min_len=-1), dict(penalty=0.0), dict(penalty=nan), dict(end_idx=Vc), dict(pad_idx=-1),
               dict(ctx_ngram=-1), dict(ctx_penalty=0.0), dict(ctx_penalty=nan), dict(ctx_penalty=inf), dict(rows_per_ctx=0),
               dict(rows_per_ctx=3), dict(rows_per_ctx=1), dict(ctx=ctx.int()), dict(ctx=ctx[0]), dict(ctx=ctx.t()),
               dict(ctx=torch.zeros(2, ops.LOGIT_RULES_MAX_CTX + 1, dtype=torch.int64, device=DEV))):
        with pytest.raises(ValueError):
            ops.logit_rules_ctx(lp, Vc, R, Vc, hist, t, **{**good, **kw})
    with pytest.raises(ValueError):
        big = ops.LOGIT_RULES_CTX_MAX_V + 1
        ops.logit_rules_ctx(torch.zeros(R, big, device=DEV), big, R, big, hist, t, **good)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.logit_rules_ctx(lp0, Vc, R, Vc, hist, t, **good)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.logit_rules_ctx(lp, Vc, R, Vc, hist, t, **{**good, "ctx": ctx.cpu()})
    ops.logit_rules_ctx(lp, Vc, R, Vc, hist, t, **good)


# ----------------------------------------------------------------------------------------------------------- decoders
NGRAM, MIN_LEN = 3, 4
RULES = dict(no_repeat_ngram=NGRAM, min_len=MIN_LEN)
CTX_RULES = dict(context_ngram=3, context_penalty=1.2)
_CACHES = ("_incremental_decoders", "_beam_decoders", "_group_beam_decoders", "_sample_decoders")


def _context_of(toks, end):
    """per clip the words of a decode's own output, as caption_segments(paragraph=True) would hand them on"""
    from bmhrl_amd.predict import caption_tokens
    return [caption_tokens(row, end, PAD) for row in toks.tolist()]


def _contexts():
    """(agent, fs, end, the contexts of the two clips: what greedy decoding under the plain rules says about them)"""
    from bmhrl_amd.decode import greedy_decode
    agent, fs, end = _setup()
    prev = greedy_decode(agent, fs, L, START, end, PAD, AV, **RULES)
    ctx = _context_of(prev, end)
    assert all(len(c) >= MIN_LEN for c in ctx), ctx
    return agent, fs, end, ctx, prev


def _ctx_array(ctx):
    width = max(len(c) for c in ctx)
    return np.array([c + [PAD] * (width - len(c)) for c in ctx], dtype=np.int64)


def _no_shared_ngram(hyps, ctx, rows_per_clip):
    for r, h in enumerate(hyps):
        assert not ref.shares_ngram(h[1:], ctx[r // rows_per_clip], 3, V, PAD), (r, h, ctx[r // rows_per_clip])


def _restated(lp, hist, t, end, ctx, rows_per_clip):
    return ref.apply_context_rules(lp, hist, t, NGRAM, MIN_LEN, 1.0, end, PAD, _ctx_array(ctx), rows_per_clip, 3, 1.2)


def _adjusted_teacher_forced(agent, fs, toks, end, ctx, rows_per_clip=1):
    """(rows, m + 1) tokens -> the full forward's log-probs of every position over the rows' own prefixes, adjusted by the
    restated rules 1, C1, 2, C2, 3: (rows, m, V) fp32"""
    from bmhrl_amd.model.masking import make_masks
    rep = {k: v.repeat_interleave(rows_per_clip, 0) for k, v in fs.items()}
    trg = toks[:, :-1].contiguous()
    with torch.no_grad():
        lp = agent.inference(((rep["rgb"], rep["flow"]), rep["audio"]), trg, make_masks(rep, trg, AV, PAD)).float().cpu().numpy()
    hist = toks.cpu().numpy()
    out = [_restated(lp[:, t], hist, t, end, ctx, rows_per_clip) for t in range(lp.shape[1])]
    return torch.from_numpy(np.stack(out, 1)).to(DEV)


def test_off_state_never_reaches_the_kernel(monkeypatch):
    """With no context, or with n_c = 0 and theta_c = 1, nothing of a decode reaches ops.logit_rules_ctx: the op is replaced
    by one that raises BEFORE the decoders exist, so that their eager token step and their graph captures run under the stub;
    the tokens equal those of the same calls without the new keywords, recorded before the stub went in."""
    _needs_gpu()
    from bmhrl_amd import ops
    from bmhrl_amd.decode import beam_decode, greedy_decode, sample_decode
    agent, fs, end, ctx, _ = _contexts()
    args = (agent, fs, L, START, end, PAD, AV)
    decodes = (lambda **k: greedy_decode(*args, **k), lambda **k: beam_decode(*args, beam_size=2, **k),
               lambda **k: beam_decode(*args, beam_size=2, beam_groups=2, **k),
               lambda **k: sample_decode(*args, n=2, seed=11, top_p=0.9, **k))
    today = [(d(), d(**RULES)) for d in decodes]
    kept = {c: agent.__dict__.pop(c) for c in _CACHES if c in agent.__dict__}

    def boom(*a, **k):
        raise AssertionError("logit_rules_ctx reached in the off state")
    monkeypatch.setattr(ops, "logit_rules_ctx", boom)
    try:
        for d, (free, ruled) in zip(decodes, today):
            assert torch.equal(d(**RULES), ruled)                                                   # plain rules only
            assert torch.equal(d(**RULES, context=None, **CTX_RULES), ruled)                        # rules, but no context
            assert torch.equal(d(**RULES, context=ctx, context_ngram=0, context_penalty=1.0), ruled)  # a context, no rule
            assert torch.equal(d(context=None, **CTX_RULES), free)
            assert torch.equal(d(context=ctx, context_ngram=0, context_penalty=1.0), free)
            assert torch.equal(d(), free)
        assert all(len(agent.__dict__[c]) == 1 for c in _CACHES)
        # and the stub does catch a rule that is set with a context present
        for d in decodes:
            with pytest.raises(AssertionError, match="logit_rules_ctx reached"):
                d(context=ctx, context_ngram=2)
    finally:
        monkeypatch.undo()
        for c in _CACHES:
            agent.__dict__.pop(c, None)
        agent.__dict__.update(kept)


def test_greedy_decoder_under_context_rules():
    _needs_gpu()
    from bmhrl_amd.decode import IncrementalDecoder, greedy_decode
    agent, fs, end, ctx, prev = _contexts()
    args = (agent, fs, L, START, end, PAD, AV)
    kw = dict(context=ctx, **RULES, **CTX_RULES)
    assert all(ref.shares_ngram(h[1:], c, 3, V, PAD) for h, c in zip(_hyps(prev, end), ctx))         # without: a repeat
    got, first = greedy_decode(*args, return_first=True, **kw)
    dec = IncrementalDecoder.for_batch(agent, fs, L, START, end, PAD)
    assert dec.ctx_rules == (3, float(np.float32(1.2))) and dec.has_context and dec.graph is not None
    assert torch.equal(dec.ctx[:, :len(ctx[0])].cpu(), torch.tensor(_ctx_array(ctx))[:, :len(ctx[0])])
    _no_shared_ngram(_hyps(got, end), ctx, 1)
    # against the full forward over its own prefixes, adjusted: the arg-max wherever the top-2 margin exceeds 1e-3, and the
    # re-run path's tokens up to the first step that is no such coin-flip (the criterion of tests/test_constrain_gpu.py)
    adj = _adjusted_teacher_forced(agent, fs, got, end, ctx)
    assert torch.equal(torch.isinf(first), torch.isinf(adj[:, 0]))
    fin = torch.isfinite(first)
    assert float(((first - adj[:, 0])[fin].abs() / adj[:, 0][fin].abs().clamp_min(1.0)).max()) < 1e-3
    top2 = adj.topk(2, -1).values
    sure = (top2[..., 0] - top2[..., 1]) > 1e-3
    assert torch.equal(got[:, 1:][sure], adj.argmax(-1)[sure])
    assert float(sure.float().mean()) > 0.8
    memo = greedy_decode(*args, incremental=False, **kw)
    n_sure = int(sure.all(0).float().cumprod(0).sum())
    assert torch.equal(memo[:, :n_sure + 1], got[:, :n_sure + 1])
    _no_shared_ngram(_hyps(memo, end), ctx, 1)
    # off again, then on again, on the cached decoder; a tensor context is a list context
    assert torch.equal(greedy_decode(*args, **RULES), prev) and not dec.has_context and dec.ctx_rules is None
    assert torch.equal(greedy_decode(*args, **{**kw, "context": torch.tensor(_ctx_array(ctx), device=DEV)}), got)
    assert IncrementalDecoder.for_batch(agent, fs, L, START, end, PAD) is dec
    print(f"greedy under context rules: {prev.tolist()} -> {got.tolist()}, sure steps {n_sure}/{got.shape[1] - 1}")


def _reference_beam_steps(agent, fs, end, K, G, ctx):
    """beam search (G = 1) or group beam search with lambda = 0 (every group its own K / G-beam search) over full re-runs
    under the restated rules, step by step -> (snapshots (tokens (B, K, i + 2), scores (B, K)), sure (steps, B)): a step is
    sure for a clip when in every group the K'-th and (K' + 1)-th candidates differ by at least 1e-3"""
    from bmhrl_amd.model.masking import make_masks
    from tests.test_beam_gpu import _stable_order
    Kp = K // G
    rep = {k: v.repeat_interleave(K, 0) for k, v in fs.items()}
    x = ((rep["rgb"], rep["flow"]), rep["audio"])
    sc = torch.full((B, K), float("-inf"), device=DEV)
    sc[:, ::Kp] = 0
    fin = torch.ones(B, K, dtype=torch.bool, device=DEV)
    fin[:, ::Kp] = False
    hist = torch.full((B * K, 1), START, dtype=torch.long, device=DEV)
    snaps, sure = [], []
    with torch.no_grad():
        for i in range(L):
            lp = agent.inference(x, hist, make_masks(rep, hist, AV, PAD))[:, -1].float()
            lp = torch.from_numpy(_restated(lp.cpu().numpy(), hist.cpu().numpy(), i, end, ctx, K)).to(DEV)
            cand = sc.unsqueeze(-1) + lp.view(B, K, V)
            only = torch.zeros_like(cand)
            only[..., PAD] = sc
            cand = torch.where(fin.unsqueeze(-1), only, cand)
            parents, toks, scores = [], [], []
            ok = torch.ones(B, dtype=torch.bool, device=DEV)
            for g in range(G):
                c_g, f_g = cand[:, g * Kp:(g + 1) * Kp].reshape(B, Kp * V), fin[:, g * Kp:(g + 1) * Kp]
                order = _stable_order(c_g, f_g, PAD)
                top = c_g.gather(1, order[:, :Kp + 1])
                n_cand = (~f_g).sum(1) * V + f_g.sum(1)
                ok &= ~(top[:, Kp - 1] - top[:, Kp] < 1e-3) | (n_cand <= Kp)
                pick = order[:, :Kp]
                parents.append(pick // V + g * Kp)
                toks.append(pick % V)
                scores.append(c_g.gather(1, pick))
            sure.append(ok)
            parent, tok, sc = torch.cat(parents, 1), torch.cat(toks, 1), torch.cat(scores, 1)
            fin = fin.gather(1, parent) | (tok == end)
            hist = hist.view(B, K, -1).gather(1, parent.unsqueeze(-1).expand(-1, -1, hist.shape[-1])).view(B * K, -1)
            hist = torch.cat([hist, tok.view(B * K, 1)], 1)
            snaps.append((hist.view(B, K, -1).clone(), sc.clone()))
            if bool(fin.all()):
                break
    return snaps, torch.stack(sure)


@pytest.mark.parametrize("G", [1, 2])
def test_beam_decoder_under_context_rules(G):
    _needs_gpu()
    from bmhrl_amd.decode import BeamDecoder, GroupBeamDecoder, beam_decode
    agent, fs, end, _, _ = _contexts()
    K = 2
    args = (agent, fs, L, START, end, PAD, AV)
    # the context: what the same search says without one -- which it would therefore say again
    free = beam_decode(*args, beam_size=K, beam_groups=G, **RULES)
    ctx = _context_of(free, end)
    assert all(len(c) >= MIN_LEN for c in ctx), ctx
    kw = dict(beam_size=K, beam_groups=G, context=ctx, **RULES, **CTX_RULES)
    toks, beams, scores = beam_decode(*args, return_beams=True, **kw)
    _no_shared_ngram(_hyps(beams, end), ctx, K)
    cls = BeamDecoder if G == 1 else GroupBeamDecoder
    dec = cls.for_batch(agent, fs, L, START, end, PAD, K)
    assert dec.ctx_rules is not None and dec.has_context and dec.graph is not None
    with torch.no_grad():                                         # (the decoder is as beam_decode left it: rules and context set)
        assert dec.begin(fs)
        steps = []
        for _ in range(L):
            dec.step()
            steps.append((dec.out[:, :dec.steps_run + 1].view(B, K, -1).clone(), dec.scores.view(B, K).clone()))
            if int(dec.last_live) < dec.steps_run:
                break
    snaps, sure = _reference_beam_steps(agent, fs, end, K, G, ctx)
    assert float(sure.float().mean()) >= 0.8, sure
    for i in range(min(len(snaps), len(steps))):
        for s in range(B):
            if bool(sure[:i + 1, s].all()):
                assert torch.equal(steps[i][0][s], snaps[i][0][s]), (i, s)
                finite = torch.isfinite(snaps[i][1][s])
                assert torch.equal(torch.isfinite(steps[i][1][s]), finite)
                d = (steps[i][1][s].double() - snaps[i][1][s].double()).abs()[finite]
                assert d.numel() == 0 or float(d.max()) <= 1e-3 * max(1.0, float(snaps[i][1][s][finite].abs().max())) * (i + 1)
    forced = beam_decode(*args, incremental=False, return_beams=True, **kw)
    if bool(sure.all()):
        assert torch.equal(forced[0], toks)
    _no_shared_ngram(_hyps(forced[1], end), ctx, K)
    assert torch.equal(beam_decode(*args, beam_size=K, beam_groups=G, **RULES), free)          # off again on the cached decoder
    again = beam_decode(*args, return_beams=True, **kw)
    assert torch.equal(again[1], beams) and torch.equal(again[2], scores)
    print(f"beam (G = {G}) under context rules: sure {float(sure.float().mean()):.2f}, best {toks.tolist()}")


def test_sample_decoder_under_context_rules():
    _needs_gpu()
    from bmhrl_amd.decode import SampleDecoder, sample_decode
    agent, fs, end, ctx, _ = _contexts()
    n = 2
    args = (agent, fs, L, START, end, PAD, AV)
    kw = dict(n=n, temperature=1.0, top_k=40, top_p=0.9, seed=3, return_samples=True, context=ctx, **RULES, **CTX_RULES)
    toks, samples, sums, slp, slq = sample_decode(*args, **kw)
    dec = SampleDecoder.for_batch(agent, fs, L, START, end, PAD, n)
    assert dec.ctx_rules is not None and dec.has_context and dec.graph is not None
    _no_shared_ngram(_hyps(samples, end), ctx, n)
    m = slp.shape[-1]
    inc = samples.reshape(B * n, m + 1)
    # every step's recorded log-prob is the adjusted teacher-forced one of the sampled token, never a banned one
    adj = _adjusted_teacher_forced(agent, fs, inc, end, ctx, n)                    # (B*n, m, V)
    toks_n = inc[:, 1:]
    is_end = toks_n == end
    live = torch.ones_like(toks_n, dtype=torch.bool)
    live[:, 1:] = (is_end.cumsum(1) - is_end.long())[:, 1:] == 0
    lp_ref = adj.gather(-1, toks_n.unsqueeze(-1)).squeeze(-1)
    assert bool(torch.isfinite(lp_ref[live]).all())
    err = float(((slp.reshape(B * n, m) - lp_ref).abs() * live)[live].max())
    assert err < 1e-3, err
    # the re-run path with the same seed: neither path draws a banned token, and at least half the rows agree throughout
    forced = sample_decode(*args, incremental=False, **kw)[1]
    _no_shared_ngram(_hyps(forced, end), ctx, n)
    forced = forced.reshape(B * n, -1)
    same_rows = 0
    for r in range(B * n):
        w = min(inc.shape[1], forced.shape[1])
        diff = (inc[r, :w] != forced[r, :w]).nonzero()
        if diff.numel() == 0:
            same_rows += 1
            continue
        s = int(diff[0]) - 1
        assert bool(torch.isfinite(adj[r, s, inc[r, s + 1]])) and bool(torch.isfinite(adj[r, s, forced[r, s + 1]])), (r, s)
    assert same_rows >= (B * n) // 2, same_rows
    again = sample_decode(*args, **kw)
    assert torch.equal(again[1], samples) and torch.equal(again[2], sums) and torch.equal(again[3], slp)
    print(f"sample under context rules: step logp error {err:.2e}, rows equal to the re-run {same_rows}/{B * n}")


def test_a_second_context_on_the_cached_decoder():
    """the static context buffer is refilled and nothing of the first context is captured: a second clip batch with another
    context gives what a decoder built for it gives"""
    _needs_gpu()
    from bmhrl_amd.decode import BeamDecoder, IncrementalDecoder, beam_decode, greedy_decode
    agent, fs, end, ctx, _ = _contexts()
    args = (agent, fs, L, START, end, PAD, AV)
    kw = dict(**RULES, **CTX_RULES)
    first_g = greedy_decode(*args, context=ctx, **kw)
    first_b = beam_decode(*args, beam_size=2, context=ctx, **kw)
    # the second context: what the first pass said, after the first context (longer, and other words)
    ctx2 = [c + [PAD] + s for c, s in zip(ctx, _context_of(first_g, end))]
    dec_g, dec_b = IncrementalDecoder.for_batch(agent, fs, L, START, end, PAD), BeamDecoder.for_batch(agent, fs, L, START, end, PAD, 2)
    graphs = (dec_g.graph, dec_b.graph)
    second_g = greedy_decode(*args, context=ctx2, **kw)
    second_b = beam_decode(*args, beam_size=2, context=ctx2, **kw)
    assert (dec_g.graph, dec_b.graph) == graphs                   # a new context needs no capture
    assert not torch.equal(second_g, first_g)
    _no_shared_ngram(_hyps(second_g, end), ctx2, 1)
    _no_shared_ngram(_hyps(second_b, end), ctx2, 1)
    # a shorter context after a longer one leaves nothing of the longer one behind
    assert torch.equal(greedy_decode(*args, context=ctx, **kw), first_g) and torch.equal(beam_decode(*args, beam_size=2, context=ctx, **kw), first_b)
    kept = {c: agent.__dict__.pop(c) for c in _CACHES if c in agent.__dict__}
    try:
        assert torch.equal(greedy_decode(*args, context=ctx2, **kw), second_g)
        assert torch.equal(beam_decode(*args, beam_size=2, context=ctx2, **kw), second_b)
        assert IncrementalDecoder.for_batch(agent, fs, L, START, end, PAD) is not dec_g
    finally:
        for c in _CACHES:
            agent.__dict__.pop(c, None)
        agent.__dict__.update(kept)


# ---------------------------------------------------------------------------------------------------------- end to end
TWICE = [[(0.0, 22.0), (0.0, 22.0), (5.5, 16.25)], [(12.0, 20.5), (12.0, 20.5), (0.12346, 7.0)]]


@pytest.mark.parametrize("which", ["greedy", "beam2"])
def test_paragraph_mode_end_to_end(setup, which):  # noqa: F811
    """two videos whose segment lists hold the same (start, end) twice: identical clips give identical sentences, so without
    paragraph mode the paragraph repeats 4-grams across sentences (Para_XRE_4 > 0); with it and context_ngram = 4 none is left"""
    from bmhrl_amd.decode import beam_decoder, greedy_decoder
    from bmhrl_amd.evaluate import paragraph_stats
    from bmhrl_amd.predict import caption_segments
    s = setup
    cfg = copy.copy(s.cfg)
    cfg.max_len = 10
    decoder = {"greedy": greedy_decoder(min_len=6, context_ngram=4), "beam2": beam_decoder(2, min_len=6, context_ngram=4)}[which]
    words = lambda results: [[cap["sentence"].lower().split() for cap in caps] for caps in results]   # noqa: E731
    # (one chunk for all six clips without paragraph mode: the identical clips are rows of one batch)
    para = caption_segments(cfg, s.agent, s.features, TWICE, decoder, s.ds, batch_size=8, paragraph=True)
    flat = caption_segments(cfg, s.agent, s.features, TWICE, decoder, s.ds, batch_size=8, paragraph=False)
    assert [[c["timestamp"] for c in caps] for caps in para] == [[list(t) for t in segs] for segs in TWICE]
    on, off = paragraph_stats(words(para), s.dev), paragraph_stats(words(flat), s.dev)
    print(f"{which}: paragraph mode {words(para)}\n cross/total at n = 4: on {on[:, 3, [3, 0]].tolist()}, off {off[:, 3, [3, 0]].tolist()}")
    for g in range(2):
        assert on[g, 3, 0] > 0 and on[g, 3, 3] == 0, (g, on[g, 3])             # total > 0, cross == 0 at n = 4
        assert off[g, 3, 3] > 0, (g, off[g, 3])
