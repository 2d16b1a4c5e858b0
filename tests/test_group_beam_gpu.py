"""Diverse (group) beam search on the GPU: bmhrl_group_beam_select (csrc/beam.hip) against the numpy restatement of
tests/group_beam_reference.py with equality on every output, and GroupBeamDecoder (the incremental token step on B*K rows plus
the grouped selection, one HIP graph per token) against the restatement on its own log-probs at every step, the re-run path,
the teacher-forced full forward, and the properties the rules promise."""
import numpy as np
import pytest
import torch

from bmhrl_amd import synthetic as syn
from tests import consensus_reference as cref
from tests import group_beam_reference as ref
from tests.test_beam_gpu import _common_end, _teacher_forced_scores
from tests.test_decode_gpu import _agent

pytestmark = pytest.mark.gpu

PAD, START = 1, 2
DEV = "cuda:0"
AV = "audio_video"
SENTINEL = -7
LAMBDAS = (0.0, 0.5, 1e4)


def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------- kernel
def _inputs(B, K, G, V, seed):
    """(logp (B, K, V), scores (B, K), finished (B, K)) as numpy.  Sample kinds, by b % 3 (B = 1: kind 0 with kind 1's holes):
    0 -- log-probs on a grid of 0.5 and integer scores, the groups' first beams equal: exact ties inside a group, ties created
         by the penalty 0.5 (a penalised candidate equals an unpenalised one), one token far above the rest that group after
         group chooses (c reaches G - 1), a finished beam where a group has more than one;
    1 -- -inf log-probs and -inf scores, finished beams, group 0 with every beam finished;
    2 -- every beam finished."""
    g = torch.Generator().manual_seed(seed)
    Kp = K // G
    logp = torch.log_softmax(torch.randn(B, K, V, generator=g) * 3, -1)
    scores = -torch.rand(B, K, generator=g) * 5
    finished = torch.zeros(B, K, dtype=torch.bool)
    for b in range(B):
        kind = b % 3
        if kind == 0:
            logp[b] = torch.round(logp[b] * 2) / 2
            scores[b] = torch.round(scores[b])
            logp[b, ::Kp] = logp[b, 0].clone()
            scores[b, ::Kp] = scores[b, 0].clone()
            logp[b, :, V // 3] = 3.0
            logp[b, :, V // 3 + 1] = 2.5                    # what V // 3 is worth to the group after its first choice
            if Kp > 1:
                finished[b, K - 1] = True
        if kind == 1 or B == 1:
            logp[b, :, ::7] = float("-inf")
            if K > 1:
                scores[b, K - 1] = float("-inf")
            if G > 1:
                finished[b, :Kp] = True
            if Kp > 1:
                finished[b, K - 2] = True
        if kind == 2:
            finished[b] = True
    return logp.numpy(), scores.numpy(), finished.numpy()


def _launch(lp, sc, fin, B, K, G, V, lam, end_idx, t=3, cols=9, alias=True, group=True):
    from bmhrl_amd import ops
    R = B * K
    d_lp = torch.from_numpy(lp).to(DEV).view(R, V)
    d_sc, d_fin = torch.from_numpy(sc).to(DEV).view(R), torch.from_numpy(fin).to(DEV).view(R).to(torch.uint8)
    parent = torch.full((R,), SENTINEL, dtype=torch.int32, device=DEV)
    tok = torch.full((R,), SENTINEL, dtype=torch.int64, device=DEV)
    big = torch.full((R, 12), SENTINEL, dtype=torch.int64, device=DEV)
    hist = big[:, :cols]
    tdev = torch.tensor([t], dtype=torch.int64, device=DEV)
    last_live = torch.zeros(1, dtype=torch.int32, device=DEV)
    out_sc, out_fin = (d_sc, d_fin) if alias else (torch.full_like(d_sc, SENTINEL), torch.full_like(d_fin, 9))
    if group:
        ops.group_beam_select(d_lp, V, d_sc, d_fin, parent, tok, hist, tdev, last_live, B, K, V, end_idx, PAD, G, lam,
                              scores_out=out_sc, finished_out=out_fin)
    else:
        ops.beam_select(d_lp, V, d_sc, d_fin, parent, tok, hist, tdev, last_live, B, K, V, end_idx, PAD, scores_out=out_sc,
                        finished_out=out_fin)
    if not alias:                                                    # the inputs are left alone
        assert np.array_equal(_bits(d_sc.cpu().numpy()), _bits(sc.reshape(-1)))
        assert np.array_equal(d_fin.cpu().numpy().astype(bool), fin.reshape(-1))
    return dict(scores=out_sc.cpu().numpy().reshape(B, K), finished=out_fin.cpu().numpy().reshape(B, K).astype(bool),
                parent=parent.cpu().numpy().reshape(B, K), tok=tok.cpu().numpy().reshape(B, K), hist=big.cpu().numpy(),
                last_live=int(last_live))


def _same(a, b):
    return (np.array_equal(_bits(a["scores"]), _bits(b["scores"])) and np.array_equal(a["finished"], b["finished"])
            and np.array_equal(a["parent"], b["parent"]) and np.array_equal(a["tok"], b["tok"])
            and np.array_equal(a["hist"], b["hist"]) and a["last_live"] == b["last_live"])


@pytest.mark.parametrize("V", [16, 150, 10172, 10173])
@pytest.mark.parametrize("K,G", [(2, 2), (4, 2), (4, 4), (6, 3), (8, 2), (16, 4), (16, 16), (3, 1), (16, 1)])
def test_group_beam_select_equals_the_restatement(K, G, V):
    _needs_gpu()
    end_idx = 5
    t = 3
    seen = dict(twice=0, penalty_tie=0, changed=0)
    for B in (1, 3):
        lp, sc, fin = _inputs(B, K, G, V, seed=K * 100003 + G * 1009 + V + B)
        plain = ref.group_beam_step(lp, sc, fin, G, 0.0, end_idx, PAD)
        for lam in LAMBDAS:
            want = ref.group_beam_step(lp, sc, fin, G, lam, end_idx, PAD, gaps=True)
            got = _launch(lp, sc, fin, B, K, G, V, lam, end_idx, t=t)
            key = (B, lam)
            assert np.array_equal(got["parent"], want[2]), key
            assert np.array_equal(got["tok"], want[3]), key
            assert np.array_equal(got["finished"], want[1]), key
            assert np.array_equal(_bits(got["scores"]), _bits(want[0])), key            # bit-equal, -inf included
            assert (got["parent"] // (K // G) == np.arange(K) // (K // G)).all(), key   # a parent lies in its own group
            # the history column and last_live as bmhrl_beam_select writes them
            assert np.array_equal(got["hist"][:, t + 1], want[3].reshape(-1)), key
            assert (np.delete(got["hist"], t + 1, axis=1) == SENTINEL).all(), key
            assert got["last_live"] == (0 if want[1].all() else t + 1), key
            # in place against separate outputs
            assert _same(got, _launch(lp, sc, fin, B, K, G, V, lam, end_idx, t=t, alias=False)), key
            if G == 1:                                                                  # beam search, for every lambda
                assert _same(got, _launch(lp, sc, fin, B, K, G, V, lam, end_idx, t=t, group=False)), key
            if lam == 0:
                assert all(np.array_equal(a, b) for a, b in zip(plain, want[:4]))
            live = ~fin[np.arange(B)[:, None], want[2]]       # the choices that were candidates of a live beam
            Kp = K // G
            for b in range(B):
                per_group = [set(want[3][b, g * Kp:(g + 1) * Kp][live[b, g * Kp:(g + 1) * Kp]].tolist()) for g in range(G)]
                earlier = [v for s in per_group[:-1] for v in s]
                seen["twice"] += int(any(earlier.count(v) >= 2 for v in earlier))
                seen["changed"] += int(lam > 0 and not np.array_equal(want[3][b], plain[3][b]))
                if lam >= 1e4 and V >= K + 8:                  # such a penalty and enough finite candidates: the groups'
                    assert sum(len(s) for s in per_group) == len(set().union(*per_group)), key     # live choices differ
            seen["penalty_tie"] += int(lam == 0.5 and G > 1 and bool((want[4] == 0).any()))
        # at t + 1 = hist_cols nothing is written past the row
        got = _launch(lp, sc, fin, B, K, G, V, 0.5, end_idx, t=t, cols=t + 1)
        assert (got["hist"] == SENTINEL).all() and np.array_equal(got["tok"], ref.group_beam_step(lp, sc, fin, G, 0.5, end_idx, PAD)[3])
    if G >= 3:
        assert seen["twice"] > 0                               # a token chosen by two earlier groups was on offer again
    if G > 1:
        assert seen["changed"] > 0
        if K == G:                                             # K' = 1: V // 3 at 3.0 - 0.5 meets V // 3 + 1 at 2.5 by construction
            assert seen["penalty_tie"] > 0                     # (other K': the penalised values stay on the grid of 0.5)


def test_refusals_leave_the_outputs_alone():
    _needs_gpu()
    from bmhrl_amd import _lib, ops
    B, K, G, V, cols = 2, 4, 2, 37, 6
    R = B * K
    lp = torch.log_softmax(torch.randn(R, V, generator=torch.Generator().manual_seed(1)), -1).to(DEV)
    sc = torch.zeros(R, device=DEV)
    fin = torch.zeros(R, dtype=torch.uint8, device=DEV)
    o_sc = torch.full((R,), float(SENTINEL), device=DEV)
    o_fin = torch.full((R,), 9, dtype=torch.uint8, device=DEV)
    parent = torch.full((R,), SENTINEL, dtype=torch.int32, device=DEV)
    tok = torch.full((R,), SENTINEL, dtype=torch.int64, device=DEV)
    hist = torch.full((R, cols), SENTINEL, dtype=torch.int64, device=DEV)
    t = torch.zeros(1, dtype=torch.int64, device=DEV)
    last_live = torch.full((1,), SENTINEL, dtype=torch.int32, device=DEV)
    lib = _lib.load()
    ptrs = dict(logp=lp, scores_in=sc, fin_in=fin, scores_out=o_sc, fin_out=o_fin, parent=parent, tok=tok, hist=hist, t=t,
                last_live=last_live)

    def call(**kw):
        a = {k: v.data_ptr() for k, v in ptrs.items()}
        a.update(ld=V, ldh=cols, hist_cols=cols, B=B, K=K, V=V, end=5, pad=PAD, G=G, lam=0.5)
        a.update(kw)
        return lib.bmhrl_group_beam_select(a["logp"], a["ld"], a["scores_in"], a["fin_in"], a["scores_out"], a["fin_out"],
                                           a["parent"], a["tok"], a["hist"], a["ldh"], a["hist_cols"], a["t"], a["last_live"],
                                           a["B"], a["K"], a["V"], a["end"], a["pad"], a["G"], a["lam"], ops.stream())
    bad = [{k: None} for k in ptrs]
    bad += [dict(B=0), dict(B=-1), dict(K=0), dict(K=-4), dict(K=17, G=1), dict(K=32, G=2), dict(G=0), dict(G=-2), dict(G=3),
            dict(G=8), dict(K=16, G=1, V=15, ld=15, pad=0), dict(K=16, G=2, V=7, ld=7), dict(lam=-0.5), dict(lam=-0.0 - 1e-30),
            dict(lam=float("inf")), dict(lam=float("-inf")), dict(lam=float("nan")), dict(ld=V - 1), dict(pad=V), dict(pad=-1),
            dict(hist_cols=0)]
    for kw in bad:
        assert call(**kw) == -22, kw
    torch.cuda.synchronize()
    assert bool((o_sc == SENTINEL).all()) and bool((o_fin == 9).all()) and bool((parent == SENTINEL).all())
    assert bool((tok == SENTINEL).all()) and bool((hist == SENTINEL).all()) and int(last_live) == SENTINEL
    assert call() == 0 and call(lam=0.0) == 0 and call(K=8, G=8, B=1) == 0 and call(K=8, G=2, B=1, V=4, ld=V) == 0
    torch.cuda.synchronize()
    assert bool((tok >= 0).all()) and bool((parent >= 0).all())
    args = dict(logp=lp, ld=V, scores=sc, finished=fin, parent=parent, tok=tok, hist=hist, t=t, last_live=last_live, B=B, K=K,
                V=V, end_idx=5, pad_idx=PAD, G=G, diversity_penalty=0.5)
    for kw in (dict(G=0), dict(G=3), dict(K=17, G=1), dict(diversity_penalty=-1.0), dict(diversity_penalty=float("nan")),
               dict(diversity_penalty=float("inf")), dict(logp=lp.double()), dict(scores=sc.double()), dict(finished=fin.bool()),
               dict(parent=parent.long()), dict(tok=tok.int()), dict(hist=hist.int()), dict(hist=hist.view(-1)),
               dict(t=t.int()), dict(last_live=last_live.long()), dict(ld=V - 1), dict(K=8, G=2, V=3, ld=3)):
        a = dict(args)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.group_beam_select(**a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.group_beam_select(**dict(args, logp=lp.cpu()))


# ------------------------------------------------------------------------------------------------------------ decoder
LAM = 0.5
L = 11


def _clip(B, Tv, Ta, V, seed=4):
    b = syn.synthetic_batch(B, Tv, Ta, 12, V, seed=seed)
    return {k: b[k].to(DEV) for k in ("rgb", "flow", "audio")}


def _begun(agent, fs, end, K, G, lam):
    from bmhrl_amd.decode import GroupBeamDecoder
    dec = GroupBeamDecoder.for_batch(agent, fs, L, START, end, PAD, K)
    dec.set_params(G, lam)
    dec.set_rules()
    assert dec.begin(fs)
    return dec


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("K,G", [(4, 2), (6, 3)])
@pytest.mark.parametrize("B,Tv,Ta,V", [(4, 64, 200, 200), (1, 40, 70, 120)])
def test_group_decoder_equals_the_restatement_at_every_step(B, Tv, Ta, V, K, G, graph, monkeypatch):
    """before each step the scores / flags are cloned, after it the step's own log-probs are read: the restatement on exactly
    those must give the step's tokens (history column), parents, scores and flags -- equality at every step, no exemptions"""
    _needs_gpu()
    from bmhrl_amd.decode import GroupBeamDecoder, beam_decode
    agent = _agent(torch.device(DEV), V, rl_critic_score_threshhold=0.5)
    fs = _clip(B, Tv, Ta, V)
    end = _common_end(agent, fs, L)
    end = -1 if end is None else end
    monkeypatch.setattr(GroupBeamDecoder, "use_graph", graph)
    with torch.no_grad():
        dec = GroupBeamDecoder.for_batch(agent, fs, L, START, end, PAD, K)
        assert dec.params == (1, 0.0) and (dec.graph is not None) == graph            # a cached decoder starts plain
        dec = _begun(agent, fs, end, K, G, LAM)
        assert dec.params == (G, LAM)
        s0, f0 = ref.initial_state(B, K, G)
        assert np.array_equal(dec.scores.view(B, K).cpu().numpy(), s0)
        assert np.array_equal(dec.finished.view(B, K).cpu().numpy().astype(bool), f0)
        changed = 0
        for i in range(L):
            sc, fin = dec.scores.view(B, K).cpu().numpy(), dec.finished.view(B, K).cpu().numpy().astype(bool)
            dec.step()
            lp = dec.logp.view(B, K, V).cpu().numpy()
            want = ref.group_beam_step(lp, sc, fin, G, LAM, end, PAD)
            assert np.array_equal(dec.out[:, i + 1].view(B, K).cpu().numpy(), want[3]), i
            assert np.array_equal(dec.tok.view(B, K).cpu().numpy(), want[3]), i
            assert np.array_equal(dec.parent.view(B, K).cpu().numpy(), want[2]), i
            assert np.array_equal(_bits(dec.scores.view(B, K).cpu().numpy()), _bits(want[0])), i
            assert np.array_equal(dec.finished.view(B, K).cpu().numpy().astype(bool), want[1]), i
            changed += int(not np.array_equal(want[3], ref.group_beam_step(lp, sc, fin, G, 0.0, end, PAD)[3]))
            if int(dec.last_live) < dec.steps_run:
                break
        assert changed > 0                                                            # the penalty steered a choice
        first = dec.result()
        # graph and eager runs are identical
        if graph:
            monkeypatch.setattr(GroupBeamDecoder, "use_graph", False)
            eager = GroupBeamDecoder(agent, B, dec.tv_cap, dec.ta_cap, L, START, end, PAD, DEV, beams=K, beam_groups=G,
                                     diversity_penalty=LAM)
            assert eager.graph is None and eager.begin(fs)
            e = eager.run()
            assert dec.begin(fs)
            d = dec.run()
            assert e[2] == d[2] and torch.equal(e[0], d[0]) and torch.equal(e[1], d[1])
            monkeypatch.setattr(GroupBeamDecoder, "use_graph", True)
        # set_params to another (G, lambda) and back reproduces the first result
        other = _begun(agent, fs, end, K, K, 2.0).run()
        assert other[0].shape[:2] == (B, K)
        again = _begun(agent, fs, end, K, G, LAM).run()
        assert again[2] == first[2] and torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
    # the cached decoder through a second clip equals a fresh one
    kw = dict(beam_size=K, beam_groups=G, diversity_penalty=LAM, return_beams=True, return_groups=True)
    got = beam_decode(agent, fs, L, START, end, PAD, AV, **kw)
    beam_decode(agent, _clip(B, Tv, Ta, V, seed=9), L, START, end, PAD, AV, **kw)
    assert all(torch.equal(a, b) for a, b in zip(got, beam_decode(agent, fs, L, START, end, PAD, AV, **kw)))
    assert len(agent.__dict__["_group_beam_decoders"]) == 1
    fresh = _agent(torch.device(DEV), V, rl_critic_score_threshhold=0.5)
    assert all(torch.equal(a, b) for a, b in zip(got, beam_decode(fresh, fs, L, START, end, PAD, AV, **kw)))


@pytest.mark.parametrize("K,G", [(4, 2), (6, 3)])
@pytest.mark.parametrize("B,Tv,Ta,V", [(4, 64, 200, 200), (1, 40, 70, 120)])
def test_group_decoder_against_rerun(B, Tv, Ta, V, K, G):
    """in the manner of test_beam_decoder_against_rerun: (a) every returned beam's score within 1e-3 relative of its
    teacher-forced sum; (b) the beams of _group_beam_rerun at every step, for samples whose every group was sure so far -- a
    group is sure when its K'-th and (K'+1)-th selection values differ by at least 1e-3; at least 0.8 of the (step, sample)
    pairs must be sure"""
    _needs_gpu()
    from bmhrl_amd import decode
    agent = _agent(torch.device(DEV), V, rl_critic_score_threshhold=0.5)
    fs = _clip(B, Tv, Ta, V)
    end = _common_end(agent, fs, L)
    end = -1 if end is None else end
    with torch.no_grad():
        dec = _begun(agent, fs, end, K, G, LAM)
        steps = []
        for _ in range(L):
            dec.step()
            steps.append((dec.out[:, :dec.steps_run + 1].view(B, K, -1).clone(), dec.scores.view(B, K).clone()))
            if int(dec.last_live) < dec.steps_run:
                break
        kw = dict(beam_size=K, beam_groups=G, diversity_penalty=LAM)
        toks, beams, scores = decode.beam_decode(agent, fs, L, START, end, PAD, AV, return_beams=True, **kw)
        tf, scale = _teacher_forced_scores(agent, fs, beams, end)
        err = float(((scores.double() - tf).abs() / scale).max())
        print(f"group beam K={K} G={G} B={B}: score error vs teacher-forced {err:.2e}")
        assert err < 1e-3, err
        trace = []
        decode._group_beam_rerun(agent, fs, L, START, end, PAD, AV, K, G, LAM, trace=trace)
    sure = []
    for st in trace:
        gap = ref.group_beam_step(st["logp"].cpu().numpy(), st["scores"].cpu().numpy(), st["finished"].cpu().numpy(), G, LAM,
                                  end, PAD, gaps=True)[4]
        sure.append(~(gap < 1e-3).any(1))                                 # (a NaN gap, -inf - -inf: sure)
    sure = np.stack(sure)
    print(f"group beam K={K} G={G} B={B}: sure {sure.mean():.2f}")
    assert sure.mean() >= 0.8, sure
    compared = 0
    for i in range(min(len(trace), len(steps))):
        for s in range(B):
            if sure[:i + 1, s].all():
                assert torch.equal(steps[i][0][s], trace[i]["hist"][s]), (i, s)
                d = (steps[i][1][s].double() - trace[i]["new_scores"][s].double()).abs()
                assert float(d.max()) <= 1e-3 * max(1.0, float(trace[i]["new_scores"][s].abs().max())) * (i + 1)
                compared += 1
    assert compared > 0
    if sure.all():
        forced = decode.beam_decode(agent, fs, L, START, end, PAD, AV, incremental=False, **kw)
        assert torch.equal(forced, toks)


# --------------------------------------------------------------------------------------------------------- properties
def _small():
    V = 200
    agent = _agent(torch.device(DEV), V, rl_critic_score_threshhold=0.5)
    fs = _clip(4, 64, 200, V)
    end = _common_end(agent, fs, L)
    return agent, fs, (-1 if end is None else end)


def test_no_penalty_is_the_small_beam_search_per_group():
    """lambda = 0, (K, G) = (4, 2): beams 2g + j equal beam j of beam_size = 2, tokens and scores bit for bit"""
    _needs_gpu()
    from bmhrl_amd.decode import BeamDecoder, GroupBeamDecoder, _incremental
    agent, fs, end = _small()
    with torch.no_grad():
        big = _incremental(GroupBeamDecoder, agent, fs, AV, L, START, end, PAD, 4, params=(2, 0.0)).run()
        small = _incremental(BeamDecoder, agent, fs, AV, L, START, end, PAD, 2).run()
    assert big[2] == small[2]
    for g in range(2):
        assert torch.equal(big[0][:, 2 * g:2 * g + 2], small[0])
        assert np.array_equal(_bits(big[1][:, 2 * g:2 * g + 2].cpu().numpy()), _bits(small[1].cpu().numpy()))


def test_a_large_penalty_makes_the_first_tokens_distinct():
    _needs_gpu()
    from bmhrl_amd.decode import beam_decode
    agent, fs, end = _small()
    _, beams, _, groups = beam_decode(agent, fs, L, START, end, PAD, AV, beam_size=4, beam_groups=4, diversity_penalty=1e4,
                                      return_beams=True, return_groups=True)
    for b in range(beams.shape[0]):
        assert len(set(beams[b, :, 1].tolist())) == 4, beams[b, :, :2]
        assert sorted(groups[b].tolist()) == [0, 1, 2, 3]


def test_one_group_takes_the_plain_beam_decoder():
    _needs_gpu()
    from bmhrl_amd.decode import beam_decode
    agent, fs, end = _small()
    want = beam_decode(agent, fs, L, START, end, PAD, AV, beam_size=4, return_scores=True, return_beams=True)
    got = beam_decode(agent, fs, L, START, end, PAD, AV, beam_size=4, beam_groups=1, diversity_penalty=0.5, return_scores=True,
                      return_beams=True)
    assert len(want) == len(got) == 4 and all(torch.equal(a, b) for a, b in zip(want, got))
    assert "_group_beam_decoders" not in agent.__dict__ and len(agent.__dict__["_beam_decoders"]) == 1


@pytest.mark.parametrize("graph", [True, False])
def test_groups_with_constraints_and_consensus(graph, monkeypatch):
    """no_repeat_ngram = 2, min_len = 3 and select="consensus" on grouped beams: the rules hold in every returned hypothesis,
    the utilities returned equal the restatement's of tests/consensus_reference.py on the returned hypotheses, and the caption
    is the one R7 picks from them"""
    _needs_gpu()
    from bmhrl_amd.decode import GroupBeamDecoder, beam_decode
    monkeypatch.setattr(GroupBeamDecoder, "use_graph", graph)
    agent, fs, end = _small()
    K = 4
    kw = dict(beam_size=K, beam_groups=2, diversity_penalty=LAM, no_repeat_ngram=2, min_len=3, return_scores=True, return_beams=True)
    base = beam_decode(agent, fs, L, START, end, PAD, AV, **kw)
    got = beam_decode(agent, fs, L, START, end, PAD, AV, select="consensus", consensus_n=2, return_groups=True, **kw)
    dec = next(iter(agent.__dict__["_group_beam_decoders"].values()))
    assert (dec.graph is not None) == graph and dec.rules is not None and dec.params == (2, LAM)
    assert len(base) == 4 and len(got) == 6 and torch.equal(got[2], base[2]) and torch.equal(got[3], base[3])
    beams, scores, groups, util = got[2].cpu(), got[3].cpu(), got[4].cpu(), got[5].cpu()
    assert groups.shape == (beams.shape[0], K) and all(sorted(r) == [0, 0, 1, 1] for r in groups.tolist())
    for row in beams.view(-1, beams.shape[-1]).tolist():
        words = cref.words(row, end)
        if end in row[1:]:
            assert row[1:].index(end) >= 3                                              # min_len
        grams = list(zip(words, words[1:]))
        assert len(grams) == len(set(grams))                                           # no bigram twice
    U = cref.utilities(cref.terms(beams.numpy(), end), 2)[0]
    assert np.array_equal(np.asarray(util.numpy(), dtype=np.float64).view(np.uint64), np.asarray(U, dtype=np.float64).view(np.uint64))
    picks = [cref.choose(U[b], range(K)) for b in range(U.shape[0])]                   # the beams arrive in rule 5's order
    caps = [cref.caption(beams[b, k].tolist(), end) for b, k in enumerate(picks)]
    n = max(len(c) for c in caps)
    assert got[0].tolist() == [c + [PAD] * (n - len(c)) for c in caps]
    assert torch.equal(got[1].cpu(), scores[torch.arange(len(picks)), torch.tensor(picks)])
