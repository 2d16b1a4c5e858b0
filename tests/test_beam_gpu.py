"""Beam-search decoding on the GPU: the plain select and the reorder kernel of csrc/beam.hip against torch restatements, and BeamDecoder (the
incremental token step on B*K rows plus the beam step, one HIP graph per token) against the greedy decoder, the
teacher-forced full forward and the re-run path of bmhrl_amd.decode.beam_decode."""
import time

import pytest
import torch

from bmhrl_amd import synthetic as syn
from tests.test_decode_gpu import _agent

pytestmark = pytest.mark.gpu

PAD, START = 1, 2
DEV = "cuda:0"


def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


# ------------------------------------------------------------------------------------------------------------ kernels
def _stable_order(cand, finished, pad_idx):
    """(B, K*V) -> every candidate index by score (descending, ties to the smaller index), the non-candidates (entries of a
    finished beam other than its pad entry) last"""
    B, K = finished.shape
    V = cand.shape[1] // K
    excluded = (finished.unsqueeze(-1) & (torch.arange(V, device=cand.device) != pad_idx)).view(B, K * V)
    order = torch.sort(-cand, dim=1, stable=True).indices
    return order.gather(1, torch.sort(excluded.gather(1, order).to(torch.uint8), dim=1, stable=True).indices)


def _select_reference(logp, scores, finished, K, V, end_idx, pad_idx):
    """rules 2-3 with stable sorts"""
    B = scores.numel() // K
    cand = scores.view(B, K, 1) + logp.view(B, K, V)
    only = torch.zeros_like(cand)
    only[..., pad_idx] = scores.view(B, K)
    cand = torch.where(finished.view(B, K, 1).bool(), only, cand).view(B, K * V)
    pick = _stable_order(cand, finished.view(B, K).bool(), pad_idx)[:, :K]
    parent, tok = pick // V, pick % V
    new_fin = finished.view(B, K).bool().gather(1, parent) | (tok == end_idx)
    return cand.gather(1, pick).view(-1), new_fin.view(-1), parent.view(-1).int(), tok.view(-1)


@pytest.mark.parametrize("V", [16, 150, 10172, 10173])
@pytest.mark.parametrize("K", [1, 2, 3, 4, 8, 16])
def test_beam_select_matches_stable_sort(K, V):
    """sample 0: log-probs on a coarse grid (many exact ties, also across beams with equal scores); sample 1: -inf beams,
    -inf log-probs and finished beams; sample 2: every beam finished; sample 3: plain"""
    _needs_gpu()
    from bmhrl_amd import ops
    g = torch.Generator().manual_seed(K * 100003 + V)
    B, R = 4, 4 * K
    logp = torch.log_softmax(torch.randn(R, V, generator=g) * 3, -1)
    logp[:K] = torch.round(logp[:K] * 2) / 2
    scores = -torch.rand(R, generator=g) * 5
    scores[:K] = torch.round(scores[:K])
    finished = torch.zeros(R, dtype=torch.uint8)
    if K > 1:
        scores[K + 1] = float("-inf")
        finished[K + K // 2] = 1
        scores[1] = scores[0]
        logp[1] = logp[0]                                    # two equal beams: every candidate of beam 1 ties with beam 0's
    logp[K:2 * K, ::7] = float("-inf")
    finished[2 * K:3 * K] = 1
    end_idx = 5
    ref_s, ref_f, ref_p, ref_t = _select_reference(logp, scores, finished, K, V, end_idx, PAD)
    d = lambda x: x.to(DEV)
    lp, sc, fin = d(logp), d(scores), d(finished)
    parent = torch.full((R,), -7, dtype=torch.int32, device=DEV)
    tok = torch.full((R,), -7, dtype=torch.int64, device=DEV)
    hist = torch.full((R, 9), -7, dtype=torch.int64, device=DEV)
    t = torch.tensor([3], dtype=torch.int64, device=DEV)
    last_live = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.beam_select(lp, V, sc, fin, parent, tok, hist, t, last_live, B, K, V, end_idx, PAD)
    torch.cuda.synchronize()
    assert torch.equal(parent.cpu(), ref_p)
    assert torch.equal(tok.cpu(), ref_t)
    assert torch.equal(fin.cpu().bool(), ref_f)
    assert torch.equal(sc.cpu(), ref_s)                   # bit-equal, -inf included
    assert torch.equal(hist[:, 4].cpu(), ref_t)
    assert bool((hist[:, :4] == -7).all()) and bool((hist[:, 5:] == -7).all())
    assert int(last_live) == (4 if not bool(ref_f.all()) else 0)
    assert bool(ref_f.view(B, K)[2].all())               # the all-finished sample stays finished, tokens pad
    assert bool((ref_t.view(B, K)[2] == PAD).all())
    # an all-finished batch leaves the word alone
    last_live.zero_()
    fin.fill_(1)
    ops.beam_select(lp, V, sc, fin, parent, tok, hist, t, last_live, B, K, V, end_idx, PAD)
    torch.cuda.synchronize()
    assert int(last_live) == 0 and bool((tok == PAD).all())


@pytest.mark.parametrize("t", ["first", "last"])
def test_beam_reorder_equals_index_select(t):
    """every buffer kind of the decoder: bf16 K|V rows, fp32 state without a position axis, int32 labels, fp32 goals,
    uint8 mask (rows not a multiple of 16 bytes), int64 history; positions after t keep their values"""
    _needs_gpu()
    from bmhrl_amd import ops
    g = torch.Generator().manual_seed(11)
    B, K, Lc = 3, 4, 24
    R = B * K
    bufs = [(torch.randn(R, Lc, 640, generator=g).to(torch.bfloat16), 640 * 2),
            (torch.randn(R, Lc, 96, generator=g).to(torch.bfloat16), 96 * 2),
            (torch.randn(R, 600, generator=g), 0),
            (torch.randint(0, 2, (R, Lc), generator=g, dtype=torch.int32), 4),
            (torch.randn(R, Lc, 64, generator=g), 64 * 4),
            (torch.randint(0, 2, (R, 1, Lc), generator=g, dtype=torch.uint8), 1),
            (torch.randint(0, 9999, (R, 11), generator=g), 8),
            (torch.randint(0, 9999, (R, 12), generator=g), 8)]              # 16-byte rows, odd positions moved
    parent = torch.stack([torch.randint(0, K, (K,), generator=g) for _ in range(B)]).view(-1)
    parent[0] = 0                                                        # an identity slot
    src_rows = (torch.arange(R) // K) * K + parent
    state = [b.clone().to(DEV) for b, _ in bufs]
    scratch = [torch.empty_like(s) for s in state]
    table, n_blocks = ops.beam_reorder_table([(s, c, pos) for s, c, (_, pos) in zip(state, scratch, bufs)], R, DEV)
    tt = 0 if t == "first" else Lc - 1
    tdev = torch.tensor([tt], dtype=torch.int64, device=DEV)
    par = parent.int().to(DEV)
    for phase in (0, 1):
        ops.beam_reorder(table, len(bufs), n_blocks, par, R, K, tdev, phase)
    torch.cuda.synchronize()
    for (orig, pos), got in zip(bufs, state):
        want = orig.index_select(0, src_rows)
        got = got.cpu()
        if pos == 0:
            assert torch.equal(got, want)
            continue
        per_row = orig[0].numel() * orig.element_size() // pos               # positions per row
        n = min(tt + 1, per_row)
        flat_g, flat_w, flat_o = got.view(R, per_row, -1), want.view(R, per_row, -1), orig.view(R, per_row, -1)
        assert torch.equal(flat_g[:, :n], flat_w[:, :n]), (orig.dtype, orig.shape)
        assert torch.equal(flat_g[:, n:], flat_o[:, n:]), (orig.dtype, orig.shape)        # later positions untouched


# ------------------------------------------------------------------------------------------------------------ decoder
def _pad_after_end(toks, end):
    out = toks.clone()
    is_end = out[:, 1:] == end
    out[:, 1:][(is_end.cumsum(1) - is_end.long()) > 0] = PAD
    return out


def _common_end(agent, fs, L):
    """a token every sample emits at some step of the free greedy decode, the earliest latest first occurrence"""
    from bmhrl_amd.decode import greedy_decode
    free = greedy_decode(agent, fs, L, START, -1, PAD, "audio_video", incremental=False)
    B = free.shape[0]
    cands = [int(v) for v in free[0, 1:].unique() if all((free[r, 1:] == v).any() for r in range(B)) and int(v) != PAD]
    if not cands:
        return None
    last_first = lambda v: max(int((free[r, 1:] == v).float().argmax()) for r in range(B))
    return min(cands, key=last_first)


def test_beam_one_equals_incremental_greedy():
    _needs_gpu()
    from bmhrl_amd.decode import BeamDecoder, beam_decode, greedy_decode
    V = 150
    agent = _agent(torch.device(DEV), V)
    b = syn.synthetic_batch(3, 64, 96, 12, V, seed=6)
    fs = {k: b[k].to(DEV) for k in ("rgb", "flow", "audio")}
    greedy = greedy_decode(agent, fs, 12, START, -1, PAD, "audio_video")
    beam = beam_decode(agent, fs, 12, START, -1, PAD, "audio_video", beam_size=1)
    assert isinstance(BeamDecoder.for_batch(agent, fs, 12, START, -1, PAD, 1), BeamDecoder)
    assert torch.equal(beam, greedy)
    end = _common_end(agent, fs, 12)
    if end is None:
        pytest.skip("no common token in this synthetic decode")
    greedy = greedy_decode(agent, fs, 12, START, end, PAD, "audio_video")
    old = BeamDecoder.check_every
    try:
        for every in (1, 4, 100):
            BeamDecoder.check_every = every
            beam = beam_decode(agent, fs, 12, START, end, PAD, "audio_video", beam_size=1)
            assert torch.equal(beam, _pad_after_end(greedy, end)), (every, beam, greedy)
    finally:
        BeamDecoder.check_every = old


def _rerun_steps(agent, fs, L, K, end):
    """the re-run path step by step: (snapshots [(tokens (B, K, i + 2), scores (B, K))], sure (steps, B)) where a step is
    sure for a sample when its K-th and (K+1)-th candidates differ by at least 1e-3"""
    from bmhrl_amd.model.masking import make_masks
    B = fs["audio"].shape[0]
    rep = {k: v.repeat_interleave(K, 0) for k, v in fs.items()}
    x = ((rep["rgb"], rep["flow"]), rep["audio"])
    scores = torch.full((B, K), float("-inf"), device=DEV)
    scores[:, 0] = 0
    fin = torch.ones(B, K, dtype=torch.bool, device=DEV)
    fin[:, 0] = False
    hist = torch.full((B * K, 1), START, dtype=torch.long, device=DEV)
    snaps, sure = [], []
    with torch.no_grad():
        for _ in range(L):
            lp = agent.inference(x, hist, make_masks(rep, hist, "audio_video", PAD))[:, -1].float()
            V = lp.shape[-1]
            cand = scores.unsqueeze(-1) + lp.view(B, K, V)
            only = torch.zeros_like(cand)
            only[..., PAD] = scores
            cand = torch.where(fin.unsqueeze(-1), only, cand).view(B, K * V)
            order = _stable_order(cand, fin, PAD)
            top = cand.gather(1, order[:, :K + 1])
            n_cand = (~fin).sum(1) * V + fin.sum(1)
            sure.append(~(top[:, K - 1] - top[:, K] < 1e-3) | (n_cand <= K))   # (a NaN gap, -inf - -inf: sure)
            pick = order[:, :K]
            parent, tok = pick // V, pick % V
            scores = cand.gather(1, pick)
            fin = fin.gather(1, parent) | (tok == end)
            hist = hist.view(B, K, -1).gather(1, parent.unsqueeze(-1).expand(-1, -1, hist.shape[-1])).view(B * K, -1)
            hist = torch.cat([hist, tok.view(B * K, 1)], 1)
            snaps.append((hist.view(B, K, -1).clone(), scores.clone()))
            if bool(fin.all()):
                break
    return snaps, torch.stack(sure)


def _teacher_forced_scores(agent, fs, beams, end):
    """per beam: sum of the full forward's log-probs of its own tokens up to its first end, and the error bound's scale"""
    from bmhrl_amd.model.masking import make_masks
    B, K, n1 = beams.shape
    rep = {k: v.repeat_interleave(K, 0) for k, v in fs.items()}
    toks = beams.reshape(B * K, n1)
    trg = toks[:, :-1].contiguous()
    with torch.no_grad():
        ref = agent.inference(((rep["rgb"], rep["flow"]), rep["audio"]), trg, make_masks(rep, trg, "audio_video", PAD))
    lp = ref.gather(-1, toks[:, 1:].unsqueeze(-1)).squeeze(-1).double()          # (B*K, n)
    is_end = toks[:, 1:] == end
    upto = (is_end.cumsum(1) - is_end.long()) == 0                               # positions up to the first end
    return (lp * upto).sum(1).view(B, K), (lp.abs().clamp_min(1.0) * upto).sum(1).view(B, K)


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("B,Tv,Ta,V", [(4, 64, 200, 200), (1, 40, 70, 120), (3, 100, 130, 300)])
@pytest.mark.parametrize("K", [2, 4])
def test_beam_decoder_against_rerun(K, B, Tv, Ta, V, graph):
    _needs_gpu()
    from bmhrl_amd.decode import BeamDecoder, beam_decode
    agent = _agent(torch.device(DEV), V, rl_critic_score_threshhold=0.5)
    b = syn.synthetic_batch(B, Tv, Ta, 12, V, seed=4)
    fs = {k: b[k].to(DEV) for k in ("rgb", "flow", "audio")}
    L = 11
    end = _common_end(agent, fs, L)
    end = -1 if end is None else end
    old = BeamDecoder.use_graph
    BeamDecoder.use_graph = graph
    try:
        dec = BeamDecoder.for_batch(agent, fs, L, START, end, PAD, K)
        assert (dec.graph is not None) == graph
        with torch.no_grad():
            assert dec.begin(fs)
            steps = []
            for _ in range(L):
                dec.step()
                steps.append((dec.out[:, :dec.steps_run + 1].view(B, K, -1).clone(), dec.scores.view(B, K).clone()))
                if int(dec.last_live) < dec.steps_run:
                    break
        toks, beams, scores = beam_decode(agent, fs, L, START, end, PAD, "audio_video", beam_size=K, return_beams=True)
        # (a) every beam's score is its teacher-forced full re-run's, summed up to its end
        ref, scale = _teacher_forced_scores(agent, fs, beams, end)
        err = float(((scores.double() - ref).abs() / scale).max())
        assert err < 1e-3, err
        # (b) the same beams as the re-run path while no sample's K-th / (K+1)-th candidates are within 1e-3
        snaps, sure = _rerun_steps(agent, fs, L, K, end)
        assert float(sure.float().mean()) >= 0.8, sure
        for i in range(min(len(snaps), len(steps))):
            for s in range(B):
                if bool(sure[:i + 1, s].all()):
                    assert torch.equal(steps[i][0][s], snaps[i][0][s]), (i, s)
                    d = (steps[i][1][s].double() - snaps[i][1][s].double()).abs()
                    assert float(d.max()) <= 1e-3 * max(1.0, float(snaps[i][1][s].abs().max())) * (i + 1)
        forced = beam_decode(agent, fs, L, START, end, PAD, "audio_video", beam_size=K, incremental=False)
        if bool(sure.all()):
            assert torch.equal(forced, toks)
        # (c) graph and no-graph results are identical
        if graph:
            BeamDecoder.use_graph = False
            eager = BeamDecoder(agent, B, dec.tv_cap, dec.ta_cap, L, START, end, PAD, DEV, beams=K)
            with torch.no_grad():
                assert eager.graph is None and eager.begin(fs)
                e_toks, e_scores, e_n = eager.run()
                assert dec.begin(fs)
                d_toks, d_scores, d_n = dec.run()
            assert e_n == d_n and torch.equal(e_toks, d_toks) and torch.equal(e_scores, d_scores)
            BeamDecoder.use_graph = graph
        # (d) the cached decoder through a second clip equals a fresh decoder
        b2 = syn.synthetic_batch(B, Tv, Ta, 12, V, seed=9)
        fs2 = {k: b2[k].to(DEV) for k in ("rgb", "flow", "audio")}
        beam_decode(agent, fs2, L, START, end, PAD, "audio_video", beam_size=K)
        again = beam_decode(agent, fs, L, START, end, PAD, "audio_video", beam_size=K)
        assert torch.equal(again, toks)
        print(f"beam K={K} B={B} graph={graph}: score error vs teacher-forced {err:.2e}, sure {float(sure.float().mean()):.2f}")
    finally:
        BeamDecoder.use_graph = old


def test_sample_without_memory_takes_the_rerun_path():
    _needs_gpu()
    from bmhrl_amd.decode import BeamDecoder, beam_decode
    V = 120
    agent = _agent(torch.device(DEV), V)
    b = syn.synthetic_batch(3, 40, 70, 12, V, seed=5)
    fs = {k: b[k].to(DEV) for k in ("rgb", "flow", "audio")}
    fs["audio"][1] = 0                                  # sample 1: no audio key at all
    with torch.no_grad():
        assert not BeamDecoder.for_batch(agent, fs, 8, START, -1, PAD, 3).begin(fs)
    got = beam_decode(agent, fs, 8, START, -1, PAD, "audio_video", beam_size=3, return_beams=True)
    want = beam_decode(agent, fs, 8, START, -1, PAD, "audio_video", beam_size=3, return_beams=True, incremental=False)
    for x, y in zip(got, want):                          # (the agent's log-probs of such a batch may be NaN)
        torch.testing.assert_close(x, y, rtol=0, atol=0, equal_nan=True)


# ------------------------------------------------------------------------------------------------------------ timing
def _time_ms(fn):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def config2_times(agent=None):
    """greedy incremental, beam K in {1, 4, 8}, greedy over the batch repeated 4x: ms for 30 tokens (B=16, Tv=256, Ta=800,
    V=10172, end_idx=-1)"""
    from bmhrl_amd.decode import beam_decode, greedy_decode
    V = 10172
    agent = agent or _agent(torch.device(DEV), V)
    b = syn.synthetic_batch(16, 256, 800, 30, V, seed=0)
    fs = {k: b[k].to(DEV) for k in ("rgb", "flow", "audio")}
    fs4 = {k: v.repeat(4, 1, 1) for k, v in fs.items()}
    times = {}
    times["greedy"], g = _time_ms(lambda: greedy_decode(agent, fs, 30, START, -1, PAD, "audio_video"))
    for K in (1, 4, 8):
        times[f"beam{K}"], toks = _time_ms(lambda: beam_decode(agent, fs, 30, START, -1, PAD, "audio_video", beam_size=K))
        assert toks.shape == (16, 31)
        if K == 1:
            assert torch.equal(toks, g)
    times["greedy_x4"], g4 = _time_ms(lambda: greedy_decode(agent, fs4, 30, START, -1, PAD, "audio_video"))
    assert g4.shape == (64, 31)
    return times


def test_beam_speed_config2():
    _needs_gpu()
    times = config2_times()
    print("decode of 30 tokens, B=16 (ms): " + ", ".join(f"{k} {v:.1f}" for k, v in times.items()) +
          f"; beam4 / greedy_x4 {times['beam4'] / times['greedy_x4']:.2f}, beam1 / greedy {times['beam1'] / times['greedy']:.2f}")
    assert times["beam4"] <= 1.5 * times["greedy_x4"]
    assert times["beam1"] <= 1.3 * times["greedy"]
