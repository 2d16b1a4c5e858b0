"""Sampled decoding on the GPU: bmhrl_sample_step (csrc/sample.hip) against a float64 restatement of the sampling rules of
bmhrl_amd/decode.py, its determinism and RNG, and SampleDecoder (the incremental token step on B*n rows plus the sample
step, one HIP graph per token) against greedy decoding, the teacher-forced full forward and the re-run path."""
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from bmhrl_amd import synthetic as syn
from tests.test_decode_gpu import _agent

pytestmark = pytest.mark.gpu

PAD, START, END = 1, 2, 5
DEV = "cuda:0"
MARGIN = 1e-5


def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _u(seed, rows, t, row_offset=0):
    from bmhrl_amd.decode import uniform01
    idx = (np.arange(rows, dtype=np.uint64) + np.uint64(row_offset)) << np.uint64(16)
    return torch.from_numpy(uniform01(seed, idx + np.uint64(t)))


def restate(lp32, T, k, p, u):
    """rules 2-4 in float64, written out independently of decode.py: (pick, logq, decidable) per row.  decidable: the draw
    lies more than MARGIN * sum(q) from every cumulative boundary of the kept tokens and top_p * sum(q) more than that from
    every prefix mass of the order (T = 0 / k = 1: always)."""
    R, V = lp32.shape
    dev = lp32.device
    lp = lp32.double()
    T = float(np.float32(T))
    p = float(np.float32(p))
    arg = lp.argmax(1)
    if T == 0 or k == 1:
        return arg, torch.zeros(R, dtype=torch.float64, device=dev), torch.ones(R, dtype=torch.bool, device=dev)
    M = lp.max(1, keepdim=True).values
    q = torch.exp((lp - M) / T)
    q[~torch.isfinite(lp)] = 0
    order = torch.sort(-lp32, dim=1, stable=True).indices
    cum = q.gather(1, order).cumsum(1)
    S = cum[:, -1]
    c = torch.full((R,), V, device=dev)
    if 0 < k < V:
        c = torch.clamp(c, max=k)
    ok = torch.ones(R, dtype=torch.bool, device=dev)
    if p < 1:
        cp = ((cum < p * S.unsqueeze(1)).sum(1) + 1).clamp(max=V)
        c = torch.minimum(c, cp)
        ok &= (cum - p * S.unsqueeze(1)).abs().min(1).values > MARGIN * S
    keep_sorted = torch.arange(V, device=dev).unsqueeze(0) < c.unsqueeze(1)
    kept = torch.zeros(R, V, dtype=torch.bool, device=dev).scatter(1, order, keep_sorted)
    kq = torch.where(kept, q, torch.zeros_like(q))
    incl = kq.cumsum(1)
    mass = incl[:, -1]
    thr = u.to(dev).double() * mass
    cand = kept & (q > 0)
    hit = cand & (incl > thr.unsqueeze(1))
    last = V - 1 - cand.flip(1).to(torch.uint8).argmax(1)
    pick = torch.where(hit.any(1), hit.to(torch.uint8).argmax(1), last)
    gap = torch.where(cand, (incl - thr.unsqueeze(1)).abs(), torch.full_like(incl, float("inf"))).min(1).values
    ok &= gap > MARGIN * S
    logq = torch.log(q.gather(1, pick.unsqueeze(1)).squeeze(1) / mass)
    return pick, logq, ok


def _inputs(R, V, seed):
    """log-probs with exact ties (row 0), -inf entries (row 1), one finite entry (row 2); every 5th row from 3 on finished"""
    g = torch.Generator().manual_seed(seed)
    lp = torch.log_softmax(torch.randn(R, V, generator=g) * 6, -1)
    lp[0] = torch.round(lp[0] * 2) / 2
    if R > 1:
        lp[1, ::7] = float("-inf")
    if R > 2:
        lp[2] = float("-inf")
        lp[2, V // 3] = -0.25
    fin = torch.zeros(R, dtype=torch.uint8)
    fin[3::5] = 1
    return lp, fin


GRID_T = [0.0, 0.5, 1.0, 1.7]
GRID_K = [0, 1, 5, 50, "V+3"]
GRID_P = [1.0, 0.9, 0.5, 1e-6]


@pytest.mark.parametrize("V", [16, 150, 10172, 10173])
@pytest.mark.parametrize("R", [1, 7, 64, 256])
def test_sample_step_matches_float64_rules(R, V):
    _needs_gpu()
    from bmhrl_amd import ops
    lp, fin0 = _inputs(R, V, R * 1000 + V)
    ld = V + 1 if R % 2 else V
    buf = torch.full((R, ld), float("nan"))
    buf[:, :V] = lp
    d_lp = buf.to(DEV)
    t, cols, seed, seed_word = 3, 9, 1234567, 89
    u = _u(seed + seed_word, R, t, row_offset=5)
    tdev = torch.tensor([t], dtype=torch.int64, device=DEV)
    sdev = torch.tensor([seed_word], dtype=torch.int64, device=DEV)
    sums0 = torch.randn(R, generator=torch.Generator().manual_seed(7))
    live = fin0 == 0
    skipped = total = 0
    for T, k, p in itertools.product(GRID_T, GRID_K, GRID_P):
        k = V + 3 if k == "V+3" else k
        fin = fin0.to(DEV)
        tok = torch.full((R,), -7, dtype=torch.int64, device=DEV)
        out = torch.full((R, cols), -7, dtype=torch.int64, device=DEV)
        slp = torch.full((R, cols), -7.0, device=DEV)
        slq = torch.full((R, cols), -7.0, device=DEV)
        sums = sums0.to(DEV)
        ops.sample_step(d_lp, ld, R, V, T, k, p, seed, sdev, tdev, END, PAD, fin, tok, out, sums, slp, slq, row_offset=5)
        torch.cuda.synchronize()
        tok, out, slp, slq, sums, fin = (x.cpu() for x in (tok, out, slp, slq, sums, fin))
        pick, logq, ok = (x.cpu() for x in restate(d_lp[:, :V], T, k, p, u))
        what = (T, k, p)
        # finished rows: pad, nothing added
        assert bool((tok[~live] == PAD).all()) and bool((out[~live, t + 1] == PAD).all()), what
        assert torch.equal(sums[~live], sums0[~live]) and bool((slp[~live, t] == 0).all()) and bool((slq[~live, t] == 0).all())
        # live rows: the model log-prob of the kernel's own pick, exactly; the same token where the draw is decidable
        got = tok[live]
        assert bool(((got >= 0) & (got < V)).all()), what
        g_lp = lp[live].gather(1, got.unsqueeze(1)).squeeze(1)
        assert torch.equal(slp[live, t], g_lp), what
        assert torch.equal(sums[live], sums0[live] + g_lp), what
        assert bool(torch.isfinite(g_lp).all()), what                    # never a token of probability zero
        sure = ok[live]
        total += int(sure.numel())
        skipped += int((~sure).sum())
        assert torch.equal(got[sure], pick[live][sure]), (what, got[sure], pick[live][sure])
        err = (slq[live, t].double() - logq[live]).abs()[sure]
        assert float(err.max()) < 1e-5 if err.numel() else True, (what, float(err.max()))
        assert torch.equal(out[:, t + 1], tok) and torch.equal(fin.bool(), fin0.bool() | (tok == END))
        other = torch.ones(cols, dtype=torch.bool)
        other[t + 1] = False
        assert bool((out[:, other] == -7).all()), what                 # only column t + 1 of the history
        other = torch.ones(cols, dtype=torch.bool)
        other[t] = False
        assert bool((slp[:, other] == -7).all()) and bool((slq[:, other] == -7).all()), what
        if R > 2:                                                       # the single finite entry is always drawn
            assert int(tok[2]) == V // 3
    print(f"R={R} V={V}: {skipped} of {total} draws within {MARGIN} of a boundary")
    assert skipped <= 0.01 * total


def _launch(lp, R, V, T, k, p, seed_word, t=0):
    from bmhrl_amd import ops
    fin = torch.zeros(R, dtype=torch.uint8, device=DEV)
    tok = torch.zeros(R, dtype=torch.int64, device=DEV)
    out = torch.zeros(R, 2, dtype=torch.int64, device=DEV)
    slq = torch.zeros(R, 2, device=DEV)
    sums = torch.zeros(R, device=DEV)
    ops.sample_step(lp, V, R, V, T, k, p, 0, torch.tensor([seed_word], dtype=torch.int64, device=DEV),
                    torch.tensor([t], dtype=torch.int64, device=DEV), -1, PAD, fin, tok, out, sums, None, slq)
    return tok, slq[:, t], sums


@pytest.mark.parametrize("T,k,p", [(1.0, 0, 1.0), (1.0, 50, 0.9), (0.8, 0, 0.9), (1.3, 200, 1.0)])
def test_sample_step_is_deterministic_and_seeded(T, k, p):
    _needs_gpu()
    R, V = 64, 10172
    g = torch.Generator().manual_seed(3)
    lp = torch.log_softmax(torch.randn(R, V, generator=g) * 2, -1).to(DEV)
    a = _launch(lp, R, V, T, k, p, 11)
    b = _launch(lp, R, V, T, k, p, 11)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)                                       # bit-identical, step logq included
    c = _launch(lp, R, V, T, k, p, 12)
    assert int((c[0] != a[0]).sum()) >= R // 4                         # a new seed word: new draws
    d = _launch(lp, R, V, T, k, p, 11, t=1)
    assert int((d[0] != a[0]).sum()) >= R // 4                         # a new step: new draws


@pytest.mark.parametrize("T,k,p", [(1.0, 0, 1.0), (0.7, 10, 1.0), (1.5, 0, 0.8), (1.0, 12, 0.9)])
def test_sample_step_frequencies(T, k, p):
    """one row replicated over 65536 rows: the pick frequencies follow the tempered, truncated softmax (chi-square at a
    fixed seed: deterministic)"""
    _needs_gpu()
    R, V = 65536, 40
    row = torch.log_softmax(torch.randn(V, generator=torch.Generator().manual_seed(5)) * 1.5, -1)
    lp = row.expand(R, V).contiguous().to(DEV)
    tok, _, _ = _launch(lp, R, V, T, k, p, 2024)
    counts = torch.bincount(tok.cpu(), minlength=V).double()
    q = torch.exp((row.double() - row.max()) / float(np.float32(T)))
    order = torch.sort(-row, stable=True).indices
    cum = q[order].cumsum(0)
    c = V if k == 0 else k
    if p < 1:
        c = min(c, int((cum < float(np.float32(p)) * cum[-1]).sum()) + 1)
    kept = torch.zeros(V, dtype=torch.bool)
    kept[order[:c]] = True
    assert int(counts[~kept].sum()) == 0
    expect = R * q[kept] / q[kept].sum()
    chi2 = float(((counts[kept] - expect) ** 2 / expect).sum())
    dof = int(kept.sum()) - 1
    print(f"T={T} k={k} p={p}: chi2 {chi2:.1f} over {dof} dof")
    assert chi2 < dof + 6 * (2 * dof) ** 0.5 + 10


def test_sample_step_refuses_bad_arguments():
    _needs_gpu()
    from bmhrl_amd import _lib, ops
    R, V = 2, 16
    lp = torch.zeros(R, V, device=DEV)
    w = lambda dt: torch.zeros(R, dtype=dt, device=DEV)
    out = torch.zeros(R, 3, dtype=torch.int64, device=DEV)
    t = torch.zeros(1, dtype=torch.int64, device=DEV)
    lib = _lib.load()
    call = lambda **kw: lib.bmhrl_sample_step(lp.data_ptr(), kw.get("ld", V), R, kw.get("V", V), kw.get("T", 1.0),
                                              kw.get("k", 0), kw.get("p", 1.0), 0, None, t.data_ptr(), 0, -1, kw.get("pad", 1),
                                              w(torch.uint8).data_ptr(), w(torch.int64).data_ptr(), out.data_ptr(), 3,
                                              w(torch.float32).data_ptr(), None, None, ops.stream())
    assert call() == 0
    for bad in (dict(T=-1.0), dict(T=float("inf")), dict(k=-1), dict(p=0.0), dict(p=1.5), dict(p=float("nan")),
                dict(V=0), dict(V=ops.SAMPLE_MAX_V + 1, ld=ops.SAMPLE_MAX_V + 1), dict(ld=V - 1), dict(pad=V)):
        assert call(**bad) == -22, bad
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ decoder
def _batch(B, Tv, Ta, V, seed):
    b = syn.synthetic_batch(B, Tv, Ta, 12, V, seed=seed)
    return {k: b[k].to(DEV) for k in ("rgb", "flow", "audio")}


def _pad_after_end(toks, end):
    out = toks.clone()
    is_end = out[:, 1:] == end
    out[:, 1:][(is_end.cumsum(1) - is_end.long()) > 0] = PAD
    return out


def _teacher_forced(agent, fs, samples):
    """(B, n, m + 1) samples -> the full forward's log-probs (B*n, m, V) of every position"""
    from bmhrl_amd.model.masking import make_masks
    B, n, m1 = samples.shape
    rep = {k: v.repeat_interleave(n, 0) for k, v in fs.items()}
    trg = samples.reshape(B * n, m1)[:, :-1].contiguous()
    with torch.no_grad():
        return agent.inference(((rep["rgb"], rep["flow"]), rep["audio"]), trg, make_masks(rep, trg, "audio_video", PAD)).float()


def test_top_k_one_equals_incremental_greedy():
    _needs_gpu()
    from bmhrl_amd.decode import SampleDecoder, greedy_decode, sample_decode
    from tests.test_beam_gpu import _common_end
    V = 150
    agent = _agent(torch.device(DEV), V)
    fs = _batch(3, 64, 96, V, 6)
    greedy = greedy_decode(agent, fs, 12, START, -1, PAD, "audio_video")
    got = sample_decode(agent, fs, 12, START, -1, PAD, "audio_video", n=1, top_k=1, seed=3)
    assert isinstance(SampleDecoder.for_batch(agent, fs, 12, START, -1, PAD, 1), SampleDecoder)
    assert torch.equal(got, greedy)
    end = _common_end(agent, fs, 12)
    if end is not None:
        greedy = greedy_decode(agent, fs, 12, START, end, PAD, "audio_video")
        for kw in (dict(top_k=1), dict(temperature=0.0), dict(top_p=1e-9)):
            got = sample_decode(agent, fs, 12, START, end, PAD, "audio_video", n=1, seed=4, **kw)
            assert torch.equal(got, _pad_after_end(greedy, end)), kw


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("n", [2, 4])
def test_sample_decoder_against_teacher_forcing_and_rerun(n, graph):
    _needs_gpu()
    from bmhrl_amd.decode import SampleDecoder, _sample_choose, sample_decode, uniform01
    V, B, L = 200, 3, 10
    agent = _agent(torch.device(DEV), V, rl_critic_score_threshhold=0.5)
    fs = _batch(B, 64, 200, V, 4)
    T, k, p = 1.2, 40, 0.9
    old = SampleDecoder.use_graph
    SampleDecoder.use_graph = graph
    try:
        dec = SampleDecoder.for_batch(agent, fs, L, START, END, PAD, n)
        assert (dec.graph is not None) == graph
        toks, samples, sums, slp, slq = sample_decode(agent, fs, L, START, END, PAD, "audio_video", n=n, temperature=T,
                                                      top_k=k, top_p=p, seed=77, return_samples=True)
        m = slp.shape[-1]
        assert samples.shape == (B, n, m + 1) and sums.shape == (B, n) and slq.shape == (B, n, m)
        # (a) every step's model log-prob is the teacher-forced forward's log-prob of the sampled token
        ref = _teacher_forced(agent, fs, samples)                                   # (B*n, m, V)
        toks_n = samples.reshape(B * n, m + 1)[:, 1:]
        live = torch.ones_like(toks_n, dtype=torch.bool)
        is_end = toks_n == END
        live[:, 1:] = (is_end.cumsum(1) - is_end.long())[:, 1:] == 0
        lp_ref = ref.gather(-1, toks_n.unsqueeze(-1)).squeeze(-1)
        err = float(((slp.reshape(B * n, m) - lp_ref).abs() * live).max())
        assert err < 1e-3, err
        assert bool((slp.reshape(B * n, m)[~live] == 0).all()) and bool((toks_n[~live] == PAD).all())
        assert torch.allclose(sums.reshape(-1).double(), (slp.reshape(B * n, m).double()).sum(1), atol=1e-4)
        # (b) every token lies in the truncated set of the teacher-forced distribution (up to 2e-3 in log-prob)
        qf = torch.exp((ref.double() - ref.double().amax(-1, keepdim=True)) / T)
        tok_lp = lp_ref.double().unsqueeze(-1)
        above = ref.double() > tok_lp + 2e-3
        assert bool(((above.sum(-1) < k) | ~live).all())
        frac = (qf * above).sum(-1) / qf.sum(-1)
        assert bool(((frac < p + 1e-3) | ~live).all())
        # (c) the re-run path with the same seed: the same tokens up to a row's first low-margin step
        forced = sample_decode(agent, fs, L, START, END, PAD, "audio_video", n=n, temperature=T, top_k=k, top_p=p, seed=77,
                               return_samples=True, incremental=False)[1].reshape(B * n, -1)
        inc = samples.reshape(B * n, -1)
        same_rows = 0
        for r in range(B * n):
            w = min(inc.shape[1], forced.shape[1])
            diff = (inc[r, :w] != forced[r, :w]).nonzero()
            if diff.numel() == 0:
                same_rows += 1
                continue
            s = int(diff[0]) - 1                                                    # the step of the first difference
            u = torch.from_numpy(uniform01(77, [(r << 16) + s])).to(DEV)
            lp_s = ref[r, s].unsqueeze(0).double()
            # at that step the teacher-forced distribution has a boundary within 1e-3: moving the draw or top_p by 1e-3 or
            # the log-probs around the k-th token by 2e-3 changes the pick
            top = torch.sort(lp_s[0], descending=True).values
            near = bool(top[k - 1] - top[k] < 2e-3)
            for du, dp in itertools.product((-1e-3, 0.0, 1e-3), (-1e-3, 0.0, 1e-3)):
                pk, _ = _sample_choose(lp_s, T, k, min(p + dp, 1.0), (u + du).clamp(0, 1 - 1e-9))
                near |= int(pk) != int(inc[r, s + 1]) or int(pk) != int(forced[r, s + 1])
            assert near, (r, s)
        assert same_rows >= (B * n) // 2, same_rows
        # (d) graph and eager decoders give bit-identical samples for the same seed
        if graph:
            SampleDecoder.use_graph = False
            eager = SampleDecoder(agent, B, dec.tv_cap, dec.ta_cap, L, START, END, PAD, DEV, beams=n)
            eager.set_params(T, k, p)
            dec.set_params(T, k, p)
            with torch.no_grad():
                assert eager.graph is None and eager.begin(fs)
                e = eager.run(77)
                assert dec.begin(fs)
                d = dec.run(77)
            assert e[4] == d[4]
            for x, y in zip(e[:4], d[:4]):
                assert torch.equal(x, y)
            SampleDecoder.use_graph = graph
        # (e) through the cached decoder: a second clip batch, then the same seed repeats and a new one does not
        fs2 = _batch(B, 64, 200, V, 9)
        sample_decode(agent, fs2, L, START, END, PAD, "audio_video", n=n, temperature=T, top_k=k, top_p=p, seed=5)
        again = sample_decode(agent, fs, L, START, END, PAD, "audio_video", n=n, temperature=T, top_k=k, top_p=p, seed=77,
                              return_samples=True)
        assert torch.equal(again[1], samples) and torch.equal(again[2], sums)
        fresh = sample_decode(agent, fs, L, START, END, PAD, "audio_video", n=n, temperature=T, top_k=k, top_p=p, seed=78,
                              return_samples=True)
        assert not torch.equal(fresh[1][..., :2], samples[..., :2])
        print(f"sample n={n} graph={graph}: step logp error vs teacher-forced {err:.2e}, rows equal to the re-run "
              f"{same_rows}/{B * n}")
    finally:
        SampleDecoder.use_graph = old


def test_sixteen_samples_per_clip():
    _needs_gpu()
    from bmhrl_amd.decode import SampleDecoder, sample_decode
    V, B, L = 300, 2, 8
    agent = _agent(torch.device(DEV), V)
    fs = _batch(B, 40, 70, V, 2)
    toks, samples, sums, slp, slq = sample_decode(agent, fs, L, START, END, PAD, "audio_video", n=16, top_p=0.95, seed=1,
                                                  return_samples=True)
    assert isinstance(SampleDecoder.for_batch(agent, fs, L, START, END, PAD, 16), SampleDecoder)
    assert samples.shape[:2] == (B, 16) and sums.shape == (B, 16)
    assert bool((slq <= 1e-6).all()) and bool((slp <= 0).all())
    assert len({tuple(r.tolist()) for r in samples[0]}) > 1                # 16 rows of one clip differ
    best = sums.argmax(1)
    for b in range(B):
        row = samples[b, best[b], :toks.shape[1]]
        assert torch.equal(toks[b, :row.shape[0]], row)
    ref = _teacher_forced(agent, fs, samples)
    m = slp.shape[-1]
    t_n = samples.reshape(B * 16, m + 1)[:, 1:]
    is_end = t_n == END
    live = (is_end.cumsum(1) - is_end.long()) == 0
    err = ((slp.reshape(B * 16, m) - ref.gather(-1, t_n.unsqueeze(-1)).squeeze(-1)).abs() * live).max()
    assert float(err) < 1e-3


def test_sample_decoder_drives_predict_1by1():
    _needs_gpu()
    from bmhrl_amd.decode import sample_decoder
    from bmhrl_amd.epoch_loops.validation_loops import predict_1by1
    V, B, L = 120, 3, 8
    agent = _agent(torch.device(DEV), V)
    fs = _batch(B, 40, 70, V, 3)
    itos = [f"w{i}" for i in range(V)]
    itos[START], itos[END], itos[PAD] = "<s>", "</s>", "<blank>"
    ds = SimpleNamespace(start_idx=START, end_idx=END, pad_idx=PAD, train_vocab=SimpleNamespace(itos=itos))
    batch = {"feature_stacks": fs, "video_ids": ["v0", "v1", "v0"], "starts": torch.tensor([0.0, 1.0, 2.0]),
             "ends": torch.tensor([1.0, 2.0, 3.0])}

    class Loader(list):
        dataset = ds
    cfg = SimpleNamespace(max_len=L, modality="audio_video")
    pred = predict_1by1(cfg, agent, Loader([batch]), sample_decoder(n=4, top_p=0.9))
    got = [seg["sentence"] for vid in ("v0", "v1") for seg in pred["results"][vid]]
    assert len(got) == B and all(isinstance(s, str) for s in got)
