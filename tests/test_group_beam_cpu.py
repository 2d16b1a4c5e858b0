"""Diverse (group) beam search, the re-run path (bmhrl_amd.decode.beam_decode with beam_groups > 1 on CPU tensors): rules
G1-G5 of the module's group beam search section pinned on a toy model whose log-probs come from a fixed table indexed by
(sample, previous token, position), against the numpy restatement of tests/group_beam_reference.py and hand-written cases."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from bmhrl_amd import decode
from bmhrl_amd.decode import beam_decode, beam_decoder
from tests import group_beam_reference as ref

START, END, PAD = 2, 3, 1
NEG = float("-inf")


class TableModel:
    """inference(x, trg, masks) -> (rows, L, V) log-probs: table[sample, trg[:, i], i]; the sample id is rgb[:, 0, 0]"""
    training = False

    def __init__(self, n_samples, V, L, seed=0, scale=1.0, table=None):
        g = torch.Generator().manual_seed(seed)
        self.table = torch.log_softmax(scale * torch.randn(n_samples, V, L, V, generator=g), -1) if table is None else table

    def inference(self, x, trg, masks):
        sid = x[0][0][:, 0, 0].long() - 1
        pos = torch.arange(trg.shape[1])
        return self.table[sid.unsqueeze(1), trg, pos.unsqueeze(0)]


def _features(B, T=5):
    rgb = torch.rand(B, T, 6) + 0.5
    rgb[:, :, 0] = torch.arange(1, B + 1, dtype=torch.float32).unsqueeze(1)     # (non-zero: every feature row is valid)
    return {"rgb": rgb, "flow": torch.rand(B, T, 6), "audio": torch.rand(B, T + 2, 4) + 0.5}


def _hand_model(V, rows):
    """one sample, log-probs that depend on the position only: rows[i] = the V values after i tokens (exact in fp32)"""
    table = torch.full((1, V, len(rows), V), NEG)
    for i, r in enumerate(rows):
        table[0, :, i, :] = torch.tensor(r, dtype=torch.float32)
    return TableModel(1, V, len(rows), table=table)


def _run(model, fs, L, K, G, lam, **kw):
    return beam_decode(model, fs, L, START, END, PAD, "audio_video", beam_size=K, beam_groups=G, diversity_penalty=lam,
                       incremental=False, **kw)


@pytest.mark.parametrize("K,G,lam", [(4, 2, 0.5), (6, 3, 0.7), (6, 2, 1e4), (4, 4, 0.25), (8, 2, 0.0)])
def test_rerun_equals_the_restatement_step_by_step(K, G, lam):
    """every step of _group_beam_rerun against tests/group_beam_reference.py on the step's own log-probs: parents, tokens,
    scores (bit for bit) and flags; log-probs on a coarse grid, so exact ties and ties created by the penalty occur"""
    B, V, L = 4, 9, 7
    model = TableModel(B, V, L + 1, seed=K * 10 + G)
    model.table = torch.round(model.table * 4) / 4
    fs = _features(B)
    trace = []
    lam32 = np.float32(lam).item()
    toks, scores, steps = decode._group_beam_rerun(model, fs, L, START, END, PAD, "audio_video", K, G, lam32, trace=trace)
    assert len(trace) == steps and toks.shape == (B, K, steps + 1)
    s0, f0 = ref.initial_state(B, K, G)
    assert np.array_equal(trace[0]["scores"].numpy(), s0) and np.array_equal(trace[0]["finished"].numpy(), f0)
    ended = penalised = 0
    for i, st in enumerate(trace):
        want = ref.group_beam_step(st["logp"].numpy(), st["scores"].numpy(), st["finished"].numpy(), G, lam32, END, PAD)
        plain = ref.group_beam_step(st["logp"].numpy(), st["scores"].numpy(), st["finished"].numpy(), G, 0.0, END, PAD)
        assert np.array_equal(st["new_scores"].numpy().view(np.int32), want[0].view(np.int32)), i
        assert np.array_equal(st["new_finished"].numpy(), want[1]), i
        assert np.array_equal(st["parent"].numpy(), want[2]) and np.array_equal(st["tok"].numpy(), want[3]), i
        assert bool((st["parent"] // (K // G) == torch.arange(K) // (K // G)).all())        # parents stay in their group
        assert torch.equal(st["hist"][..., -1], st["tok"])
        if i + 1 < len(trace):
            assert torch.equal(trace[i + 1]["scores"], st["new_scores"]) and torch.equal(trace[i + 1]["finished"], st["new_finished"])
        ended += int(want[1].sum())
        penalised += int((want[3] != plain[3]).sum())
    assert torch.equal(toks, trace[-1]["hist"]) and torch.equal(scores, trace[-1]["new_scores"])
    assert ended > 0
    assert (penalised > 0) == (lam > 0 and G > 1), penalised


@pytest.mark.parametrize("lam", [0.0, 0.7])
def test_one_group_is_beam_search(lam):
    B, V, L, K = 4, 9, 7, 5
    model = TableModel(B, V, L + 1, seed=3)
    fs = _features(B)
    want = beam_decode(model, fs, L, START, END, PAD, "audio_video", beam_size=K, return_scores=True, return_beams=True,
                       incremental=False)
    got = _run(model, fs, L, K, 1, lam, return_scores=True, return_beams=True)
    assert len(got) == len(want) == 4 and all(torch.equal(a, b) for a, b in zip(got, want))
    # ... and the grouped re-run itself, asked for one group, is beam search too
    a = decode._group_beam_rerun(model, fs, L, START, END, PAD, "audio_video", K, 1, lam)
    b = decode._beam_rerun(model, fs, L, START, END, PAD, "audio_video", K)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2]


def test_no_penalty_makes_every_group_the_small_beam_search():
    """lambda = 0, (K, G) = (6, 3): beam g*2 + j equals beam j of beam_size = 2, tokens and scores bit for bit"""
    B, V, L = 4, 9, 7
    model = TableModel(B, V, L + 1, seed=5)
    fs = _features(B)
    small = decode._beam_rerun(model, fs, L, START, END, PAD, "audio_video", 2)
    big = decode._group_beam_rerun(model, fs, L, START, END, PAD, "audio_video", 6, 3, 0.0)
    assert big[2] == small[2]
    for g in range(3):
        assert torch.equal(big[0][:, 2 * g:2 * g + 2], small[0]) and torch.equal(big[1][:, 2 * g:2 * g + 2], small[1])
    toks, beams, scores, groups = _run(model, fs, L, 6, 3, 0.0, return_beams=True, return_groups=True)
    s_toks, s_beams, s_scores = beam_decode(model, fs, L, START, END, PAD, "audio_video", beam_size=2, return_beams=True,
                                            incremental=False)
    assert torch.equal(toks, s_toks)                      # ties between the groups' copies go to the lower beam index
    assert torch.equal(scores[:, ::3], s_scores) and torch.equal(scores[:, 1::3], s_scores)
    assert torch.equal(groups[:, :3], torch.tensor([[0, 1, 2]] * B))


def test_penalty_changes_the_second_groups_token():
    """V = 6, two groups of one beam, two steps.  Step 1: both groups would take token 4 (-0.25); group 1 pays 0.5 for it
    (-0.75) and takes token 5 (-0.5) instead.  Step 2: group 0 takes 0 (-0.125); group 1 pays 0.5 on 0 (-0.625) and takes 4
    (-0.25).  The returned scores are the unpenalised sums."""
    rows = [[-4.0, -9.0, -9.0, -9.0, -0.25, -0.5],
            [-0.125, -9.0, -9.0, -9.0, -0.25, -3.0]]
    model = _hand_model(6, rows)
    fs = _features(1)
    toks, score, beams, scores, groups = _run(model, fs, 2, 2, 2, 0.5, return_scores=True, return_beams=True, return_groups=True)
    assert beams.tolist() == [[[START, 4, 0], [START, 5, 4]]]
    assert scores.tolist() == [[-0.375, -0.75]]                   # -0.25 - 0.125 and -0.5 - 0.25: no penalty inside
    assert groups.tolist() == [[0, 1]] and toks.tolist() == [[START, 4, 0]] and score.tolist() == [-0.375]
    # without the penalty both groups are the same greedy search
    _, beams0, scores0 = _run(model, fs, 2, 2, 2, 0.0, return_beams=True)
    assert beams0.tolist() == [[[START, 4, 0], [START, 4, 0]]] and scores0.tolist() == [[-0.375, -0.375]]
    # a penalty that only ties: 0.25 makes token 4 (-0.25 - 0.25) equal token 5 (-0.5); the tie goes to the smaller v, token 4
    _, beams1, _ = _run(model, fs, 1, 2, 2, 0.25, return_beams=True)
    assert beams1.tolist() == [[[START, 4], [START, 4]]]


def test_a_token_chosen_by_two_groups_counts_twice():
    """three groups of one beam.  Token 4: -0.25, token 5: -1.0, token 0: -1.5.  lambda = 0.5: group 1 sees 4 at -0.75 and
    still takes it; group 2 sees it at -0.25 - 0.5 * 2 = -1.25 and takes 5 (-1.0).  Counted once, 4 would be -0.75: taken."""
    rows = [[-1.5, -9.0, -9.0, -9.0, -0.25, -1.0]]
    model = _hand_model(6, rows)
    fs = _features(1)
    _, beams, scores, groups = _run(model, fs, 1, 3, 3, 0.5, return_beams=True, return_groups=True)
    by_group = {int(g): (beams[0, i].tolist(), float(scores[0, i])) for i, g in enumerate(groups[0])}
    assert by_group == {0: ([START, 4], -0.25), 1: ([START, 4], -0.25), 2: ([START, 5], -1.0)}
    # the restatement on the same step agrees
    lp = np.tile(np.asarray(rows[0], dtype=np.float32), (1, 3, 1))
    s0, f0 = ref.initial_state(1, 3, 3)
    assert ref.group_beam_step(lp, s0, f0, 3, 0.5, END, PAD)[3].tolist() == [[4, 4, 5]]


def _two_steps(rows):
    trace = []
    decode._group_beam_rerun(_hand_model(6, rows), _features(1), 2, START, END, PAD, "audio_video", 4, 2, 1.0, trace=trace)
    for st in trace:                                      # the restatement agrees on both steps
        got = ref.group_beam_step(st["logp"].numpy(), st["scores"].numpy(), st["finished"].numpy(), 2, 1.0, END, PAD)
        assert got[2].tolist() == st["parent"].tolist() and got[3].tolist() == st["tok"].tolist()
        assert got[0].tolist() == st["new_scores"].tolist()
    return trace


def test_a_finished_beams_pad_is_not_penalised():
    """two groups of two beams, V = 6, PAD = 1, lambda = 1.  Step 1: group 0 takes END (-0.125) and PAD (-0.25; a live beam's
    pad candidate, which counts), group 1 pays 1 on both and takes 4 (-1.0) and END (-0.125 - 1).  Step 2: group 0 keeps its
    finished beam, (0, PAD) at -0.125, and its live beam takes PAD (-0.25): PAD is counted once.  Group 1's finished beam 3
    offers (3, PAD) at -0.125 unpenalised and comes first, before (2, 0) at -1.0625; penalised (-1.125) it would come second."""
    trace = _two_steps([[-5.0, -0.25, -9.0, -0.125, -1.0, -2.0],
                        [-0.0625, 0.0, -9.0, -9.0, -9.0, -9.0]])
    assert trace[0]["tok"].tolist() == [[END, PAD, 4, END]]
    assert trace[0]["new_scores"].tolist() == [[-0.125, -0.25, -1.0, -0.125]]
    assert trace[0]["new_finished"].tolist() == [[True, False, False, True]]
    assert trace[1]["tok"].tolist() == [[PAD, PAD, PAD, 0]]
    assert trace[1]["parent"].tolist() == [[0, 1, 3, 2]]
    assert trace[1]["new_scores"].tolist() == [[-0.125, -0.25, -0.125, -1.0625]]


def test_a_finished_beams_pad_is_not_counted():
    """as above, but group 1 takes 4 (-0.5) and 5 (-0.75) at step 1 and stays live.  Step 2: group 0 chooses (0, PAD) of its
    finished beam and (1, PAD) of its live beam: c(PAD) = 1, not 2.  Group 1 then sees (2, PAD) at -0.5 - 1 = -1.5 and (3, PAD)
    at -0.75 - 1 = -1.75, both before (2, 5) at -2.75; with c = 2 they would be -2.5 and -2.75, and (2, 5) would win the tie
    for the second slot by its smaller index."""
    trace = _two_steps([[-5.0, -0.25, -9.0, -0.125, -0.5, -0.75],
                        [-9.0, 0.0, -9.0, -9.0, -9.0, -2.25]])
    assert trace[0]["tok"].tolist() == [[END, PAD, 4, 5]]
    assert trace[0]["new_scores"].tolist() == [[-0.125, -0.25, -0.5, -0.75]]
    assert trace[1]["tok"].tolist() == [[PAD, PAD, PAD, PAD]]
    assert trace[1]["parent"].tolist() == [[0, 1, 2, 3]]
    assert trace[1]["new_scores"].tolist() == [[-0.125, -0.25, -0.5, -0.75]]          # s, not a


def test_return_groups_layout():
    B, V, L, K, G = 3, 9, 6, 4, 2
    model = TableModel(B, V, L + 1, seed=8)
    fs = _features(B)
    base = _run(model, fs, L, K, G, 0.5, return_scores=True, return_beams=True)
    got = _run(model, fs, L, K, G, 0.5, return_scores=True, return_beams=True, return_groups=True)
    assert len(base) == 4 and len(got) == 5 and all(torch.equal(a, b) for a, b in zip(base, got[:4]))
    groups = got[4]
    assert groups.shape == (B, K) and groups.dtype == torch.int64
    raw = decode._group_beam_rerun(model, fs, L, START, END, PAD, "audio_video", K, G, 0.5)
    for b in range(B):
        assert sorted(groups[b].tolist()) == [0, 0, 1, 1]
        for i in range(K):                                 # hypothesis i of the result is a beam of the group it names
            rows = [k for k in range(K) if k // 2 == int(groups[b, i])]
            assert any(raw[0][b, k, :got[2].shape[-1]].tolist() == got[2][b, i].tolist() and raw[1][b, k] == got[3][b, i]
                       for k in rows)
    cons = _run(model, fs, L, K, G, 0.5, return_scores=True, return_beams=True, return_groups=True, select="consensus")
    assert len(cons) == 6 and torch.equal(cons[4], groups) and cons[5].dtype == torch.float64 and cons[5].shape == (B, K)
    assert torch.equal(cons[2], got[2]) and torch.equal(cons[3], got[3])
    cons_plain = _run(model, fs, L, K, G, 0.5, return_scores=True, return_beams=True, select="consensus")
    assert len(cons_plain) == 5 and torch.equal(cons_plain[4], cons[5])
    one = _run(model, fs, L, K, 1, 0.5, return_beams=True, return_groups=True)
    assert len(one) == 4 and not one[3].any()


def test_invalid_arguments_are_refused():
    model = TableModel(1, 6, 4)
    fs = _features(1)
    bad = [dict(beam_groups=0), dict(beam_groups=-2), dict(beam_groups=1.5), dict(beam_groups="2"), dict(beam_groups=True),
           dict(beam_groups=3), dict(beam_groups=8), dict(diversity_penalty=-0.1), dict(diversity_penalty=math.inf),
           dict(diversity_penalty=math.nan), dict(diversity_penalty=1e39), dict(beam_groups=2, diversity_penalty=-1.0)]
    for kw in bad:
        for incremental in (None, False):
            with pytest.raises(ValueError):
                beam_decode(model, fs, 3, START, END, PAD, "audio_video", beam_size=4, incremental=incremental, **kw)
        with pytest.raises(ValueError):
            beam_decoder(4, **kw)
    for kw in (dict(return_groups=True), dict(return_groups=True, return_scores=True), dict(return_groups=True, beam_groups=2)):
        with pytest.raises(ValueError):
            beam_decode(model, fs, 3, START, END, PAD, "audio_video", beam_size=4, **kw)
    beam_decode(model, fs, 3, START, END, PAD, "audio_video", beam_size=4, beam_groups=2.0, diversity_penalty=0)    # whole: fine


def test_grouped_decoder_drives_predict_1by1():
    from bmhrl_amd.epoch_loops.captioning_bmrl_loops import beam_decoder as exported
    from bmhrl_amd.epoch_loops.validation_loops import predict_1by1, tokens_to_sentences
    assert exported is beam_decoder
    B, V, L = 3, 10, 6
    model = TableModel(B, V, L + 1, seed=4)
    fs = _features(B)
    itos = [f"w{i}" for i in range(V)]
    itos[START], itos[END], itos[PAD] = "<s>", "</s>", "<blank>"
    ds = SimpleNamespace(start_idx=START, end_idx=END, pad_idx=PAD, train_vocab=SimpleNamespace(itos=itos))
    batch = {"feature_stacks": fs, "video_ids": ["v0", "v1", "v0"], "starts": torch.tensor([0.0, 1.0, 2.0]),
             "ends": torch.tensor([1.0, 2.0, 3.0])}

    class Loader(list):
        dataset = ds
    cfg = SimpleNamespace(max_len=L, modality="audio_video")
    pred = predict_1by1(cfg, model, Loader([batch]), beam_decoder(4, beam_groups=2, diversity_penalty=0.5, select="consensus"))
    want = tokens_to_sentences(_run(model, fs, L, 4, 2, 0.5, select="consensus").numpy(), itos)
    got = [seg["sentence"] for vid in ("v0", "v1") for seg in pred["results"][vid]]
    assert sorted(got) == sorted(want) and len(got) == B


def test_default_keywords_change_nothing():
    B, V, L, K = 3, 9, 6, 4
    model = TableModel(B, V, L + 1, seed=9)
    fs = _features(B)
    for kw in (dict(), dict(return_scores=True, return_beams=True), dict(return_beams=True, select="consensus")):
        want = beam_decode(model, fs, L, START, END, PAD, "audio_video", beam_size=K, **kw)
        got = beam_decode(model, fs, L, START, END, PAD, "audio_video", beam_size=K, beam_groups=1, diversity_penalty=0.0,
                          return_groups=False, **kw)
        want, got = (want, got) if isinstance(want, tuple) else ((want,), (got,))
        assert len(want) == len(got) and all(torch.equal(a, b) for a, b in zip(want, got))
    d0, d1 = beam_decoder(K), beam_decoder(K, beam_groups=1, diversity_penalty=0.0)
    assert torch.equal(d0(model, fs, L, START, END, PAD, "audio_video"), d1(model, fs, L, START, END, PAD, "audio_video"))
