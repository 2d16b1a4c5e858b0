"""Beam-search decoding, the re-run path (bmhrl_amd.decode.beam_decode with incremental=False; on CPU tensors the only path):
the rules of the module's beam-search section pinned on a toy model whose log-probs come from a fixed table indexed by
(sample, previous token, position)."""
import itertools
from types import SimpleNamespace

import pytest
import torch

from bmhrl_amd.decode import beam_decode, beam_decoder, greedy_decode

START, END, PAD = 2, 3, 1


class TableModel:
    """inference(x, trg, masks) -> (rows, L, V) log-probs: table[sample, trg[:, i], i]; the sample id is rgb[:, 0, 0]"""
    training = False

    def __init__(self, n_samples, V, L, seed=0, scale=1.0):
        g = torch.Generator().manual_seed(seed)
        self.table = torch.log_softmax(scale * torch.randn(n_samples, V, L, V, generator=g), -1)

    def inference(self, x, trg, masks):
        sid = x[0][0][:, 0, 0].long() - 1
        assert masks["C_mask"].shape == (trg.shape[0], trg.shape[1], trg.shape[1])
        pos = torch.arange(trg.shape[1])
        return self.table[sid.unsqueeze(1), trg, pos.unsqueeze(0)]


def _features(B, T=5):
    rgb = torch.rand(B, T, 6) + 0.5
    rgb[:, :, 0] = torch.arange(1, B + 1, dtype=torch.float32).unsqueeze(1)     # (non-zero: every feature row is valid)
    return {"rgb": rgb, "flow": torch.rand(B, T, 6), "audio": torch.rand(B, T + 2, 4) + 0.5}


def _pad_after_end(toks):
    """greedy tokens with pad_idx after each sample's first END (the beam result's rule 6)"""
    out = toks.clone()
    is_end = out[:, 1:] == END
    after = (is_end.cumsum(1) - is_end.long()) > 0
    out[:, 1:][after] = PAD
    return out


def test_beam_one_is_greedy_with_pad_after_end():
    B, V, L = 6, 12, 9
    model = TableModel(B, V, L + 1, seed=1)
    fs = _features(B)
    greedy = greedy_decode(model, fs, L, START, END, PAD, "audio_video", memoise=False)
    assert (greedy[:, 1:] == END).any()                 # the end rule is exercised
    beam = beam_decode(model, fs, L, START, END, PAD, "audio_video", beam_size=1, incremental=False)
    assert beam.dtype == torch.int64
    assert torch.equal(beam, _pad_after_end(greedy))
    never = beam_decode(model, fs, L, START, -1, PAD, "audio_video", beam_size=1, incremental=False)
    assert torch.equal(never, greedy_decode(model, fs, L, START, -1, PAD, "audio_video", memoise=False))


@pytest.mark.parametrize("length_penalty", [0.0, 1.0])
def test_full_width_beam_is_exhaustive(length_penalty):
    """V = 4, max_len = 2, K = 16 keeps every hypothesis (4 after the first step, 3 * 4 + 1 = 13 after the second): the
    best one is the arg-max over all token sequences under rules 1-5, with the same fp32 score"""
    B, V, L = 5, 4, 2
    model = TableModel(B, V, L + 1, seed=2, scale=2.0)
    fs = _features(B)
    toks, score, beams, beam_scores = beam_decode(model, fs, L, START, END, PAD, "audio_video", beam_size=16,
                                                  length_penalty=length_penalty, return_scores=True, return_beams=True,
                                                  incremental=False)
    zero = torch.zeros((), dtype=torch.float32)
    longest = 0
    for b in range(B):
        hyps = []
        for v0, v1 in itertools.product(range(V), range(V)):
            s0 = zero + model.table[b, START, 0, v0]
            if v0 == END:
                if v1 == 0:                               # the sequence ends after one token
                    hyps.append(((v0,), s0, 1))
                continue
            hyps.append(((v0, v1), s0 + model.table[b, v0, 1, v1], 2))
        assert len(hyps) == 13
        final = lambda h: float(h[1] / ((5.0 + h[2]) / 6.0) ** length_penalty)
        best = max(hyps, key=final)
        longest = max(longest, len(best[0]))
        got = toks[b, 1:].tolist()
        assert got[:len(best[0])] == list(best[0]) and all(t == PAD for t in got[len(best[0]):]), (b, got, best)
        assert torch.equal(score[b], best[1])
        real = beam_scores[b] > float("-inf")
        assert int(real.sum()) == len(hyps)                # every hypothesis survived, the dead beams rank last
        assert sorted(float(h[1]) for h in hyps) == sorted(beam_scores[b][real].tolist())
    assert toks.shape == (B, longest + 1)


def test_return_beams_sorted_with_pad_after_end():
    B, V, L, K = 4, 9, 7, 5
    model = TableModel(B, V, L + 1, seed=3)
    fs = _features(B)
    toks, beams, scores = beam_decode(model, fs, L, START, END, PAD, "audio_video", beam_size=K, return_beams=True,
                                      incremental=False)
    assert beams.shape[:2] == (B, K) and scores.shape == (B, K) and scores.dtype == torch.float32
    assert bool((scores[:, :-1] >= scores[:, 1:]).all())            # length_penalty 0: raw scores, best first
    assert torch.equal(beams[:, 0, :toks.shape[1]], toks)
    assert bool((beams[:, :, 0] == START).all())
    ended = 0
    for b, k in itertools.product(range(B), range(K)):
        row = beams[b, k, 1:].tolist()
        if END in row:
            ended += 1
            assert all(t == PAD for t in row[row.index(END) + 1:])
    assert ended > 0
    # the scores are the sums of the chosen tokens' log-probs (stop at the end token)
    for b, k in itertools.product(range(B), range(K)):
        row = beams[b, k].tolist()
        s = torch.zeros((), dtype=torch.float32)
        for i in range(1, len(row)):
            s = s + model.table[b, row[i - 1], i - 1, row[i]]
            if row[i] == END:
                break
        assert torch.equal(s, scores[b, k])


def test_length_penalty_ranks_by_normalised_score():
    """the search is the same for every length_penalty; the ranking of rule 5 divides by ((5 + n_k) / 6) ** length_penalty"""
    B, V, L, K = 3, 8, 6, 6
    model = TableModel(B, V, L + 1, seed=5)
    fs = _features(B)
    _, raw = beam_decode(model, fs, L, START, END, PAD, "audio_video", beam_size=K, length_penalty=0.0, incremental=False,
                         return_scores=True)
    _, beams, scores = beam_decode(model, fs, L, START, END, PAD, "audio_video", beam_size=K, length_penalty=2.0,
                                   return_beams=True, incremental=False)
    assert torch.equal(raw, scores.max(1).values)       # the same search: raw best is among the beams
    is_end = beams[..., 1:] == END
    n = torch.where(is_end.any(-1), (is_end.cumsum(-1) == 0).sum(-1) + 1, torch.full(is_end.shape[:2], beams.shape[-1] - 1))
    final = scores / ((5.0 + n.float()) / 6.0) ** 2.0
    assert bool((final[:, :-1] >= final[:, 1:]).all())


def test_beam_decoder_drives_predict_1by1():
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
    pred = predict_1by1(cfg, model, Loader([batch]), beam_decoder(2))
    want = tokens_to_sentences(beam_decode(model, fs, L, START, END, PAD, "audio_video", beam_size=2).numpy(), itos)
    got = [seg["sentence"] for vid in ("v0", "v1") for seg in pred["results"][vid]]
    assert sorted(got) == sorted(want) and len(got) == B
    assert [s["timestamp"] for s in pred["results"]["v0"]] == [[0.0, 1.0], [2.0, 3.0]]


def test_beam_size_below_one_is_refused():
    model = TableModel(1, 5, 4)
    fs = _features(1)
    with pytest.raises(ValueError):
        beam_decode(model, fs, 3, START, END, PAD, "audio_video", beam_size=0)
    with pytest.raises(ValueError):
        beam_decoder(0)
