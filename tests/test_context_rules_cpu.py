"""Paragraph-aware decoding without a GPU: the re-run path's _apply_context_rules against the numpy
restatement of tests/context_rules_reference.py over the whole case table, the refusals of rule C5, the header constant, and
predict.caption_segments(paragraph=True) on CPU VideoFeatures -- wave order, contexts, result order -- with stub decoders and
with the real re-run decoders over a stub model whose log-probs follow a fixed bigram table."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import context_rules_reference as ref
from tests import segment_crop_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD, START, END = C.PAD_IDX, 2, 3
AV = "audio_video"


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def test_apply_context_rules_equals_the_restatement():
    from bmhrl_amd.decode import _apply_context_rules, _f32
    cases = ref.case_table()
    assert len(cases) > 200
    for i, c in enumerate(cases):
        lp = ref.case_logp(c, i)
        got = _apply_context_rules(torch.from_numpy(lp.copy()), torch.from_numpy(c["hist"]), c["t"],
                                   (c["n"], c["m"], _f32(c["theta"])), c["end"], c["pad"], torch.from_numpy(c["ctx"]), c["rpc"],
                                   (c["n_c"], _f32(c["theta_c"])))
        assert got.dtype == torch.float32
        assert np.array_equal(_bits(got.numpy()), _bits(ref.want(c, lp))), c["name"]


def test_the_case_table_holds_what_it_promises():
    """the restatement itself on hand-checked cases, and the table's coverage"""
    V = 12
    lp = np.full((1, V), -1.0, dtype=np.float32)
    hist = np.array([[START, 7, 3, 4]])
    # tail (3, 4) at t = 3: followers 8 and 9 banned, the window over the separator and the one with a gap are not
    ctx = np.array([[3, 4, 8, PAD, 3, 4, 9, 3, PAD, 4, 10, 3, 4, -1, 4, 11]])
    out = ref.apply_context_rules(lp, hist, 3, 0, 0, 1.0, END, PAD, ctx, 1, 3, 1.0)
    assert np.isinf(out[0]).nonzero()[0].tolist() == [8, 9]
    # the start token is never part of the tail: at t = 1 the tail of n_c = 3 would need s[0]
    assert not np.isinf(ref.apply_context_rules(lp, np.array([[3, 4]]), 1, 0, 0, 1.0, END, PAD, ctx, 1, 3, 1.0)).any()
    assert np.isinf(ref.apply_context_rules(lp, np.array([[0, 3, 4]]), 2, 0, 0, 1.0, END, PAD, ctx, 1, 3, 1.0)[0, 8])
    # n_c = 1: every word of the context; C1 once per id, after rule 1's multiply
    out = ref.apply_context_rules(lp, hist, 3, 0, 0, 1.0, END, PAD, ctx, 1, 1, 1.0)
    assert np.isinf(out[0]).nonzero()[0].tolist() == [3, 4, 8, 9, 10, 11]
    out = ref.apply_context_rules(lp, hist, 3, 0, 0, 1.5, END, PAD, ctx, 1, 0, 3.0)
    assert out[0].tolist() == [-1, -1, -1.5, -4.5, -4.5, -1, -1, -1.5, -3, -3, -3, -3]
    names = " | ".join(c["name"] for c in ref.case_table())
    for what in ("C=1024", "C=63", "C=64", "C=65", "rpc=3", "gap -1 at position 0", "gap 1 at position 2", "j = C - n_c",
                 "several followers", "22 times", "gaps only", "2^40", "V = 65", "V = 10172"):
        assert what in names, what
    assert ref.paragraphs_share_ngram([[1, 2, 3], [4, 1, 2, 3]], 3) and not ref.paragraphs_share_ngram([[1, 2, 3, 1, 2, 3], [3, 2, 1, 3]], 3)


def test_max_ctx_is_the_headers():
    from bmhrl_amd import ops, predict
    with open(os.path.join(ROOT, "include", "bmhrl_hip.h")) as f:
        text = f.read()
    assert re.findall(r"^#define\s+BMHRL_LOGIT_RULES_MAX_CTX\s+(\d+)\s*$", text, re.M) == [str(ops.LOGIT_RULES_MAX_CTX)]
    assert re.findall(r"^#define\s+BMHRL_LOGIT_RULES_CTX_MAX_V\s+(\d+)\s*$", text, re.M) == [str(ops.LOGIT_RULES_CTX_MAX_V)]
    assert re.findall(r"^#define\s+BMHRL_PARAGRAPH_MAX_TOKENS\s+(\d+)\s*$", text, re.M) == [str(ops.LOGIT_RULES_MAX_CTX)]
    assert ops.LOGIT_RULES_MAX_CTX == predict.PARAGRAPH_MAX_CONTEXT == 1024


# ------------------------------------------------------------------------------------------------ a model with `inference`
VOC = 8
ITOS = ["<unk>", "<blank>", "<s>", "</s>", "a", "man", "runs", "fast"]
# the best and second-best next token: <s> -> a; a -> man; man -> runs; runs -> fast, else a; fast -> </s>, else a
NEXT = {START: (4, 5), 4: (5, 6), 5: (6, 7), 6: (7, 4), 7: (END, 4), END: (PAD, 4), PAD: (PAD, 4), 0: (4, 5)}


class BigramModel:
    """log-probs that depend on the last token only: a cycle a man runs fast [a man runs fast ...] that ends after `fast`
    once the minimum length allows it"""
    training = False

    def __init__(self):
        table = torch.full((VOC, VOC), -8.0)
        for a, (best, second) in NEXT.items():
            table[a] -= torch.arange(VOC) * 0.01            # no ties
            table[a, best], table[a, second] = -0.1, -2.0
        self.table = table

    def inference(self, x, trg, masks):
        return self.table[trg]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    vp, ap, arrays = C.write_features(tmp_path_factory.mktemp("features"))
    return SimpleNamespace(vp=vp, ap=ap, arrays=arrays)


def _features(files):
    from bmhrl_amd.predict import VideoFeatures
    cfg = SimpleNamespace(video_features_path=files.vp, audio_features_path=files.ap)
    return VideoFeatures.from_npy(cfg, C.VIDEO_IDS, C.DURATIONS, C.PAD_TO, C.PAD_IDX, "cpu")


def _cfg(max_len=10, batch=2):
    return SimpleNamespace(max_len=max_len, modality=AV, inference_batch_size=batch)


DS = SimpleNamespace(start_idx=START, end_idx=END, pad_idx=PAD, train_vocab=SimpleNamespace(itos=ITOS))


def _words(results):
    return [[cap["sentence"].lower().split() for cap in caps] for caps in results]


def test_c5_refusals():
    from bmhrl_amd.decode import (_context_args, beam_decode, beam_decoder, greedy_decode, greedy_decoder, sample_decode,
                                  sample_decoder)
    model = BigramModel()
    fs = {"rgb": torch.ones(2, 3, 4), "flow": torch.ones(2, 3, 4), "audio": torch.ones(2, 3, 4)}
    args = (model, fs, 6, START, END, PAD, AV)
    bad_rules = [dict(context_ngram=-1), dict(context_ngram=1.5), dict(context_ngram="x"), dict(context_ngram=True),
                 dict(context_penalty=0.0), dict(context_penalty=-1.0), dict(context_penalty=float("nan")),
                 dict(context_penalty=float("inf")), dict(context_penalty=1e39), dict(context_penalty=1e-60)]
    bad_context = [dict(context=torch.zeros(2, 1025, dtype=torch.int64)), dict(context=torch.zeros(3, 4, dtype=torch.int64)),
                   dict(context=[[4, 5]]), dict(context=[[4], [5], [6]]), dict(context=[[4] * 1025, [5]]),
                   dict(context=torch.zeros(2, 4)), dict(context=torch.zeros(2, dtype=torch.int64))]
    for decode in (greedy_decode, lambda *a, **k: beam_decode(*a, beam_size=2, **k),
                   lambda *a, **k: beam_decode(*a, beam_size=2, beam_groups=2, **k), lambda *a, **k: sample_decode(*a, n=2, seed=1, **k)):
        for kw in bad_rules:
            with pytest.raises(ValueError):
                decode(*args, context=[[4], [5]], **kw)
            with pytest.raises(ValueError):
                decode(*args, **kw)                             # refused without a context too
        for kw in bad_context:
            with pytest.raises(ValueError):
                decode(*args, context_ngram=2, **kw)
            with pytest.raises(ValueError):
                decode(*args, **kw)                             # and with the rules at their defaults
        # the limits themselves pass: 1024 columns, a list of B lists, empty lists
        decode(*args, context=torch.full((2, 1024), 4, dtype=torch.int64), context_ngram=2)
        decode(*args, context=[[], []], context_ngram=2, context_penalty=1.5)
    for factory in (greedy_decoder, beam_decoder, sample_decoder):
        for kw in bad_rules:
            with pytest.raises(ValueError):
                factory(**kw)
    assert _context_args(0, 1.0) is None and _context_args(2, 1.0) == (2, 1.0) and _context_args(0, 1.3)[1] == float(np.float32(1.3))


def test_rerun_decoders_obey_the_context_on_the_cpu():
    """greedy, beam (plain and grouped) and sample over a model with `inference` only: no returned hypothesis shares a 3-gram
    with its context, the off states equal the calls without the keywords, and a penalty alone changes the first word"""
    from bmhrl_amd.decode import beam_decode, greedy_decode, sample_decode
    model = BigramModel()
    fs = {"rgb": torch.ones(2, 3, 4), "flow": torch.ones(2, 3, 4), "audio": torch.ones(2, 3, 4)}
    args = (model, fs, 10, START, END, PAD, AV)
    free = greedy_decode(*args, min_len=6)
    assert free.tolist() == [[START, 4, 5, 6, 7, 4, 5, 6, 7, END]] * 2
    ctx = [[4, 5, 6, 7, 4, 5, 6, 7], [9, 9, PAD, 4, 5, PAD, 6, 7]]                # clip 1: no 3-gram inside a sentence
    kw = dict(min_len=6, context=ctx, context_ngram=3)
    got = greedy_decode(*args, **kw)
    # clip 0: `runs` after `a man` is banned (-> fast), the end is banned before 6 tokens (-> a), `man` after `fast a` is
    # banned (-> runs), `a` after `runs fast` is banned and the end is free by then
    assert got[0].tolist() == [START, 4, 5, 7, 4, 6, 7, END, PAD, PAD]
    assert got[1].tolist() == free[1].tolist()                                  # gaps: nothing to ban for clip 1
    decodes = {"greedy": lambda **k: greedy_decode(*args, **k),
               "beam": lambda **k: beam_decode(*args, beam_size=2, **k),
               "group beam": lambda **k: beam_decode(*args, beam_size=2, beam_groups=2, diversity_penalty=0.5, **k),
               "sample": lambda **k: sample_decode(*args, n=2, seed=5, **k)}
    for name, decode in decodes.items():
        out = decode(**kw)
        for row, c in zip(out.tolist(), ctx):
            assert not ref.shares_ngram(row[1:], c, 3, VOC, PAD), (name, row)
        assert ref.shares_ngram(decode(min_len=6)[0].tolist()[1:], ctx[0], 3, VOC, PAD), name
        plain = decode(min_len=6)
        for off in (dict(context=None, context_ngram=3, context_penalty=1.3), dict(context=ctx, context_ngram=0, context_penalty=1.0)):
            assert torch.equal(decode(min_len=6, **off), plain), (name, off)
    # C1 alone: `a` (-0.1) times 30 falls below `man` (-2.0) as the first word
    pen = greedy_decode(*args, context=[[4], [PAD]], context_penalty=30.0)
    assert pen[0, 1].item() == 5 and pen[1, 1].item() == 4


# --------------------------------------------------------------------------------------------------------- paragraph mode
SEGS = [[(3.0, 5.0), (0.0, 2.0), (3.0, 4.0)], [(10.0, 20.0), (1.0, 2.0)]]
LONG_ITOS = ITOS + [f"w{i}" for i in range(40)]
LONG_DS = SimpleNamespace(start_idx=START, end_idx=END, pad_idx=PAD, train_vocab=SimpleNamespace(itos=LONG_ITOS))


def _stub(calls):
    """call k, row i -> <s> w(k) w(10 + i) <blank> runs </s> fast <blank>: the caption is [8 + k, 18 + i, 6]"""
    def decoder(model, fs, max_len, start, end, pad, modality, context=None):
        k = len(calls)
        calls.append(dict(context=None if context is None else context.clone(), rows=fs["rgb"].shape[0], fs=fs,
                          args=(max_len, start, end, pad, modality)))
        return torch.tensor([[START, 8 + k, 18 + i, PAD, 6, END, 7, PAD] for i in range(fs["rgb"].shape[0])])
    return decoder


def _cap(k, i):
    return [8 + k, 18 + i, 6]


def _sentence(k, i):
    return f"W{k} w{10 + i} <blank> runs"          # (tokens_to_sentences keeps a pad before the end, as it always has)


def test_paragraph_mode_waves_contexts_and_order(files):
    from bmhrl_amd.predict import caption_segments
    feats = _features(files)
    calls = []
    got = caption_segments(_cfg(), "agent", feats, SEGS, _stub(calls), LONG_DS, batch_size=2, paragraph=True)
    # time order: v_a (0,2) (3,4) (3,5), v_b (1,2) (10,20); wave w = the w-th of each video, videos in index order
    assert [c["rows"] for c in calls] == [2, 2, 1]
    assert all(c["args"] == (10, START, END, PAD, AV) for c in calls)
    want = [[{"sentence": _sentence(2, 0), "timestamp": [3.0, 5.0]}, {"sentence": _sentence(0, 0), "timestamp": [0.0, 2.0]},
             {"sentence": _sentence(1, 0), "timestamp": [3.0, 4.0]}],
            [{"sentence": _sentence(1, 1), "timestamp": [10.0, 20.0]}, {"sentence": _sentence(0, 1), "timestamp": [1.0, 2.0]}]]
    assert got == want                                                          # in the GIVEN order
    assert [c["context"].dtype for c in calls] == [torch.int64] * 3
    assert calls[0]["context"].tolist() == [[PAD], [PAD]]                       # nothing said yet
    assert calls[1]["context"].tolist() == [_cap(0, 0), _cap(0, 1)]             # end and pads stripped, no start token
    assert calls[2]["context"].tolist() == [_cap(0, 0) + [PAD] + _cap(1, 0)]    # oldest first, one pad between sentences
    # the clips are the crops of those segments
    one = feats.crop([0, 1], [(3.0, 4.0), (10.0, 20.0)], AV)
    assert all(torch.equal(calls[1]["fs"][k], one[k]) for k in one)
    # batch_size = 1: one call per clip, wave by wave; context_sentences = 1 keeps the last caption only
    calls = []
    got1 = caption_segments(_cfg(), "agent", feats, SEGS, _stub(calls), LONG_DS, batch_size=1, paragraph=True, context_sentences=1)
    assert len(calls) == 5 and [c["rows"] for c in calls] == [1] * 5
    assert [c["context"].tolist() for c in calls] == [[[PAD]], [[PAD]], [_cap(0, 0)], [_cap(1, 0)], [_cap(2, 0)]]
    assert [[cap["timestamp"] for cap in caps] for caps in got1] == [[list(s) for s in segs] for segs in SEGS]
    assert got1[0][0]["sentence"] == _sentence(4, 0) and got1[1][0]["sentence"] == _sentence(3, 0)
    calls = []
    caption_segments(_cfg(), "agent", feats, SEGS, _stub(calls), LONG_DS, batch_size=8, paragraph=True, context_sentences=0)
    assert [c["context"].tolist() for c in calls] == [[[PAD]] * 2, [[PAD]] * 2, [[PAD]]]
    # filled chunks: the short chunk is decoded at the full batch size and the extra rows are thrown away
    calls = []
    filled = caption_segments(_cfg(), "agent", feats, SEGS, _stub(calls), LONG_DS, batch_size=2, paragraph=True, fill_chunks=True)
    assert [c["rows"] for c in calls] == [2, 2, 2] and filled == want
    assert calls[2]["context"].tolist() == [_cap(0, 0) + [PAD] + _cap(1, 0)] * 2
    # videos without segments, and none at all
    calls = []
    assert caption_segments(_cfg(), "agent", feats, [[], [(1.0, 2.0)]], _stub(calls), LONG_DS, paragraph=True) == \
        [[], [{"sentence": _sentence(0, 0), "timestamp": [1.0, 2.0]}]]
    assert caption_segments(_cfg(), "agent", feats, [[], []], _stub(calls), LONG_DS, paragraph=True) == [[], []] and len(calls) == 1
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError):
            caption_segments(_cfg(), "agent", feats, SEGS, _stub(calls), LONG_DS, paragraph=True, context_sentences=bad)
    with pytest.raises(ValueError):
        caption_segments(_cfg(), "agent", feats, SEGS[:1], _stub(calls), LONG_DS, paragraph=True)


def test_paragraph_mode_off_is_the_old_call(files):
    from bmhrl_amd.predict import VideoCaptioner, caption_segments
    feats = _features(files)
    calls = []

    def old(model, fs, max_len, start, end, pad, modality):                   # no `context` keyword: a call with one fails
        calls.append(fs["rgb"].shape[0])
        return torch.tensor([[START, 4, 5, END]] * fs["rgb"].shape[0])
    got = caption_segments(_cfg(), "agent", feats, SEGS, old, DS, batch_size=2)
    assert calls == [2, 2, 1] and [[c["timestamp"] for c in caps] for caps in got] == [[list(s) for s in segs] for segs in SEGS]
    assert got == caption_segments(_cfg(), "agent", feats, SEGS, old, DS, batch_size=2, paragraph=False, context_sentences=3)
    with pytest.raises(TypeError):
        caption_segments(_cfg(), "agent", feats, SEGS, old, DS, batch_size=2, paragraph=True)
    # VideoCaptioner hands both keywords on
    props = [[{"timestamp": list(s), "proposal_score": 0.5} for s in segs] for segs in SEGS]
    log = []
    cap = VideoCaptioner(_cfg(), None, "agent", LONG_DS, _stub(log), paragraph=True, context_sentences=1)
    out = cap.caption(feats, props, batch_size=2)
    assert log[2]["context"].tolist() == [_cap(1, 0)] and out[0][0]["proposal_score"] == 0.5
    log = []
    VideoCaptioner(_cfg(), None, "agent", LONG_DS, _stub(log)).caption(feats, props, batch_size=2)
    assert all(c["context"] is None for c in log) and [c["rows"] for c in log] == [2, 2, 1]


def test_paragraph_context_is_cut_at_sentence_boundaries(files):
    from bmhrl_amd.predict import caption_segments, caption_tokens, paragraph_context
    feats = _features(files)
    calls = []

    def long(model, fs, max_len, start, end, pad, modality, context=None):
        k = len(calls)
        calls.append(context.clone())
        return torch.tensor([[START] + [8 + k] * 399])                         # no end token: 399 words
    segs = [[(0.0, 1.0), (1.0, 2.0), (2.0, 3.0), (3.0, 4.0), (4.0, 5.0)], []]
    caption_segments(_cfg(), "agent", feats, segs, long, LONG_DS, batch_size=1, paragraph=True)
    s = [[8 + k] * 399 for k in range(5)]
    assert [c.shape for c in calls] == [(1, 1), (1, 399), (1, 799), (1, 799), (1, 799)]
    assert calls[2].tolist() == [s[0] + [PAD] + s[1]]
    assert calls[3].tolist() == [s[1] + [PAD] + s[2]] and calls[4].tolist() == [s[2] + [PAD] + s[3]]   # oldest dropped, whole
    assert paragraph_context([[4] * 1024], PAD) == [4] * 1024 and paragraph_context([[4] * 1025], PAD) == []
    assert paragraph_context([[4] * 511, [5] * 512], PAD) == [4] * 511 + [PAD] + [5] * 512
    assert paragraph_context([[4] * 512, [5] * 512], PAD) == [5] * 512
    assert paragraph_context([[4], [], [5]], PAD) == [4, PAD, PAD, 5] and paragraph_context([[4], [5], [6]], PAD, 2) == [5, PAD, 6]
    assert paragraph_context([[4], [5]], PAD, 5) == [4, PAD, 5]
    assert caption_tokens([START, 4, PAD, 5, END, 6, END], END, PAD) == [4, 5] and caption_tokens([START, END], END, PAD) == []
    assert caption_tokens([START, 4, 5], -1, PAD) == [4, 5]


def test_identical_segments_repeat_unless_the_context_bans_it(files):
    """two identical segments of one video: the same sentence twice -- and under context_ngram = 4 in paragraph mode no 4-gram
    of the first in the second"""
    from bmhrl_amd.decode import beam_decoder, greedy_decoder
    from bmhrl_amd.predict import caption_segments
    feats = _features(files)
    model = BigramModel()
    segs = [[(1.0, 4.0), (1.0, 4.0)], []]
    plain = caption_segments(_cfg(), model, feats, segs, greedy_decoder(min_len=6), DS)
    assert plain[0][0]["sentence"] == plain[0][1]["sentence"] == "A man runs fast a man runs fast"
    assert ref.paragraphs_share_ngram(_words(plain)[0], 4)
    for decoder in (greedy_decoder(min_len=6, context_ngram=4), beam_decoder(2, min_len=6, context_ngram=4)):
        # without paragraph mode the decoder gets no context and repeats itself; with it, it cannot
        assert ref.paragraphs_share_ngram(_words(caption_segments(_cfg(), model, feats, segs, decoder, DS))[0], 4)
        para = caption_segments(_cfg(), model, feats, segs, decoder, DS, paragraph=True)
        words = _words(para)[0]
        assert len(words[0]) >= 6 and len(words[1]) >= 6 and not ref.paragraphs_share_ngram(words, 4), words
    assert para[0][0]["timestamp"] == [1.0, 4.0]
