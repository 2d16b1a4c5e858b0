"""Paragraph evaluation on the GPU: csrc/paragraph.hip through ops.ngram_stats against the Counter
restatement (tests/paragraph_reference.py) -- integers, compared for equality -- and the evaluator's Para_* keys against
the restatement of P1-P8: integers exact, the fp64 keys within 1e-12 relative, the bound DESIGN.md sections 13 / 24 hold
caption_eval and METEOR to (the means run in the restatement's order)."""
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import paragraph_reference as pr
from tests.meteor_reference import DictStemmer, dict_synonyms
from tests.test_loops_gpu import setup  # noqa: F401  (the synthetic loader and agent of the loop tests)
from tests.test_paragraph_cpu import job  # noqa: F401  (two invented ground-truth files and a submission)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
RTOL = 1e-12
I32 = dict(dtype=torch.int32, device=DEV)
PARA_KEYS = ["Para_" + m for m in pr.METRICS] + list(pr.STAT_KEYS)


def run(paragraphs):
    """ops.ngram_stats of paragraphs of integer-token sentences -> (G, 4, 5) numpy"""
    from bmhrl_amd import ops
    tok, sent_off, para_off = pr.flatten(paragraphs)
    out = ops.ngram_stats(torch.tensor(tok, **I32), torch.tensor(sent_off, **I32), torch.tensor(para_off, **I32))
    assert out.dtype == torch.int32 and tuple(out.shape) == (len(paragraphs), 4, ops.NGRAM_STATS_INTS)
    return out.cpu().numpy()


def want(paragraphs):
    return np.array([pr.ngram_stats(p) for p in paragraphs], dtype=np.int32).reshape(len(paragraphs), 4, 5)


_IDS = {}


def ids(text):
    return [_IDS.setdefault(w, 100 + len(_IDS)) for w in text.split()]


def test_the_hand_check():
    from bmhrl_amd.evaluate import paragraph_means, paragraph_stats
    got = run([[ids(" ".join(s)) for s in pr.HAND_PARAGRAPH]])
    np.testing.assert_array_equal(got[0], pr.HAND_STATS)
    words = paragraph_stats([pr.HAND_PARAGRAPH], DEV)                     # the same through the public helper, from words
    assert words.dtype == np.int32
    np.testing.assert_array_equal(words[0], pr.HAND_STATS)
    assert paragraph_means(words) == {"Para_RE_4": 0.375, "Para_XRE_4": 0.375, "Para_Div_1": 10 / 17, "Para_Div_2": 9 / 14}
    assert paragraph_stats([], DEV).shape == (0, 4, 5)


def edge_paragraphs():
    rng = np.random.RandomState(3)
    few = lambda n: rng.randint(0, 5, n).tolist()                                                          # noqa: E731
    long = few(1024)
    cases = [
        [],                                                               # 0: no sentence
        [[7]],                                                            # 1: one sentence of one token
        [[1], [1, 2]], [[1, 2], [1, 2, 3]], [[1, 2, 3], [1, 2, 3, 4]],    # 2-4: n - 1 and n tokens, n = 2..4
        [[1, 2, 3], [], [2, 3, 1]],                                       # 5: an empty sentence between two sentences
        [ids("the the the the the")],                                     # 6
        [ids("a man plays the guitar"), ids("a man plays the guitar")],   # 7: the same sentence twice
        [ids("a b"), ids("c d"), ids("b c")],                             # 8: nothing may match across the boundary
        [few(255)], [few(256)], [few(257)],                               # 9-11: around one wave-stride multiple
        [long],                                                           # 12: the limit as one sentence
        [long[k:k + 4] for k in range(0, 1024, 4)],                       # 13: the limit as 256 sentences of 4
        [[0, -1, 2 ** 31 - 1, 0, -1, 2 ** 31 - 1, -1], [2 ** 31 - 1, 0, -1]],   # 14: any id is a word
        [[], [], []],                                                     # 15: only empty sentences
    ]
    return cases


def test_edge_paragraphs_in_one_launch():
    cases = edge_paragraphs()
    got = run(cases)
    np.testing.assert_array_equal(got, want(cases))
    assert not got[0].any() and not got[15].any()
    np.testing.assert_array_equal(got[1], [[1, 1, 0, 0, 1], [0] * 5, [0] * 5, [0] * 5])
    for n in (2, 3, 4):                                                   # the n - 1 tokens carry no n-gram, the n tokens one
        np.testing.assert_array_equal(got[n][n - 1], [1, 1, 0, 0, 1])
    np.testing.assert_array_equal(got[5][1], [4, 3, 2, 1, 2])            # "1 2", "2 3" | | "2 3", "3 1": only "2 3" repeats
    np.testing.assert_array_equal(got[6][1], [4, 1, 4, 0, 4])
    np.testing.assert_array_equal(got[7], [[10, 5, 10, 5, 2], [8, 4, 8, 4, 2], [6, 3, 6, 3, 2], [4, 2, 4, 2, 2]])
    np.testing.assert_array_equal(got[8][1], [3, 3, 0, 0, 1])
    assert [int(got[k][0][0]) for k in (9, 10, 11)] == [255, 256, 257]
    assert got[12][:, 0].tolist() == [1024, 1023, 1022, 1021] and not got[12][:, 3].any()
    assert got[13][:, 0].tolist() == [1024, 768, 512, 256] and got[13][3, 3] > 0
    np.testing.assert_array_equal(got[14][0], [10, 3, 10, 3, 4])


def test_adjacent_paragraphs_do_not_leak():
    a = [ids("a man plays"), ids("a man sings")]
    b = [ids("a man plays"), ids("plays a man plays")]
    c = [ids("sings a man")]
    both = run([a, b, [], c, a])
    for k, p in enumerate([a, b, [], c, a]):
        assert both[k].tobytes() == run([p])[0].tobytes(), k
    np.testing.assert_array_equal(both, want([a, b, [], c, a]))
    assert both[3][:, 2:4].sum() == 0                                     # c repeats nothing of its neighbours


@pytest.fixture(scope="module")
def random_job():
    rng = np.random.RandomState(17)
    paras = [[rng.randint(0, 12, rng.randint(0, 21)).tolist() for _ in range(rng.randint(0, 13))] for _ in range(300)]
    big = rng.randint(0, 12, 1024).tolist()
    cuts = [0] + sorted(rng.choice(np.arange(1, 1024), 40, replace=False).tolist()) + [1024]
    paras.insert(150, [big[a:b] for a, b in zip(cuts[:-1], cuts[1:])])
    return paras, want(paras)


def test_random_job_matches_the_restatement_and_repeats_bit_for_bit(random_job):
    paras, exp = random_job
    got = run(paras)
    np.testing.assert_array_equal(got, exp)
    assert got[150][0][0] == 1024 and np.count_nonzero(got[:, 1, 3]) > 150 and np.count_nonzero(got[:, 3, 3]) > 0
    assert run(paras).tobytes() == got.tobytes()


def test_refusals_leave_the_output_untouched():
    from bmhrl_amd import _lib, ops
    lib = _lib.load()
    tok = torch.arange(1030, **I32)
    stats = torch.full((3, 4, 5), -7, **I32)

    def call(sent_off, para_off, n_tok=6, S=None, G=None, null=None):
        so, po = torch.tensor(sent_off, **I32), torch.tensor(para_off, **I32)
        p = [None if i == null else t.data_ptr() for i, t in enumerate((tok, so, po, stats))]
        return lib.bmhrl_ngram_stats(p[0], n_tok, p[1], len(sent_off) - 1 if S is None else S, p[2],
                                     len(para_off) - 1 if G is None else G, p[3], ops.stream())
    good = ([0, 2, 2, 6], [0, 1, 3])
    for null in range(4):
        assert call(*good, null=null) == -22
    assert call(*good, G=0) == -22 and call(*good, G=-1) == -22 and call(*good, S=-1) == -22 and call(*good, n_tok=-1) == -22
    assert call([0, 3, 2, 6], [0, 1, 3]) == -22 and call([0, 2, 2, 6], [0, 3, 2, 3]) == -22        # descending
    assert call([1, 2, 2, 6], [0, 1, 3]) == -22 and call([0, 2, 2, 5], [0, 1, 3]) == -22           # not spanning [0, n_tok]
    assert call([0, 2, 2, 7], [0, 1, 3]) == -22
    assert call([0, 2, 2, 6], [1, 1, 3]) == -22 and call([0, 2, 2, 6], [0, 1, 2]) == -22           # not spanning [0, S]
    assert call([0, 2, 2, 6], [0, 1, 4]) == -22
    assert call([0, 1025], [0, 1], n_tok=1025) == -22                                               # one sentence past the limit
    assert call([0, 5, 1030], [0, 0, 2, 2], n_tok=1030) == -22                                      # two sentences past it
    torch.cuda.synchronize()
    assert bool((stats == -7).all())
    assert call(*good) == 0                                                                         # (valid: two paragraphs)
    torch.cuda.synchronize()
    assert stats[0, 0].tolist() == [2, 2, 0, 0, 1] and stats[1, 0].tolist() == [4, 4, 0, 0, 1] and bool((stats[2] == -7).all())
    assert call([0, 5, 1029], [0, 1, 2, 2], n_tok=1029) == 0                                        # (valid: 5, 1024 and 0 tokens)
    torch.cuda.synchronize()
    assert stats[1, 0].tolist() == [1024, 1024, 0, 0, 1] and stats[1, 3].tolist() == [1021, 1021, 0, 0, 1]
    assert not stats[2].any()
    with pytest.raises(ValueError):
        ops.ngram_stats(tok.long(), torch.tensor([0, 6], **I32), torch.tensor([0, 1], **I32))
    with pytest.raises(ValueError):
        ops.ngram_stats(tok, torch.tensor([[0, 6]], **I32), torch.tensor([0, 1], **I32))
    with pytest.raises(ValueError):
        ops.ngram_stats(tok[::2], torch.tensor([0, 6], **I32), torch.tensor([0, 1], **I32))
    with pytest.raises(_lib.HipError):
        ops.ngram_stats(tok[:1025], torch.tensor([0, 1025], **I32), torch.tensor([0, 1], **I32))
    with pytest.raises(ValueError, match="1025 tokens"):
        from bmhrl_amd.evaluate import paragraph_stats
        paragraph_stats([[["w"] * 1025]], DEV)


def test_ngram_stats_is_one_launch(monkeypatch):
    from bmhrl_amd import ops
    calls = []
    real = ops._launch
    monkeypatch.setattr(ops, "_launch", lambda name, *a: (calls.append(name), real(name, *a))[1])
    run([[[1, 2, 3]], [[1, 1]]])
    assert calls == ["bmhrl_ngram_stats"]


@pytest.mark.parametrize("top,sort_references", [(None, False), (3, True)])
def test_end_to_end(job, top, sort_references):  # noqa: F811
    from bmhrl_amd import ops
    from bmhrl_amd.evaluate import DenseCaptionEvaluator, tokenize
    gts, results = job
    sub = {"results": results, "version": "x", "external_data": {}}
    tious = [0.3, 0.5, 0.7]
    st = DictStemmer()
    launches = []
    real = ops._launch
    ops._launch = lambda name, *a: (launches.append(name), real(name, *a))[1]
    try:
        ev = DenseCaptionEvaluator(gts, sub, tious, 1000, device=DEV, stemmer=st, synonyms=dict_synonyms, paragraph=True,
                                   paragraph_top=top, sort_references=sort_references)
        ev.evaluate()
    finally:
        ops._launch = real
    assert launches.count("bmhrl_ngram_stats") == 1                       # every video once, not once per file
    exp, exp_video = pr.evaluate(gts, sub, len(tious), 1000, tokenize, st.stem, dict_synonyms, top, sort_references)
    assert sorted(k for k in ev.scores if k.startswith("Para_")) == sorted(PARA_KEYS) == sorted(exp)
    for k in PARA_KEYS:
        print(k, ev.scores[k], exp[k])
        assert len(ev.scores[k]) == len(tious) and ev.scores[k][0] == ev.scores[k][1] == ev.scores[k][2]
        np.testing.assert_allclose(ev.scores[k], exp[k], rtol=RTOL, atol=0, err_msg=k)
    for k in pr.STAT_KEYS:                                                # quotients of equal integers, summed in one order
        assert ev.scores[k] == exp[k], k
    assert ev.scores["Para_METEOR"][0] > 0.0 and ev.scores["Para_CIDEr"][0] > 0.0 and ev.scores["Para_Bleu_4"][0] > 0.0
    if top is None:                                                       # v1 says "a man plays a guitar" twice
        assert ev.scores["Para_RE_4"][0] == ev.scores["Para_XRE_4"][0] == (6 - 4) / 6
    assert list(ev.paragraph_per_video) == list(exp_video) == ["v1", "v2", "v3", "v4", "v5"]
    for vid, rec in ev.paragraph_per_video.items():
        assert sorted(rec) == ["sentences", "stats", "tokens"]
        assert rec["stats"].dtype == np.int32 and rec["stats"].shape == (4, 5)
        assert rec["stats"].tolist() == exp_video[vid]["stats"], vid
        assert (rec["sentences"], rec["tokens"]) == (exp_video[vid]["sentences"], exp_video[vid]["tokens"]), vid


def test_defaults_are_unchanged(job):  # noqa: F811
    from bmhrl_amd.evaluate import DenseCaptionEvaluator
    gts, results = job
    sub = {"results": results, "version": "x", "external_data": {}}
    kw = dict(device=DEV, stemmer=DictStemmer(), synonyms=dict_synonyms, verbose=True)
    plain = DenseCaptionEvaluator(gts, sub, [0.3, 0.7], 1000, **kw)
    off = DenseCaptionEvaluator(gts, sub, [0.3, 0.7], 1000, paragraph=False, paragraph_top=2, **kw)
    on = DenseCaptionEvaluator(gts, sub, [0.3, 0.7], 1000, paragraph=True, **kw)
    for ev in (plain, off, on):
        ev.evaluate()
    assert list(plain.scores) == list(off.scores) and not any(k.startswith("Para_") for k in off.scores)
    assert off.paragraph_per_video == {}
    for k in plain.scores:
        assert np.asarray(plain.scores[k]).tobytes() == np.asarray(off.scores[k]).tobytes(), k
        assert np.asarray(plain.scores[k]).tobytes() == np.asarray(on.scores[k]).tobytes(), k     # the other keys do not move
    assert list(on.scores)[:len(plain.scores) - 2] == list(plain.scores)[:-2]                     # Para_* before Recall, Precision


def test_loop_writes_the_paragraph_scalars(setup, tmp_path):  # noqa: F811
    from epoch_loops.validation_loops import validation_1by1_loop
    from epoch_loops.captioning_bmrl_loops import bmhrl_greedy_decoder
    cfg, ds, loader, agent, wv, ls, bkl, dev = setup
    cfg.max_len, cfg.modality, cfg.log_path, cfg.max_prop_per_vid = 6, "audio_video", str(tmp_path), 100
    refs = []
    for k in range(2):                                    # references over the synthetic vocabulary's words
        gt = {f"v{j}": {"duration": 1.0, "timestamps": [[0.0, 1.0], [0.0, 0.6]],
                        "sentences": [" ".join(f"w{(7 * j + 3 * k + i) % 80}" for i in range(5)), f"W{j + 4} w{k + 5}."]}
              for j in range(4 if k else 5)}              # (v4 has no predictions)
        refs.append(str(tmp_path / f"ref{k}.json"))
        with open(refs[-1], "w") as f:
            json.dump(gt, f)
    cfg.reference_paths, cfg.tIoUs = refs, [0.3, 0.5, 0.7, 0.9]
    base = dict(device=dev, stemmer=DictStemmer(), synonyms=dict_synonyms)
    old_itos3 = ds.train_vocab.itos[3]
    ds.train_vocab.itos[3] = "</s>"
    wrapped = SimpleNamespace(module=agent, eval=agent.eval)
    agent.set_inference_mode(True)
    scalars = []
    board = SimpleNamespace(add_scalar=lambda tag, value, step: scalars.append((tag, value)))
    usual = ["meteor", "bleu4", "bleu3", "precision", "recall"]
    try:
        ds.phase = "val_1"
        cfg.caption_evaluator_options = dict(base, paragraph=True)
        out = validation_1by1_loop(cfg, wrapped, loader, bmhrl_greedy_decoder, 0, board, evaluator="device")
        assert list(out) == [0.5, "Average across tIoUs"]
        for entry in out.values():
            assert set(PARA_KEYS) <= set(entry)
            for name in PARA_KEYS:
                assert 0.0 <= entry[name] <= (10.0 if name == "Para_CIDEr" else 1.0), (name, entry[name])
        avg = out["Average across tIoUs"]
        assert [t for t, _ in scalars] == [f"val_1/{t}" for t in usual + ["para_meteor", "para_cider", "para_re4",
                                                                          "duration_of_1by1"]]
        written = dict(scalars)
        assert written["val_1/para_meteor"] == avg["Para_METEOR"] * 100 and written["val_1/para_cider"] == avg["Para_CIDEr"] * 100
        assert written["val_1/para_re4"] == avg["Para_RE_4"] * 100
        ds.phase = "learned_props"                        # every tIoU of the config
        out = validation_1by1_loop(cfg, wrapped, loader, bmhrl_greedy_decoder, 0, None, evaluator="device")
        assert list(out) == cfg.tIoUs + ["Average across tIoUs"]
        for entry in out.values():
            assert set(PARA_KEYS) <= set(entry)
            assert all(entry[k] == out[0.3][k] for k in PARA_KEYS)        # a paragraph does not depend on the threshold
        ds.phase = "val_1"
        del scalars[:]
        cfg.caption_evaluator_options = base              # without the option: today's scalars
        out = validation_1by1_loop(cfg, wrapped, loader, bmhrl_greedy_decoder, 1, board, evaluator="device")
        assert not any(k.startswith("Para_") for k in out["Average across tIoUs"])
        assert [t for t, _ in scalars] == [f"val_1/{t}" for t in usual + ["duration_of_1by1"]]
    finally:
        ds.phase = "train"
        ds.train_vocab.itos[3] = old_itos3
        del cfg.caption_evaluator_options
