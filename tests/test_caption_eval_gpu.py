"""The dense-captioning evaluator on the GPU (csrc/caption_eval.hip through ops.caption_eval and bmhrl_amd/evaluate.py)
against the float64 restatement (tests/caption_eval_reference.py) and the fixture recorded from the reference's
ANETcaptions (tests/golden/caption_eval.json).  Integers are exact; the fp64 values are held to 1e-12 relative, the bound
DESIGN.md section 13 measured for the same kind of arithmetic (pow, exp, log and sqrt differ from the host's in the last
place; every sum here adds non-negative terms in the restatement's order)."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import caption_eval_reference as cr
from tests.conftest import GOLDEN
from tests.meteor_reference import DictStemmer, dict_synonyms
from tests.test_loops_gpu import setup  # noqa: F401  (the synthetic loader and agent of the loop tests)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
RTOL = 1e-12


def run(pairs, off):
    """ops.caption_eval of token pairs grouped by off -> numpy (pair_ints, pair_lcs, pair_cider, group_scores)"""
    from bmhrl_amd import ops
    from bmhrl_amd.evaluate import encode_pairs
    arrays = encode_pairs([h for h, _ in pairs], [r for _, r in pairs])
    dev = [torch.from_numpy(a).to(DEV) for a in arrays + (np.asarray(off, dtype=np.int32),)]
    return tuple(t.cpu().numpy() for t in ops.caption_eval(*dev))


def want(pairs, off):
    """the same four arrays by the restatement, group by group"""
    ints, lcs, cider, groups = [], [], [], []
    for g0, g1 in zip(off[:-1], off[1:]):
        grp = pairs[g0:g1]
        if not grp:
            groups.append([0.0] * 6)
            continue
        for h, r in grp:
            guess, correct, tl, rl = cr.bleu_counts(h, r)
            ints.append(guess + correct + [tl, rl])
            lcs.append(cr.lcs(h, r))
        c = cr.cider_pairs(grp)
        cider += c
        groups.append(cr.bleu_group(grp) + [cr.mean([cr.rouge_pair(h, r) for h, r in grp]), cr.mean(c)])
    return np.array(ints, dtype=np.int32), np.array(lcs, dtype=np.int32), np.array(cider), np.array(groups)


def check(got, exp):
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == got[3].dtype == np.float64
    np.testing.assert_array_equal(got[0], exp[0])
    np.testing.assert_array_equal(got[1], exp[1])
    np.testing.assert_allclose(got[2], exp[2], rtol=RTOL, atol=0)
    np.testing.assert_allclose(got[3], exp[3], rtol=RTOL, atol=0)


def test_the_four_hand_checked_pairs():
    got = run(cr.HAND_PAIRS, [0, 4])
    check(got, want(cr.HAND_PAIRS, [0, 4]))
    np.testing.assert_array_equal(got[0][0], [6, 5, 4, 3, 3, 1, 0, 0, 6, 7])
    np.testing.assert_array_equal(got[0][3], [0, 0, 0, 0, 0, 0, 0, 0, 0, 3])
    np.testing.assert_array_equal(got[1], cr.HAND_LCS)
    np.testing.assert_allclose(got[2], cr.HAND_CIDER_PAIRS, rtol=RTOL, atol=0)
    np.testing.assert_allclose(got[3][0, :4], cr.HAND_BLEU, rtol=RTOL, atol=0)
    np.testing.assert_allclose(got[3][0, 4], cr.mean(cr.HAND_ROUGE), rtol=RTOL, atol=0)
    np.testing.assert_allclose(got[3][0, 5], cr.HAND_CIDER, rtol=RTOL, atol=0)


def test_edge_cases_each_in_a_group_of_its_own():
    rng = np.random.RandomState(5)
    vocab = [f"w{i}" for i in range(9)]
    long_h, long_r = [vocab[i] for i in rng.randint(0, 9, 256)], [vocab[i] for i in rng.randint(0, 9, 512)]
    filler = ("a dog runs fast".split(), "the dog runs".split())
    cases = [
        [("a man sits".split(), "a man sits down".split())],                       # one pair only
        [("a man plays the guitar".split(), "a man plays the guitar".split()), filler],
        [("dog".split(), "the dog runs".split()), filler],                          # a one-word hypothesis
        [("the the the".split(), "the cat".split()), filler],                       # a repeated word is clipped
        [([], "a man sits".split()), filler],                                       # an empty hypothesis
        [("a man sits".split(), [cr.GARBAGE]), filler],                             # the garbage reference
        [(long_h, long_r), (long_h[:40], long_r[:50])],                             # the length limits
    ]
    pairs = [p for c in cases for p in c]
    off = np.concatenate([[0], np.cumsum([len(c) for c in cases])]).tolist()
    got = run(pairs, off)
    check(got, want(pairs, off))
    assert got[2][0] == 0.0 and got[3][0, 5] == 0.0                                 # one pair: CIDEr is exactly 0
    np.testing.assert_array_equal(got[0][1], [5, 4, 3, 2, 5, 4, 3, 2, 5, 5])        # hypothesis == reference
    assert got[1][1] == 5 and got[2][1] > 0.0
    np.testing.assert_array_equal(got[0][3], [1, 0, 0, 0, 1, 0, 0, 0, 1, 3])        # one word: no 2..4-gram guesses
    np.testing.assert_array_equal(got[0][5], [3, 2, 1, 0, 1, 0, 0, 0, 3, 2])        # "the" counts once
    np.testing.assert_array_equal(got[0][7], [0, 0, 0, 0, 0, 0, 0, 0, 0, 3])        # empty
    assert got[1][7] == 0 and got[2][7] == 0.0
    np.testing.assert_array_equal(got[0][9][4:], [0, 0, 0, 0, 3, 1])                # garbage: nothing matches
    assert got[1][9] == 0 and got[2][9] == 0.0
    np.testing.assert_array_equal(got[0][11][8:], [256, 512])


def test_document_frequencies_do_not_leak_between_groups():
    a = [("a man plays the guitar".split(), "a man plays the guitar on stage".split()),
         ("the man plays".split(), "a man plays the guitar".split()),
         ("a guitar".split(), "the guitar on stage".split())]
    b = [(h, r) for h, r in reversed(a)] + [a[0]]                                   # the same grams, other counts
    both = run(a + b, [0, 3, 7])
    alone_a, alone_b = run(a, [0, 3]), run(b, [0, 4])
    for k in range(3):
        assert both[k][:3].tobytes() == alone_a[k].tobytes()
        assert both[k][3:].tobytes() == alone_b[k].tobytes()
    assert both[3][0].tobytes() == alone_a[3][0].tobytes() and both[3][1].tobytes() == alone_b[3][0].tobytes()
    assert not np.array_equal(both[2][:3], both[2][[5, 4, 3]])                      # (the groups do weigh the grams apart)
    check(both, want(a + b, [0, 3, 7]))


@pytest.fixture(scope="module")
def random_job():
    rng = np.random.RandomState(11)
    vocab = [f"w{i}" for i in range(12)]

    def sent(max_len):
        return [vocab[i] for i in rng.randint(0, 12, rng.randint(0, max_len + 1))]
    sizes = []
    while sum(sizes) < 300:
        sizes.append(int(rng.randint(1, 34)))
    sizes += [257, 0, 2048]                               # more pairs than a workgroup has threads; empty; the largest
    pairs = []
    for n in sizes:
        pairs += [(sent(6 if n == 2048 else 12), sent(6 if n == 2048 else 12)) for _ in range(n)]
    off = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    return pairs, off, want(pairs, off)


def test_random_job_matches_the_restatement_and_repeats_bit_for_bit(random_job):
    pairs, off, exp = random_job
    got = run(pairs, off)
    check(got, exp)
    assert np.count_nonzero(got[2]) > 100 and np.count_nonzero(got[1]) > 100
    assert not got[3][-2].any()                           # the empty group
    again = run(pairs, off)
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()


def test_meteor_is_the_mean_of_the_whole_sentence_scores():
    from bmhrl_amd.evaluate import score_pairs
    from bmhrl_amd.rewards import MeteorTables
    st = DictStemmer()
    pairs = [("a big dog walks fast".split(), "the large dogs walked quick".split()),
             ("the cat jumps".split(), "a feline jumped on the man".split()),
             ([], "a man".split()),
             ("a man".split(), [cr.GARBAGE]),
             ("dogs play with a small cat".split(), "dogs play with a small cat".split()),
             ("the man plays and the man walks".split(), "a man walking and playing".split())]
    off = [0, 2, 2, 5, 6]
    words = sorted({w for h, _ in pairs for w in h})
    for stem, syn in ((True, True), (True, False), (False, True), (False, False)):
        tables = MeteorTables(words, st if stem else False, dict_synonyms if syn else False)
        got = score_pairs([h for h, _ in pairs], [r for _, r in pairs], off, DEV, tables)["METEOR"]
        per_pair = [cr.meteor_pair(h, r, st.stem if stem else None, dict_synonyms if syn else None) for h, r in pairs]
        exp = [cr.mean(per_pair[a:b]) if b > a else 0.0 for a, b in zip(off[:-1], off[1:])]
        assert any(per_pair) and per_pair[2] == 0.0 and per_pair[3] == 0.0
        np.testing.assert_allclose(got, exp, rtol=RTOL, atol=0)


def test_fixture_end_to_end(tmp_path):
    from bmhrl_amd.evaluate import DenseCaptionEvaluator
    with open(os.path.join(GOLDEN, "caption_eval.json")) as f:
        fx = json.load(f)
    paths = []
    for name, obj in (("a.json", fx["ground_truths"][0]), ("b.json", fx["ground_truths"][1]), ("s.json", fx["submission"])):
        paths.append(str(tmp_path / name))
        with open(paths[-1], "w") as f:
            json.dump(obj, f)
    ev = DenseCaptionEvaluator(paths[:2], paths[2], fx["tious"], fx["max_proposals"], device=DEV, stemmer=DictStemmer(),
                               synonyms=dict_synonyms)
    ev.evaluate()
    assert sorted(ev.scores) == sorted(k for k in fx["scores"] if k not in ("Precision", "Recall"))
    for name, got in ev.scores.items():
        print(name, got, fx["scores"][name])
        np.testing.assert_allclose(got, fx["scores"][name], rtol=RTOL, atol=0, err_msg=name)
    # already loaded dicts instead of paths
    ev2 = DenseCaptionEvaluator(fx["ground_truths"], fx["submission"], [0.5], fx["max_proposals"], device=DEV,
                                stemmer=DictStemmer(), synonyms=dict_synonyms)
    ev2.evaluate()
    assert all(ev2.scores[k][0] == ev.scores[k][1] for k in ev.scores)


def test_loop_scores_on_the_device(setup, tmp_path):  # noqa: F811
    from epoch_loops.validation_loops import validation_1by1_loop
    from epoch_loops.captioning_bmrl_loops import bmhrl_greedy_decoder
    cfg, ds, loader, agent, wv, ls, bkl, dev = setup
    cfg.max_len, cfg.modality, cfg.log_path, cfg.max_prop_per_vid = 6, "audio_video", str(tmp_path), 100
    refs = []
    for k in range(4):                                    # references over the synthetic vocabulary's words
        gt = {f"v{j}": {"duration": 1.0, "timestamps": [[0.0, 1.0], [0.0, 0.6]],
                        "sentences": [" ".join(f"w{(7 * j + 3 * k + i) % 80}" for i in range(5)), f"W{j + 4} w{k + 5}."]}
              for j in range(4 if k else 5)}              # (v4 has no predictions)
        refs.append(str(tmp_path / f"ref{k}.json"))
        with open(refs[-1], "w") as f:
            json.dump(gt, f)
    cfg.reference_paths, cfg.tIoUs = refs, [0.3, 0.5, 0.7, 0.9]
    cfg.caption_evaluator_options = dict(device=dev, stemmer=DictStemmer(), synonyms=dict_synonyms)
    old_itos3 = ds.train_vocab.itos[3]
    ds.train_vocab.itos[3] = "</s>"
    wrapped = SimpleNamespace(module=agent, eval=agent.eval)
    agent.set_inference_mode(True)
    scalars = []
    board = SimpleNamespace(add_scalar=lambda tag, value, step: scalars.append(tag))
    try:
        for phase, keys in (("val_1", [0.5]), ("learned_props", cfg.tIoUs)):
            ds.phase = phase
            out = validation_1by1_loop(cfg, wrapped, loader, bmhrl_greedy_decoder, 0, board, evaluator="device")
            assert list(out) == keys + ["Average across tIoUs"]
            for entry in out.values():
                assert sorted(entry) == sorted(["Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "METEOR", "ROUGE_L", "CIDEr", "Precision",
                                                "Recall"])
                for name, value in entry.items():
                    assert 0.0 <= value <= (10.0 if name == "CIDEr" else 1.0), (name, value)
            assert out[0.5]["Recall"] > 0.0               # [0, 1] against [0, 1]: covered at 0.5
        assert scalars == [f"val_1/{t}" for t in ("meteor", "bleu4", "bleu3", "precision", "recall", "duration_of_1by1")]
        cfg.caption_evaluator = "device"                  # six positional arguments: the config selects the evaluator
        ds.phase = "val_1"
        out = validation_1by1_loop(cfg, wrapped, loader, bmhrl_greedy_decoder, 1, None)
        assert list(out) == [0.5, "Average across tIoUs"]
    finally:
        ds.phase = "train"
        ds.train_vocab.itos[3] = old_itos3
        del cfg.caption_evaluator_options
        if hasattr(cfg, "caption_evaluator"):
            del cfg.caption_evaluator


def test_refusals():
    from bmhrl_amd import _lib, ops
    lib = _lib.load()
    P, G, L, R = 3, 2, 4, 5
    i32 = dict(dtype=torch.int32, device=DEV)
    hyp, ref = torch.zeros(P, L, **i32), torch.zeros(P, R, **i32)
    hl, rl = torch.ones(P, **i32), torch.ones(P, **i32)
    ints, lcs = torch.zeros(P, 10, **i32), torch.zeros(P, **i32)
    cider, groups = torch.zeros(P, dtype=torch.float64, device=DEV), torch.zeros(G, 6, dtype=torch.float64, device=DEV)

    def call(off, P=P, G=G, L=L, R=R, ldh=L, ldr=R, null=None):
        off_t = torch.tensor(off, **i32)
        ptrs = [hyp, hl, ref, rl, off_t, ints, lcs, cider, groups]
        p = [None if i == null else t.data_ptr() for i, t in enumerate(ptrs)]
        return lib.bmhrl_caption_eval(p[0], ldh, p[1], p[2], ldr, p[3], p[4], P, G, L, R, p[5], p[6], p[7], p[8], ops.stream())
    for null in range(9):
        assert call([0, 1, 3], null=null) == -22
    assert call([0, 1, 3], P=0) == -22 and call([0, 1, 3], G=0) == -22
    assert call([0, 2, 1]) == -22 and call([0, 4, 3]) == -22          # descending
    assert call([1, 2, 3]) == -22 and call([0, 1, 2]) == -22          # not spanning [0, P]
    assert call([0, 1, 3], L=257, ldh=257) == -22 and call([0, 1, 3], R=513, ldr=513) == -22
    assert call([0, 1, 3], L=0) == -22 and call([0, 1, 3], ldh=L - 1) == -22 and call([0, 1, 3], ldr=R - 1) == -22
    assert call([0, 1, 3]) == 0 and call([0, 0, 3]) == 0               # (valid; an empty group is allowed)
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.caption_eval(hyp.long(), hl, ref, rl, torch.tensor([0, 1, 3], **i32))
