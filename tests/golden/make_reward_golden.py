"""Runs the reference's own CiderScorer (metrics/cider.py) and BleuScorer (metrics/bleu.py) on small cases and writes
tests/golden/rewards.npz: the vocabulary, corpus, captions and sampled rows as plain (unicode / integer) arrays, and per
case the worker and manager outputs, the per-prefix `rewards` rows and the sections after delta_cider_manager's in-place
write.  The scorers import nltk (metrics/batched_meteor.py) and tqdm without using them here: empty stand-in modules let
them import.  The archive is written with fixed zip timestamps, so a rerun reproduces it byte for byte.
usage: make_reward_golden.py REFERENCE_CHECKOUT"""
import io
import os
import sys
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "rewards.npz")

ITOS = ["<unk>", "<pad>", "<s>", "</s>", "a", "man", "Man", "is", "playing", "guitar", "the", "dog", "runs", "  ", "",
        "Dog", "on", "grass", " red ", "ball", "A", "woman", "sings", "with", "</s>x", "PLAYING", "song", "and", "field", "."]
CORPUS = [
    "a man is playing guitar", "a man is playing a guitar", "the dog runs on the grass", "a dog runs on grass",
    "a woman sings a song", "a woman sings with a man", "the man is playing guitar on the grass", "a red ball",
    "the dog is playing with a red ball", "a man and a woman sing a song", "the woman is playing guitar", "a dog runs",
    "Man is playing", "Man is playing guitar", "the Dog runs on the field", "the Dog runs on the field .",
    "a man is playing guitar .", "a woman sings .", "a dog is on the grass", "a man is on the field",
]
CAPTIONS = [
    "A man is playing guitar.",
    "a man is playing a guitar",
    "The DOG runs on the grass , happily",
    "",
    "a woman sings a song with a man and a woman",
    "zebra quokka man is playing",
    "a red ball a red ball",
    "Man is PLAYING guitar on the field .",
]
# sampled rows (vocab ids): end token first, in the middle, absent, repeated; whitespace-only and empty entries;
# repeated n-grams; uppercase entries
HYP = [
    [3, 4, 5, 7, 8, 9, 1, 1, 1, 1, 1, 1],
    [4, 5, 7, 8, 9, 3, 1, 1, 1, 1, 1, 1],
    [10, 11, 12, 16, 10, 17, 13, 12, 16, 10, 17, 28],
    [4, 14, 5, 13, 7, 3, 3, 4, 5, 3, 9, 9],
    [20, 21, 22, 4, 26, 23, 4, 6, 27, 4, 21, 3],
    [6, 7, 25, 9, 6, 7, 25, 9, 6, 7, 25, 9],
    [4, 18, 19, 4, 18, 19, 4, 18, 19, 24, 29, 3],
    [13, 14, 13, 6, 7, 8, 9, 16, 10, 28, 29, 3],
]
CASES = [(1, 6.0, "hyp"), (2, 6.0, "hyp"), (3, 6.0, "hyp"), (4, 6.0, "hyp"), (4, 3.0, "hyp"), (2, 3.0, "hyp"),
         (4, 6.0, "hyp1"), (1, 3.0, "hyp1")]
GAMMA, GAMMA_M = 0.9, 0.7


def stub_modules():
    """nltk and tqdm stand-ins: metrics/batched_meteor.py and metrics/bleu.py import names from them at module level"""
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    unused = lambda *a, **k: None           # noqa: E731
    mod("nltk")
    mod("nltk.translate", meteor=unused)
    mod("nltk.translate.meteor_score", meteor_score=unused, single_meteor_score=unused)
    mod("nltk.tokenize")
    mod("nltk.tokenize.treebank", TreebankWordDetokenizer=type("TreebankWordDetokenizer", (), {}))
    mod("tqdm", tqdm=unused)


def sections_for(B, L):
    s = np.zeros((B, L), dtype=np.int64)
    for b in range(B):
        s[b, (b * 5 + 2) % L] = 1
        s[b, (b * 3 + 1) % L] = 1
    return s


def save(path, arrays):
    """np.savez layout (one .npy member per array), deflated, with fixed timestamps"""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o600 << 16
            zf.writestr(info, buf.getvalue())


def main(ref):
    stub_modules()
    sys.path.insert(0, os.path.abspath(ref))
    import torch
    from metrics.cider import CiderScorer
    from metrics.bleu import BleuScorer
    vocab = types.SimpleNamespace(itos=ITOS)
    corpus = [c.split() for c in CORPUS]
    hyps = {"hyp": torch.tensor(HYP, dtype=torch.int64), "hyp1": torch.tensor([[r[0]] for r in HYP], dtype=torch.int64)}
    out = {"itos": np.array(ITOS), "corpus": np.array(CORPUS), "captions": np.array(CAPTIONS),
           "hyp": hyps["hyp"].numpy(), "hyp1": hyps["hyp1"].numpy(), "gamma": np.array([GAMMA, GAMMA_M])}
    cases = []
    for c, (n, sigma, which) in enumerate(CASES):
        pred = hyps[which]
        B, L = pred.shape
        cases.append([n, sigma, 1.0 if which == "hyp1" else 0.0])
        cid = CiderScorer(vocab, iter(corpus), "cpu", GAMMA, GAMMA_M, n=n, sigma=sigma)
        ble = BleuScorer(vocab, "cpu", GAMMA, GAMMA_M, n=n, sigma=sigma)
        w, r = cid.delta_cider_worker(pred, CAPTIONS)
        out[f"c{c}_cider_worker"], out[f"c{c}_cider_rewards"] = w.numpy(), r.numpy()
        w, r = ble.delta_bleu_worker(pred, CAPTIONS)
        out[f"c{c}_bleu_worker"], out[f"c{c}_bleu_rewards"] = w.numpy(), r.numpy()
        if which == "hyp":                  # every caption is shorter than L: delta_cider_manager's write stays in range
            sec = torch.from_numpy(sections_for(B, L))
            m, _ = cid.delta_cider_manager(pred, CAPTIONS, None, sec)
            out[f"c{c}_cider_manager"], out[f"c{c}_cider_sections"] = m.numpy(), sec.numpy()
            sec = torch.from_numpy(sections_for(B, L))
            m, _ = ble.delta_bleu_manager(pred, CAPTIONS, None, sec)
            out[f"c{c}_bleu_manager"] = m.numpy()
    out["cases"] = np.array(cases, dtype=np.float64)
    out["sections_in"] = sections_for(len(HYP), len(HYP[0]))
    save(OUT, out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
