"""Device METEOR rewards (csrc/meteor.hip): one JSON line with
- the device time of the bmhrl_meteor launch and of one worker-reward call (scorer.reward_fn() on bound captions: the
  launch and the discount product) at B = 16 and 64, L = 30, all three stages on, from graphs of 20 calls -- and of the
  launch with the exact stage alone and with exact + stem, which tells what each stage costs;
- the CIDEr and BLEU launches and calls at the same shapes in the same process (tests/bench_rewards.py's data: vocabulary
  10172, a 20000-caption corpus, references of 8..20 words);
- the host restatement's time for the same METEOR rows at B = 16 (tests/meteor_reference.py, one thread);
- the construction time of the METEOR tables.
The stemmer and the synonyms are synthetic and sized like the real ones: stems shared by three words, synonym sets of
0..24 words (12 on average) of which a few are outside the vocabulary."""
import json
import os
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bmhrl_amd.rewards import BleuScorer, CiderScorer, MeteorScorer  # noqa: E402
from tests import meteor_reference as mr  # noqa: E402
from tests.bench_rewards import data, graph_us, launch_us  # noqa: E402


class Stemmer:
    def stem(self, word):
        return f"s{int(word[1:]) // 3}" if word[1:].isdigit() else word


def synonyms(word):
    if not word[1:].isdigit():
        return []
    i = int(word[1:])
    return [f"w{i + 1 + 7 * k}" for k in range(i % 25)] + ([f"lemma{i}"] if i % 4 == 0 else [])


def main():
    dev = torch.device("cuda:0")
    itos, corpus, caps, hyp = data()
    vocab = types.SimpleNamespace(itos=itos)
    t0 = time.perf_counter()
    met = MeteorScorer(vocab, dev, 0.9, 0.7, stemmer=Stemmer(), synonyms=synonyms)
    out = {"metric": "meteor reward launch", "meteor_construction_s": round(time.perf_counter() - t0, 3),
           "synonym_ids": int(met.tables.syn_off[-1])}
    scorers = [("meteor", met), ("meteor_exact_stem", MeteorScorer(vocab, dev, 0.9, 0.7, stemmer=Stemmer(), synonyms=False)),
               ("meteor_exact", MeteorScorer(vocab, dev, 0.9, 0.7, stemmer=False, synonyms=False)),
               ("cider", CiderScorer(vocab, iter(corpus), dev, 0.9, 0.7)), ("bleu", BleuScorer(vocab, dev, 0.9, 0.7))]
    for name, sc in scorers:
        for B in (16, 64):
            pred = hyp[:B].to(dev)
            sc.bind(caps[:B])
            fn = sc.reward_fn()
            out[f"{name}_B{B}_launch_us"] = round(graph_us(lambda: sc._launch(pred)), 1)
            if "_exact" not in name:
                out[f"{name}_B{B}_call_us"] = round(graph_us(lambda: fn(pred, None)), 1)
                out[f"{name}_B{B}_eager_call_us"] = round(launch_us(lambda: fn(pred, None)), 1)
    t0 = time.perf_counter()
    met.bind(caps[:16])
    torch.cuda.synchronize()
    out["meteor_bind_B16_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    rows = hyp[:16].tolist()
    stem = Stemmer().stem
    t0 = time.perf_counter()
    for i, r in enumerate(rows):
        mr.meteor_scores(itos, r, caps[i], stem, synonyms)
    out["host_restatement_meteor_B16_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
