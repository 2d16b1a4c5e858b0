"""Plain-Python restatement of the per-prefix METEOR rewards: nltk 3.5's single_meteor_score as the
reference's metrics/batched_meteor.py:63-89 calls it, with nltk's list-`pop` loops and Python float arithmetic, one prefix
at a time.  nltk itself is not needed: `stem` is a callable word -> stem (None: no stem stage) and `syn` a callable word ->
iterable of synonyms (None: no synonym stage).  tests/test_meteor_cpu.py pins it to nltk's documented values;
tests/test_meteor_gpu.py checks the device scorer against it.

Each stage works on what the stage before left unmatched."""
import numpy as np

from tests.reward_reference import delta_row as _delta_row, discount  # noqa: F401  (discount: re-exported)


def _match_enums(hyp, ref):
    """nltk's _match_enums: hyp / ref are lists of (position, key), matched pairs are popped from both"""
    word_match = []
    for i in range(len(hyp))[::-1]:
        for j in range(len(ref))[::-1]:
            if hyp[i][1] == ref[j][1]:
                word_match.append((hyp[i][0], ref[j][0]))
                hyp.pop(i)
                ref.pop(j)
                break
    return word_match, hyp, ref


def _stem_match(hyp, ref, stem):
    """_enum_stem_match: exact matching of the stems; the words whose stems stayed unmatched go on"""
    sh = [(p, stem(w)) for p, w in hyp]
    sr = [(p, stem(w)) for p, w in ref]
    word_match, sh, sr = _match_enums(sh, sr)
    left_h, left_r = {p for p, _ in sh}, {p for p, _ in sr}
    return word_match, [x for x in hyp if x[0] in left_h], [x for x in ref if x[0] in left_r]


def _syn_match(hyp, ref, syn):
    """_enum_wordnetsyn_match: the reference word lies in the hypothesis word's synonym set (or is the word itself)"""
    word_match = []
    for i in range(len(hyp))[::-1]:
        hypothesis_syns = set(syn(hyp[i][1])).union({hyp[i][1]})
        for j in range(len(ref))[::-1]:
            if ref[j][1] in hypothesis_syns:
                word_match.append((hyp[i][0], ref[j][0]))
                hyp.pop(i)
                ref.pop(j)
                break
    return word_match, hyp, ref


def align(hyp_words, ref_words, stem=None, syn=None):
    """(matches sorted by hypothesis position, [exact, stem, synonym] match counts)"""
    hyp, ref = list(enumerate(hyp_words)), list(enumerate(ref_words))
    exact, hyp, ref = _match_enums(hyp, ref)
    stems, syns = [], []
    if stem is not None:
        stems, hyp, ref = _stem_match(hyp, ref, stem)
    if syn is not None:
        syns, hyp, ref = _syn_match(hyp, ref, syn)
    return sorted(exact + stems + syns, key=lambda pair: pair[0]), [len(exact), len(stems), len(syns)]


def count_chunks(matches):
    """_count_chunks: 1 + the neighbouring pairs that do not continue each other"""
    i, chunks = 0, 1
    while i < len(matches) - 1:
        if matches[i + 1][0] == matches[i][0] + 1 and matches[i + 1][1] == matches[i][1] + 1:
            i += 1
            continue
        i += 1
        chunks += 1
    return chunks


def meteor_prefix(hyp_words, ref_words, stem=None, syn=None, alpha=0.9, beta=3, gamma=0.5):
    """single_meteor_score of one word list against another"""
    matches, _ = align(hyp_words, ref_words, stem, syn)
    matches_count = len(matches)
    try:
        precision = float(matches_count) / len(hyp_words)
        recall = float(matches_count) / len(ref_words)
        fmean = (precision * recall) / (alpha * precision + (1 - alpha) * recall)
        chunk_count = float(count_chunks(matches))
        frag_frac = chunk_count / matches_count
    except ZeroDivisionError:
        return 0.0
    penalty = gamma * frag_frac ** beta
    return (1 - penalty) * fmean


def meteor_sentence(hypothesis, reference, stem=None, syn=None, **kw):
    """single_meteor_score(reference, hypothesis) of two strings (lowercased, whitespace-split)"""
    return meteor_prefix(hypothesis.lower().split(), reference.lower().split(), stem, syn, **kw)


def meteor_scores(itos, row, caption, stem=None, syn=None, alpha=0.9, beta=3, gamma=0.5):
    """the reference's `rewards` row before its float32 store (fp64, len(row)): every prefix of the row, no cut at an end
    token"""
    hypo = [itos[int(i)] if 0 <= int(i) < len(itos) else "" for i in row]      # (an id outside the vocabulary: no word)
    return np.array([meteor_sentence(" ".join(hypo[:l + 1]), caption, stem, syn, alpha=alpha, beta=beta, gamma=gamma)
                     for l in range(len(hypo))], dtype=np.float64)


def meteor_scores_reduced(itos, row, caption, stem=None, syn=None, alpha=0.9, beta=3, gamma=0.5):
    """the same row by what the `pop` loops reduce to: per stage, the unmatched hypothesis words from last to first each
    take the highest unmatched reference position that passes the stage's test.  The positions that pass do not depend
    on the prefix, so they are one integer bit mask per word; this makes the largest shapes affordable on the host
    (tests/test_meteor_cpu.py checks it against meteor_scores)."""
    hypo = [itos[int(i)] if 0 <= int(i) < len(itos) else "" for i in row]
    counts = [len(" ".join(hypo[:l + 1]).lower().split()) for l in range(len(hypo))]
    words, ref = " ".join(hypo).lower().split(), caption.lower().split()

    def masks(test):
        return [sum(1 << j for j, r in enumerate(ref) if test(w, r)) for w in words]
    stages = [masks(lambda w, r: w == r)]
    if stem is not None:
        ref_stems = [stem(r) for r in ref]
        stages.append([sum(1 << j for j, r in enumerate(ref_stems) if stem(w) == r) for w in words])
    if syn is not None:
        sets = [set(syn(w)).union({w}) for w in words]
        stages.append([sum(1 << j for j, r in enumerate(ref) if r in s) for s in sets])
    by_m = [0.0]
    for m in range(1, len(words) + 1):
        used, mate = 0, [-1] * m
        for cand in stages:
            for h in range(m - 1, -1, -1):
                c = cand[h] & ~used
                if mate[h] < 0 and c:
                    mate[h] = c.bit_length() - 1
                    used |= 1 << mate[h]
        matches = [(h, j) for h, j in enumerate(mate) if j >= 0]
        if not matches or not ref:
            by_m.append(0.0)
            continue
        precision, recall = float(len(matches)) / m, float(len(matches)) / len(ref)
        fmean = (precision * recall) / (alpha * precision + (1 - alpha) * recall)
        frag_frac = float(count_chunks(matches)) / len(matches)
        by_m.append((1 - gamma * frag_frac ** beta) * fmean)
    return np.array([by_m[c] for c in counts], dtype=np.float64)


def rewards_row(scores):
    """the float32 `rewards` row the reference stores"""
    return np.asarray(scores, dtype=np.float64).astype(np.float32)


def delta_row(scores):
    """column 0: the fp32 score; then the differences of the fp32 scores, in fp32"""
    return _delta_row(rewards_row(scores))


# ---- the random cases tests/test_meteor_cpu.py (coverage) and tests/test_meteor_gpu.py (device against this file) share
STEMS = {"walks": "walk", "walked": "walk", "walking": "walk", "walker": "walk", "jumps": "jump", "jumped": "jump",
         "plays": "play", "playing": "play", "played": "play", "dogs": "dog", "cats": "cat", "running": "run", "runs": "run"}
# asymmetric on purpose: the set belongs to the hypothesis word.  "great", "swift" and "feline" are in no vocab entry.
SYNONYMS = {"big": ["large", "huge", "great"], "large": ["big"], "huge": ["big", "large", "huge"],
            "small": ["little", "tiny"], "little": ["small"], "fast": ["quick", "rapid", "swift"], "quick": ["fast"],
            "cat": ["feline"], "walk": ["stroll", "walk"], "man": []}


class DictStemmer:
    def __init__(self, stems=None):
        self.stems = STEMS if stems is None else stems

    def stem(self, word):
        return self.stems.get(word, word)


def dict_synonyms(word):
    return SYNONYMS.get(word, [])


def case_vocab():
    """about 40 entries: specials, "" and " ", stem clusters, synonym clusters, upper-case entries"""
    words = ["a", "the", "on", "in", "dog", "dogs", "cat", "cats", "man", "walk", "walks", "walked", "walking", "jump",
             "jumps", "jumped", "play", "plays", "playing", "big", "large", "huge", "small", "little", "tiny", "fast",
             "quick", "rapid", "THE", "Dog", "Walking", "BIG", "and", "with"]
    return ["<unk>", "<pad>", "<s>", "</s>", " ", ""] + words


def random_case(seed, B=32, L=30, R_max=20):
    """(itos, captions, hyp (B, L) int64 numpy): reference lengths 0..R_max, words of the vocabulary (any case) and some
    outside it; about one token in twenty yields no word.  Every eighth caption is empty; every fifth is a shuffled-in-
    blocks copy of its hypothesis, so that long chunks occur."""
    rng = np.random.RandomState(seed)
    itos = case_vocab()
    V = len(itos)
    extra = ["walker", "played", "great", "swift", "feline", "running", "runs", "oov"]
    pool = [s.lower() for s in itos[6:]] + extra
    hyp = np.empty((B, L), dtype=np.int64)
    caps = []
    for b in range(B):
        for t in range(L):
            hyp[b, t] = rng.choice([4, 5, 1]) if rng.rand() < 0.05 else rng.randint(6, V)
        if b % 8 == 3:
            words = []
        elif b % 5 == 1:
            src = " ".join(itos[i] for i in hyp[b]).lower().split()
            cut = sorted(rng.choice(len(src), size=3, replace=False)) if len(src) > 3 else []
            blocks = np.split(np.arange(len(src)), cut)
            order = rng.permutation(len(blocks))
            words = [src[i] for k in order for i in blocks[k]][:R_max]
        else:
            words = [pool[rng.randint(len(pool))] for _ in range(rng.randint(0, R_max + 1))]
        caps.append(" ".join(w.upper() if rng.rand() < 0.1 else w for w in words))
    return itos, caps, hyp


def coverage(itos, caps, hyp, stem, syn):
    """what the cases exercise, by this restatement: matches per stage, the largest chunk count, empty references, and
    the number of (row, prefix) pairs where a word is matched to another reference position than in the next prefix"""
    stages, max_chunks, empty, disagree = [0, 0, 0], 0, 0, 0
    for b, row in enumerate(hyp.tolist()):
        ref = caps[b].lower().split()
        empty += not ref
        words = " ".join(itos[i] for i in row).lower().split()
        prev = None
        for m in range(1, len(words) + 1):
            matches, counts = align(words[:m], ref, stem, syn)
            cur = dict(matches)
            if prev is not None:
                disagree += any(h in cur and cur[h] != j for h, j in prev.items())
            prev = cur
            if m == len(words):
                stages = [a + c for a, c in zip(stages, counts)]
            if matches:
                max_chunks = max(max_chunks, count_chunks(matches))
    return {"stages": stages, "max_chunks": max_chunks, "empty": empty, "disagree": disagree}
