"""Device-side CIDEr and BLEU rewards for the RL steps: drop-in replacements of the reference's metrics/cider.py
CiderScorer and metrics/bleu.py BleuScorer whose per-prefix scoring (every prefix of every sampled caption, on the host)
runs as one HIP launch (csrc/rewards.hip, bmhrl_rewards).  The discounting and segment sums reuse rl_glue.

Strings never reach the device.  At construction one string -> id table is built from the vocabulary (every `itos`
entry, raw and lowercased) and, for CIDEr, the corpus (`dictionary`: the dataset's tokenized captions).  A vocab entry
maps to the id of its one word (CIDEr: `itos` as it is, BLEU: lowercased), to -1 when it splits into no word (its
position still gets a prefix score), and is refused when it splits into more.  Reference captions are lowercased and
split on the host by bind(); their words outside the table get fresh ids for that batch.  CIDEr's document frequencies
(precook_corpus: n-grams of lengths 1..4 counted over the corpus, kept when the count is above 1) live in an
open-addressing hash table on the device, keyed by 4 word ids, with log(df) precomputed here.

Graph-safe use: scorer.bind(captions) copies the batch's reference word ids into a fixed device buffer (one non-blocking
host -> device copy, no read-back); CaptionTrainer(phase="worker", reward_fn=scorer.reward_fn()) captures the reward
launch in the step graph, and bind(batch["captions"]) before each replay() refreshes it.

METEOR (MeteorScorer, csrc/meteor.hip, bmhrl_meteor): stemming and synonym lookup depend on the
vocabulary alone, so they become tables built here once (MeteorTables: vocab id -> stem id, and the synonym sets as CSR rows
of word ids); the reference buffer then carries a row of stem ids beside the row of word ids.

install() registers metrics.cider and metrics.bleu in sys.modules so that the reference's driver imports these classes;
install(meteor=True) also metrics.batched_meteor.
"""
from __future__ import annotations

import importlib
import sys
import types
from typing import Dict, Iterable, List, Sequence, Tuple

import numpy as np
import torch

from . import ops, rl_glue

Tensor = torch.Tensor
EOS = "</s>"
_HASH_MUL = np.array([0x9E3779B1, 0x85EBCA77, 0xC2B2AE3D, 0x27D4EB2F], dtype=np.uint32)


def _hash(keys: np.ndarray) -> np.ndarray:
    """uint32 hash of (N, 4) int32 keys; csrc/rewards.hip gram_hash computes the same"""
    k = keys.astype(np.int64).astype(np.uint32)
    h = (k[:, 0] * _HASH_MUL[0]) ^ (k[:, 1] * _HASH_MUL[1]) ^ (k[:, 2] * _HASH_MUL[2]) ^ (k[:, 3] * _HASH_MUL[3])
    h = h ^ (h >> np.uint32(15))
    h = h * np.uint32(0x2C1B3C6D)
    return h ^ (h >> np.uint32(12))


class StringTable:
    """string -> int id; ids are dense from 0 in insertion order"""

    def __init__(self):
        self.ids: Dict[str, int] = {}

    def add(self, s: str) -> int:
        i = self.ids.get(s)
        if i is None:
            i = self.ids[s] = len(self.ids)
        return i

    def __len__(self):
        return len(self.ids)

    def __getitem__(self, s: str) -> int:
        return self.ids[s]

    def get(self, s: str, default=None):
        return self.ids.get(s, default)


def vocab_word_ids(itos: Sequence[str], table: StringTable, lower: bool) -> np.ndarray:
    """(V,) int32: the table id of each entry's one word (-1: no word).  An entry of two or more words -> ValueError."""
    out = np.full(len(itos), -1, dtype=np.int32)
    for i, s in enumerate(itos):
        words = (s.lower() if lower else s).split()
        if len(words) > 1:
            raise ValueError(f"vocab entry {i} ({s!r}) splits into {len(words)} words; a token must yield at most one")
        if words:
            out[i] = table[words[0]]
    return out


def vocab_strings(itos: Sequence[str]) -> StringTable:
    """the string table of a vocabulary: every entry, raw and lowercased, then the words the vocab maps point at"""
    table = StringTable()
    for s in itos:
        table.add(s)
        table.add(s.lower())
    for s in itos:
        for w in s.split() + s.lower().split():
            table.add(w)
    return table


class DocFrequency:
    """precook_corpus of metrics/cider.py as a hash table: keys (cap, 4) int32 word ids (-1 behind the gram, key[0] = -1:
    empty slot), logs (cap,) fp64 = log(df) of the grams counted more than once, cap a power of two >= 2 * entries."""

    def __init__(self, caps: Iterable, table: StringTable, n: int = 4):
        rows, lens = [], []
        for cap in caps:
            toks = list(cap)                  # as precook_corpus slices it (a string caption gives characters)
            rows.append(toks)
            lens.append(len(toks))
        flat = [table.add(w) for toks in rows for w in toks]
        words = np.asarray(flat, dtype=np.int32)
        lens = np.asarray(lens, dtype=np.int64)
        starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64) if len(lens) else np.zeros(0, np.int64)
        cap_of = np.repeat(np.arange(len(lens)), lens)
        pos_in = np.arange(words.size, dtype=np.int64) - (starts[cap_of] if words.size else 0)
        keys = []
        for k in range(1, n + 1):
            ok = pos_in + k <= lens[cap_of] if words.size else np.zeros(0, bool)
            idx = np.nonzero(ok)[0]
            key = np.full((idx.size, 4), -1, dtype=np.int32)
            for q in range(k):
                key[:, q] = words[idx + q]
            keys.append(key)
        allk = np.concatenate(keys) if keys else np.zeros((0, 4), np.int32)
        uniq, counts = np.unique(allk, axis=0, return_counts=True)
        keep = counts > 1
        self.grams, self.counts = uniq[keep], counts[keep]
        # log(max(1, df)) as the reference evaluates it (np.log of one count at a time)
        vals, inv = np.unique(self.counts, return_inverse=True)
        self.log_df = np.array([np.log(float(c)) for c in vals], dtype=np.float64)[inv.reshape(-1)] if vals.size else \
            np.zeros(0, np.float64)
        N = self.grams.shape[0]
        cap = 2
        while cap < 2 * N:
            cap *= 2
        self.cap = cap
        self.keys = np.full((cap, 4), -1, dtype=np.int32)
        self.logs = np.zeros(cap, dtype=np.float64)
        mask = cap - 1
        slot = (_hash(self.grams).astype(np.int64) & mask) if N else np.zeros(0, np.int64)
        pending = np.arange(N)
        owner = np.full(cap, -1, dtype=np.int64)
        while pending.size:                   # linear probing, one probe step for every unplaced key per round
            s = slot[pending]
            free = owner[s] < 0
            cand, cs = pending[free], s[free]
            won_slots, first = np.unique(cs, return_index=True)
            owner[won_slots] = cand[first]
            placed = np.zeros(N, bool)
            placed[cand[first]] = True
            pending = pending[~placed[pending]]
            slot[pending] = (slot[pending] + 1) & mask
        used = owner >= 0
        self.keys[used] = self.grams[owner[used]]
        self.logs[used] = self.log_df[owner[used]]

    def lookup(self, gram: Sequence[int]) -> float:
        """log(max(1, df)) of a gram of word ids (host twin of the device probe; 0 for grams not in the table)"""
        key = np.full((1, 4), -1, dtype=np.int32)
        key[0, :len(gram)] = gram
        mask = self.cap - 1
        s = int(_hash(key)[0]) & mask
        for _ in range(self.cap):
            if self.keys[s, 0] == -1:
                return 0.0
            if tuple(self.keys[s]) == tuple(key[0]):
                return float(self.logs[s])
            s = (s + 1) & mask
        return 0.0


class _DeviceScorer:
    """what CiderScorer and BleuScorer share: the string table, the vocab maps, the bound reference buffer, the launch"""
    metric = None

    def __init__(self, vocab, device, gamma, gamma_manager, n, sigma, dictionary=None):
        assert (n <= 4 and n > 0)
        self.counter = 0
        self.vocab = vocab
        self.device = torch.device(device)
        self._n = n
        self._sigma = sigma
        self.gamma = gamma
        self.gamma_m = gamma_manager
        itos = list(vocab.itos)
        self.strings = vocab_strings(itos)
        self.df = DocFrequency(dictionary, self.strings) if dictionary is not None else None
        cider = self.metric == ops.REWARD_CIDER
        vmap = vocab_word_ids(itos, self.strings, lower=not cider)
        eos = [i for i, s in enumerate(itos) if s == EOS] if cider else []
        if len(eos) > 1:
            raise ValueError(f"vocab holds {EOS!r} more than once (ids {eos})")
        self.eos = eos[0] if eos else -1
        self.vmap = torch.from_numpy(vmap).to(self.device)
        if self.df is not None:
            self.df_keys = torch.from_numpy(self.df.keys).to(self.device)
            self.df_logs = torch.from_numpy(self.df.logs).to(self.device)
        else:
            self.df_keys = self.df_logs = None
        self._ref = None                      # encode()'s planes of (capacity rows, R) int32 ids, then capacity ref_len words
        self._ref_host = None
        self._copied = None                   # event of the last host -> device copy out of _ref_host
        self._bound = 0

    # ---- host: reference captions -> word ids
    def tokenize(self, captions: Sequence[str]) -> List[List[int]]:
        """lowercased, whitespace-split word ids of every caption; words outside the table get fresh ids (this batch)"""
        fresh: Dict[str, int] = {}
        out = []
        for c in captions:
            ids = []
            for w in c.lower().split():
                i = self.strings.get(w)
                if i is None:
                    i = fresh.setdefault(w, len(self.strings) + len(fresh))
                ids.append(i)
            if len(ids) > ops.REWARDS_MAX_R:
                raise ValueError(f"reference caption of {len(ids)} words; at most {ops.REWARDS_MAX_R} are supported")
            out.append(ids)
        return out

    def encode(self, captions: Sequence[str]) -> List[List[List[int]]]:
        """the id rows a caption puts into the reference buffer, plane by plane (here one plane: the word ids)"""
        return [self.tokenize(captions)]

    def bind(self, captions: Sequence[str]) -> None:
        """tokenize the batch's reference captions and copy their word ids into the fixed device buffer (one non-blocking
        copy on the current stream, no read-back).  The buffer keeps its address while the batch size does not grow, so a
        captured reward launch reads the newly bound captions at its next replay."""
        planes = self.encode(captions)
        P, B, R = len(planes), len(planes[0]), ops.REWARDS_MAX_R
        if B == 0:
            raise ValueError("bind: no captions")
        if self._ref is None or self._ref_rows < B:
            self._ref_rows = B
            self._ref = torch.empty(P * B * R + B, dtype=torch.int32, device=self.device)
            self._ref_host = torch.empty(P * B * R + B, dtype=torch.int32, pin_memory=True)
            self._copied = None
        if self._copied is not None:
            self._copied.synchronize()        # the previous copy out of the staging buffer has finished
        rows = self._ref_rows
        host = self._ref_host.numpy()
        words, lens = host[:P * rows * R].reshape(P, rows, R), host[P * rows * R:]
        lens[:] = 0
        for p, ids in enumerate(planes):
            for b, w in enumerate(ids):
                words[p, b, :len(w)] = w
                lens[b] = len(w)
        self._ref.copy_(self._ref_host, non_blocking=True)
        self._copied = torch.cuda.Event()
        self._copied.record()
        self._bound = B

    def bound(self) -> Tuple[Tensor, Tensor]:
        """views of the device buffer: ref (planes, capacity rows, R) int32 ids and ref_len (capacity rows) int32"""
        rows, R = self._ref_rows, ops.REWARDS_MAX_R
        return self._ref[:-rows].view(-1, rows, R), self._ref[-rows:]

    def _launch(self, pred: Tensor) -> Tuple[Tensor, Tensor]:
        """(delta (B, L) fp32, scores (B, L) fp64) of the sampled tokens against the bound captions"""
        B, L = pred.shape
        if self._bound < B:
            raise ValueError(f"{B} sampled captions but {self._bound} reference captions bound")
        if L > ops.REWARDS_MAX_L:
            raise ValueError(f"captions of {L} tokens; at most {ops.REWARDS_MAX_L} are supported")
        hyp = pred if (pred.dtype == torch.int64 and pred.stride(1) == 1) else pred.long().contiguous()
        ref, ref_len = self.bound()
        scores = torch.empty(B, L, dtype=torch.float64, device=self.device)
        delta = torch.empty(B, L, dtype=torch.float32, device=self.device)
        self._score(hyp, ref, ref_len, scores, delta)
        return delta, scores

    def _score(self, hyp, ref, ref_len, scores, delta):
        """the launch: ref (planes, rows, R) as encode() laid it out"""
        ops.rewards(hyp, self.vmap, self.eos, ref[0], ref_len, self.df_keys, self.df_logs, self.metric, self._n, self._sigma,
                    scores, delta)

    def _diff(self, pred, target):
        if target is not None:
            self.bind(list(target[:pred.shape[0]]))
        delta, scores = self._launch(pred)
        self.counter += 1
        return delta, scores

    def prefix_scores(self, pred, captions: Sequence[str]) -> Tensor:
        """the fp64 per-prefix score table (rows, L) of the token rows pred (rows, L) against `captions`, one reference per
        row (bound first).  Every scorer built on this class has it, the METEOR scorer included (its encode / _score)."""
        if isinstance(captions, str):
            raise TypeError("prefix_scores: captions must be a sequence of strings, one per row")
        self.bind(list(captions))
        return self._launch(pred)[1]

    def reward_fn(self):
        """(sampled (B, L), captions) -> (B, L) fp32 discounted worker reward, as delta_*_worker.  captions: a list of
        strings (bound first) or None (the last bound captions: CaptionTrainer._rl_loss passes None).  Graph-safe: the
        discount matrix is built at the first (eager) call and reused."""
        cache = {}

        def fn(sampled, captions=None):
            if captions is not None:
                if isinstance(captions, str) or not isinstance(captions, (list, tuple)):
                    raise TypeError("reward_fn: captions must be a list of strings or None")
                self.bind(list(captions))
            delta, _ = self._launch(sampled)
            L = sampled.shape[1]
            w = cache.get(L)
            if w is None:
                w = cache[L] = rl_glue.discount_matrix(L, self.gamma, device=self.device)
            return delta @ w.t()
        return fn


class CiderScorer(_DeviceScorer):
    """metrics/cider.py CiderScorer on the device (same constructor, .type, methods and results)"""
    metric = ops.REWARD_CIDER

    def __init__(self, vocab, dictionary, device, gamma, gamma_manager, n=4, sigma=6.0,):
        super().__init__(vocab, device, gamma, gamma_manager, n, sigma, dictionary=dictionary)
        self.type = "CIDER"

    def _cider_diff(self, pred, target):
        return self._diff(pred, target)

    def delta_cider_manager(self, pred, trg, mask, sections):
        """writes the end of every caption into the caller's sections (index len(trg[i].split()): IndexError past L)"""
        _mark_caption_ends(sections, trg, pred.shape[0])
        manager_segment_score, _ = self.delta_cider(pred, trg, mask, sections)
        return manager_segment_score.float(), None

    def delta_cider_worker(self, pred, trg):
        delta_cider_step_reward, rewards = self.delta_cider_step(pred, trg, self.gamma)
        return delta_cider_step_reward.float(), rewards

    def delta_cider(self, pred, trg, mask, sections):
        delta_cider_step_reward, rewards = self.delta_cider_step(pred, trg, self.gamma)
        delta_cider_section_reward, _ = self.delta_cider_segment(delta_cider_step_reward, sections, self.gamma)
        return delta_cider_section_reward, rewards

    def delta_cider_segment(self, delta_cider_step_reward, sections, gamma):
        segment_cider_dif, segment_reward_index = rl_glue.segment_reward(delta_cider_step_reward, sections)
        return rl_glue.discontinue_reward(segment_cider_dif, gamma, segments=sections), segment_reward_index

    def delta_cider_step(self, pred, tar, gamma):
        cider_diff, rewards = self._cider_diff(pred, tar)
        return rl_glue.discontinue_reward(cider_diff, gamma), rewards


class BleuScorer(_DeviceScorer):
    """metrics/bleu.py BleuScorer on the device (same constructor, .type, methods and results; `rewards` is fp32 as
    there)"""
    metric = ops.REWARD_BLEU

    def __init__(self, vocab, device, gamma, gamma_manager, n=4, sigma=6.0,):
        super().__init__(vocab, device, gamma, gamma_manager, n, sigma)
        self.type = "BLEU"

    def _bleu_diff(self, pred, target):
        delta, scores = self._diff(pred, target)
        return delta, scores.float()

    def delta_bleu_manager(self, pred, trg, mask, sections):
        manager_segment_score, _ = self.delta_bleu(pred, trg, mask, sections)
        return manager_segment_score.float(), None

    def delta_bleu_worker(self, pred, trg):
        delta_bleu_step_reward, rewards = self.delta_bleu_step(pred, trg, self.gamma)
        return delta_bleu_step_reward.float(), rewards

    def delta_bleu(self, pred, trg, mask, sections):
        delta_bleu_step_reward, rewards = self.delta_bleu_step(pred, trg, self.gamma)
        delta_bleu_section_reward, _ = self.delta_bleu_segment(delta_bleu_step_reward, sections, self.gamma)
        return delta_bleu_section_reward, rewards

    def delta_bleu_segment(self, delta_bleu_step_reward, sections, gamma):
        segment_bleu_dif, segment_reward_index = rl_glue.segment_reward(delta_bleu_step_reward, sections)
        return rl_glue.discontinue_reward(segment_bleu_dif, gamma), segment_reward_index    # no segments=: as the reference

    def delta_bleu_step(self, pred, tar, gamma):
        bleu_diff, rewards = self._bleu_diff(pred, tar)
        return rl_glue.discontinue_reward(bleu_diff, gamma), rewards


def _nltk_stemmer():
    from nltk.stem.porter import PorterStemmer
    return PorterStemmer()


def _nltk_synonyms():
    from nltk.corpus import wordnet

    def synonyms(word):
        """the lemma names without "_" of every synset of the word, as nltk's _enum_wordnetsyn_match collects them"""
        return [lemma.name() for synset in wordnet.synsets(word) for lemma in synset.lemmas() if lemma.name().find("_") < 0]
    return synonyms


class MeteorTables:
    """the host side of the METEOR scorer: what stemming and synonym lookup contribute, as tables over the vocabulary.
    strings / stems: the word and stem string tables; vmap (V,) int32 vocab id -> id of the entry's lowercased word (-1: no
    word); vstem (V,) int32 vocab id -> id of that word's stem (-1: no word; None: no stem stage); syn_off (V + 1,) /
    syn_ids int32: per vocab id the ascending, distinct word ids of synonyms(word) (None: no synonym stage).  A row holds
    the word itself only when `synonyms` returns it; the kernel counts the word itself as its own synonym either way.
    Every synonym is added to the word table, so a reference word that is one gets the same id.  syn_ids is never empty
    (one -1 stands in), so its device pointer is never null.

    stemmer: an object with .stem(str) -> str (None: nltk's PorterStemmer, False: no stem stage); synonyms: a callable
    word -> iterable of str (None: the WordNet lemma names, False: no synonym stage)."""

    def __init__(self, itos: Sequence[str], stemmer=None, synonyms=None, strings: StringTable = None):
        if stemmer is None or synonyms is None:
            try:
                stemmer = _nltk_stemmer() if stemmer is None else stemmer
                synonyms = _nltk_synonyms() if synonyms is None else synonyms
            except ImportError as e:
                raise ImportError("METEOR's default stemmer and synonyms come from nltk (PorterStemmer, WordNet), which cannot "
                                  "be imported; install it, or pass stemmer= (an object with .stem) and synonyms= (a callable "
                                  "word -> words); False switches the stage off") from e
        itos = list(itos)
        self.strings = strings if strings is not None else vocab_strings(itos)
        self.vmap = vocab_word_ids(itos, self.strings, lower=True)
        self._stem = stemmer.stem if stemmer is not False else None
        self._stem_cache: Dict[str, str] = {}
        self.stems = StringTable()
        words = [s.lower().split() for s in itos]
        self.vstem = None
        if self._stem is not None:
            self.vstem = np.full(len(itos), -1, dtype=np.int32)
            for i, w in enumerate(words):
                if w:
                    self.vstem[i] = self.stems.add(self.stem(w[0]))
        self.syn_off = self.syn_ids = None
        if synonyms is not False:
            rows = [sorted({self.strings.add(str(x)) for x in synonyms(w[0])}) if w else [] for w in words]
            self.syn_off = np.zeros(len(itos) + 1, dtype=np.int32)
            self.syn_off[1:] = np.cumsum([len(r) for r in rows])
            flat = [i for r in rows for i in r]
            self.syn_ids = np.asarray(flat if flat else [-1], dtype=np.int32)

    def stem(self, word: str) -> str:
        s = self._stem_cache.get(word)
        if s is None:
            s = self._stem_cache[word] = self._stem(word)
        return s

    def encode(self, captions: Sequence[str]) -> List[List[List[int]]]:
        """[word ids, stem ids] of every caption's lowercased, whitespace-split words; words and stems outside the tables
        get fresh ids (this batch).  Without a stem stage the stem ids are -1."""
        fresh_w: Dict[str, int] = {}
        fresh_s: Dict[str, int] = {}
        out_w, out_s = [], []
        for c in captions:
            ws, ss = [], []
            for w in c.lower().split():
                i = self.strings.get(w)
                if i is None:
                    i = fresh_w.setdefault(w, len(self.strings) + len(fresh_w))
                ws.append(i)
                j = -1
                if self._stem is not None:
                    s = self.stem(w)
                    j = self.stems.get(s)
                    if j is None:
                        j = fresh_s.setdefault(s, len(self.stems) + len(fresh_s))
                ss.append(j)
            if len(ws) > ops.REWARDS_MAX_R:
                raise ValueError(f"reference caption of {len(ws)} words; at most {ops.REWARDS_MAX_R} are supported")
            out_w.append(ws)
            out_s.append(ss)
        return [out_w, out_s]


class MeteorScorer(_DeviceScorer):
    """metrics/batched_meteor.py MeteorScorer on the device (its constructor arguments, .type, methods and results; the
    rules are in DESIGN.md section 19).  stemmer / synonyms: see MeteorTables."""
    type = "METEOR"
    alpha, beta, gamma_frag = 0.9, 3.0, 0.5       # single_meteor_score's defaults, which the reference uses

    def __init__(self, vocab, device, gamma_step, gamma_section, stemmer=None, synonyms=None):
        super().__init__(vocab, device, gamma_step, gamma_section, 4, 6.0)
        self.gamma_manager = gamma_section
        self.tables = MeteorTables(vocab.itos, stemmer, synonyms, strings=self.strings)
        dev = lambda a: None if a is None else torch.from_numpy(a).to(self.device)                       # noqa: E731
        self.vstem, self.syn_off, self.syn_ids = dev(self.tables.vstem), dev(self.tables.syn_off), dev(self.tables.syn_ids)

    def encode(self, captions):
        return self.tables.encode(captions)

    def _score(self, hyp, ref, ref_len, scores, delta):
        ops.meteor(hyp, self.vmap, self.vstem, self.syn_off, self.syn_ids, ref[0], ref[1] if self.vstem is not None else None,
                   ref_len, self.alpha, self.beta, self.gamma_frag, scores, delta)

    def _meteor_diff(self, pred, trg, mask=None):
        delta, scores = self._diff(pred, trg)
        return delta, scores.float()

    def delta_meteor_segment(self, delta_meteor_step_reward, sections, gamma):
        segment_meteor_dif, segment_reward_index = rl_glue.segment_reward(delta_meteor_step_reward, sections)
        return rl_glue.discontinue_reward(segment_meteor_dif, gamma), segment_reward_index

    def delta_meteor_step(self, pred, trg, mask, gamma):
        meteor_diff, rewards = self._meteor_diff(pred, trg, mask)
        return rl_glue.discontinue_reward(meteor_diff, gamma), rewards

    def delta_meteor_worker(self, pred, trg, mask=None):
        delta_meteor_step_reward, rewards = self.delta_meteor_step(pred, trg, mask, self.gamma)
        return delta_meteor_step_reward.float(), rewards

    def delta_meteor_manager(self, pred, trg, mask, sections):
        manager_segment_score, _ = self.delta_meteor(pred, trg, mask, sections)
        return manager_segment_score.float(), None

    def delta_meteor(self, pred, trg, mask, sections):
        delta_meteor_step_reward, rewards = self.delta_meteor_step(pred, trg, mask, self.gamma)
        delta_meteor_section_reward, _ = self.delta_meteor_segment(delta_meteor_step_reward, sections, self.gamma)
        return delta_meteor_section_reward, rewards

    def get_meteor_gamma(self, gamma, B, L):
        """(B, L, L): row i holds gamma^(k - i) at columns k >= i, zeros before"""
        return rl_glue.discount_matrix(L, gamma, n_step=L, device=self.device).expand(B, L, L).contiguous()


segment_reward = rl_glue.segment_reward       # metrics/batched_meteor.py exposes it (tests/golden/make_golden.py reads it there)


def _mark_caption_ends(sections: Tensor, trg: Sequence[str], B: int) -> None:
    """delta_cider_manager's in-place write: sections[i][e] = 1 and sections[i][e + 1:] = 0 with e = len(trg[i].split()),
    row by row; the row whose e is not a valid index raises IndexError after the rows before it were written"""
    L = sections.shape[1]
    ends = [len(trg[i].split()) for i in range(B)]
    bad = next((i for i, e in enumerate(ends) if e >= L), None)
    n_ok = B if bad is None else bad
    if n_ok:
        e = torch.tensor(ends[:n_ok], device=sections.device)[:, None]
        col = torch.arange(L, device=sections.device)[None, :]
        rows = sections[:n_ok]
        sections[:n_ok] = torch.where(col < e, rows, (col == e).to(sections.dtype))
    if bad is not None:
        raise IndexError(f"index {ends[bad]} is out of bounds for dimension 0 with size {L}")


def install(meteor: bool = False) -> List[str]:
    """register metrics.cider and metrics.bleu (the reference's scorer modules) as this module, so that the driver's
    `from metrics.cider import CiderScorer` gets the device scorers; meteor=True registers metrics.batched_meteor too
    (MeteorScorer, segment_reward).  Opt-in; bmhrl_amd.install does not do it."""
    if "metrics" not in sys.modules:
        try:
            importlib.import_module("metrics")           # the reference's package, when it is on sys.path
        except Exception:
            sys.modules["metrics"] = types.ModuleType("metrics")
            sys.modules["metrics"].__path__ = []
    mod = sys.modules[__name__]
    names = ["metrics.cider", "metrics.bleu"] + (["metrics.batched_meteor"] if meteor else [])
    for name in names:
        sys.modules[name] = mod
        setattr(sys.modules["metrics"], name.split(".")[1], mod)
    return names
