"""Training the segment critic with this package: CriticTrainer and segment_examples.

The agent only reads its SegmentCritic (LSTM(4) -> AReLU -> GRU(2) -> AReLU -> Linear): `cfg.rl_critic_path` names a
state dict, and without one the labels that drive the manager's goals come from a random initialisation.  This module
produces that file: build a standalone `SegmentCritic(cfg)`, train it with `CriticTrainer` on (tokens, 0/1 segment
labels) and `save()` it.  The step runs eagerly on the HIP kernels of csrc/critic_train.hip (functional.SegmentCriticFn);
the optimiser is torch.optim.Adam.

Train a standalone critic.  An agent's own `critic` must not be unfrozen while a CaptionTrainer holds the agent: the
trainer builds its flat parameter bucket from `requires_grad`.
"""
from __future__ import annotations

import json
import os

import torch


def segment_examples(records, stoi, start_token, end_token, pad_token, unk_idx, max_len):
    """(tokens int64 (N, max_len + 1), labels fp32 (N, max_len + 1)) from segment-labelled captions.

    records: an iterable of {"captions": [str], "seg_labels": [[0/1 per word]]}, or the path of a JSON file holding one.
    Per caption: words = caption.split() with the last word replaced by end_token; the sequence is [start_token, *words]
    and its labels [0, *seg_labels]; words missing from `stoi` map to unk_idx; longer sequences are cut to max_len + 1,
    shorter ones padded with stoi[pad_token] and label 0.  A caption whose label count differs from its word count raises
    ValueError."""
    if isinstance(records, (str, os.PathLike)):
        with open(records) as f:
            records = json.load(f)
    width = max_len + 1
    pad = stoi[pad_token]
    tokens, labels = [], []
    for rec in records:
        if len(rec["captions"]) != len(rec["seg_labels"]):
            raise ValueError(f"record has {len(rec['captions'])} captions and {len(rec['seg_labels'])} label lists")
        for caption, segs in zip(rec["captions"], rec["seg_labels"]):
            words = caption.split()
            if len(words) != len(segs) or not words:
                raise ValueError(f"caption {caption!r}: {len(words)} words but {len(segs)} segment labels")
            words[-1] = end_token
            ids = [stoi.get(w, unk_idx) for w in [start_token] + words][:width]
            lab = ([0.0] + [float(s) for s in segs])[:width]
            tokens.append(ids + [pad] * (width - len(ids)))
            labels.append(lab + [0.0] * (width - len(lab)))
    return (torch.tensor(tokens, dtype=torch.int64).reshape(-1, width),
            torch.tensor(labels, dtype=torch.float32).reshape(-1, width))


class CriticTrainer:
    """Trains a standalone SegmentCritic on (tokens (B, L) int64, labels (B, L) 0/1) with the masked, positively weighted
    BCE-with-logits; mask = tokens != pad_idx.

    embed: a VocabularyEmbedder or any callable tokens (B, L) -> (B, L, d_caps) fp32 on the device, called under no_grad
    (the input the agent gives its critic: emb_C(trg)).  pos_weight None = 1.  grad_clip: max gradient norm, or None."""

    def __init__(self, critic, embed, pad_idx, lr=1e-3, pos_weight=None, grad_clip=None):
        if not callable(embed):
            raise TypeError("embed must be callable: tokens (B, L) -> (B, L, d_caps)")
        if critic.lstm.input_size % 4 != 0:
            raise ValueError(f"d_caps = {critic.lstm.input_size} must be a multiple of 4 (16-byte rows of the fp32 kernels)")
        if lr <= 0:
            raise ValueError("lr must be positive")
        if pos_weight is not None and pos_weight <= 0:
            raise ValueError("pos_weight must be positive")
        if grad_clip is not None and grad_clip <= 0:
            raise ValueError("grad_clip must be positive")
        self.critic = critic
        self.embed = embed
        self.pad_idx = int(pad_idx)
        self.pos_weight = 1.0 if pos_weight is None else float(pos_weight)
        self.grad_clip = grad_clip
        critic.unfreeze()
        self.optimizer = torch.optim.Adam(critic.parameters(), lr=lr)

    def _loss(self, tokens, labels):
        with torch.no_grad():
            emb = self.embed(tokens)
        return self.critic.masked_bce(emb.float(), labels, tokens != self.pad_idx, self.pos_weight)[0]

    def step(self, tokens, labels):
        """one optimiser step; returns the loss as a 0-dim device tensor (no host synchronisation)"""
        self.optimizer.zero_grad(set_to_none=True)
        loss = self._loss(tokens, labels)
        loss.backward()
        if self.grad_clip is not None:
            torch.nn.utils.clip_grad_norm_(self.critic.parameters(), self.grad_clip)
        self.optimizer.step()
        return loss.detach()

    def fit(self, tokens, labels, epochs, batch_size, seed=0):
        """`epochs` passes over the examples in batches shuffled by a generator seeded with `seed`; returns the mean loss of
        each epoch (host floats: one synchronisation per epoch)"""
        n = tokens.shape[0]
        gen = torch.Generator().manual_seed(seed)
        means = []
        for _ in range(epochs):
            order = torch.randperm(n, generator=gen).to(tokens.device)
            losses = [self.step(tokens[idx], labels[idx]) for idx in order.split(batch_size)]
            means.append(float(torch.stack(losses).mean()))
        return means

    def evaluate(self, tokens, labels, threshold=0.5):
        """loss, and precision / recall / f1 of the labels of score_and_labels (the inference path the agent uses) over the
        non-pad positions"""
        with torch.no_grad():
            loss = self._loss(tokens, labels)
            pred = self.critic.score_and_labels(self.embed(tokens).float(), threshold)[1].bool()
        valid = tokens != self.pad_idx
        truth = labels > 0.5
        tp = float((pred & truth & valid).sum())
        fp = float((pred & ~truth & valid).sum())
        fn = float((~pred & truth & valid).sum())
        precision = tp / (tp + fp) if tp + fp else 0.0
        recall = tp / (tp + fn) if tp + fn else 0.0
        f1 = 2 * precision * recall / (precision + recall) if precision + recall else 0.0
        return {"loss": float(loss), "precision": precision, "recall": recall, "f1": f1}

    def save(self, path):
        """the critic's state dict (the reference's keys): usable as cfg.rl_critic_path here and in the reference"""
        torch.save(self.critic.state_dict(), path)

    def close(self):
        """freeze the critic again"""
        self.critic.freeze()
