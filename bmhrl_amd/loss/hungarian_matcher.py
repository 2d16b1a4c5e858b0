"""HungarianMatcher with the reference's contract (loss/hungarian_matcher.py:5-59) and the word loss that consumes it
(`loss_labels`, epoch_loops/captioning_bmrl_loops.py:1114-1129), on the device (csrc/word_loss.hip).

The reference takes a softmax over (B * Q, C), copies the cost matrix to the host, runs scipy's linear_sum_assignment per
sample and scores the class map with F.cross_entropy.  Here the cost pass, the assignment, the class map, the weighted mean
and its gradient are four launches and nothing leaves the device: `HungarianMatcher.match` and `loss_labels(outputs,
targets)` never synchronise.  `HungarianMatcher.forward` returns what the reference returns -- a list of (index_i,
index_j) int64 CPU tensors, index_i ascending as scipy orders them -- and pays one copy at the end for it.

`targets` is the (B, L) int64 caption tensor the reference's loop passes (train_detr, :1045), or a list of 1-D id tensors.
Entries equal to pad_idx are no words, wherever they sit; the reference hard-codes 1, the default here.  One rule is added:
an id outside [0, C - 2] is dropped like a pad (the reference would index out of range or match the "no word" class).
Where several assignments have the same total cost the two implementations may pick different ones; both are optimal.
Limits (include/bmhrl_hip.h): Q <= 128 queries, L <= 64 caption positions, L <= Q."""
import torch
import torch.nn as nn

from .. import ops
from ..functional import DetrWordLossFn


def _captions(targets, pad_idx, device):
    """(B, L) int64 on `device`: the caption tensor itself, or a list of 1-D id tensors padded with pad_idx"""
    if torch.is_tensor(targets):
        cap = targets
    else:
        cap = torch.nn.utils.rnn.pad_sequence([t.reshape(-1) for t in targets], batch_first=True, padding_value=pad_idx)
    if cap.dim() != 2:
        raise ValueError("targets: a (B, L) tensor of token ids or a list of 1-D tensors expected")
    return cap.to(device=device, dtype=torch.int64)


class HungarianMatcher(nn.Module):

    def __init__(self, cost_class: float = 1, pad_idx: int = 1):
        super().__init__()
        self.cost_class = cost_class
        self.pad_idx = pad_idx

    @torch.no_grad()
    def match(self, outputs, targets, eos_coef=0.1):
        """sync-free device form: (tgt_class (B, Q) int32 -- the matched word or C - 1, query_of_target (B, L) int32 -- the
        query of word j of the compacted caption or -1, n_words (B) int32)"""
        cap = _captions(targets, self.pad_idx, outputs.device)
        x = outputs.detach().float()
        words, n_words, lse, x_none, gathered, cost = ops.word_cost(x.contiguous(), cap, self.pad_idx, self.cost_class)
        qot = ops.lsa_match(cost, n_words)
        tgt_class, _, _ = ops.word_loss(words, n_words, qot, lse, x_none, gathered, eos_coef, x.shape[2])
        return tgt_class, qot, n_words

    @torch.no_grad()
    def forward(self, outputs, targets):
        _, qot, n_words = self.match(outputs, targets)
        host = torch.cat([qot, n_words.unsqueeze(1)], 1).cpu().to(torch.int64)          # the one copy
        res = []
        for row in host:
            q = row[:int(row[-1])]
            order = torch.argsort(q)
            res.append((q[order], order))
        return res


def _query_of_target(indices, B, L, device):
    """the reference's list of (index_i, index_j) as the (B, L) int32 map the kernels read"""
    qot = torch.full((B, L), -1, dtype=torch.int32)
    if len(indices) != B:
        raise ValueError(f"indices: one (index_i, index_j) pair per sample expected, got {len(indices)} for {B} samples")
    for b, (i, j) in enumerate(indices):
        i, j = torch.as_tensor(i).reshape(-1).cpu(), torch.as_tensor(j).reshape(-1).cpu().long()
        if i.numel() != j.numel() or (j.numel() and (int(j.min()) < 0 or int(j.max()) >= L)):
            raise ValueError("indices: index_i and index_j must pair up, index_j within the caption")
        qot[b, j] = i.to(torch.int32)
    return qot.to(device)


def loss_labels(outputs, targets, indices=None, eos_coef=0.1, pad_idx=1, cost_class=1.0):
    """The classification loss of the DETR word head: cross entropy of outputs (B, Q, C) against the matched words, "no
    word" (C - 1) for the unmatched queries at weight eos_coef; weighted mean as F.cross_entropy forms it.  indices=None
    matches and scores in one call, without a host synchronisation; the reference's list of tuples scores that matching."""
    cap = _captions(targets, pad_idx, outputs.device)
    qot = None if indices is None else _query_of_target(indices, cap.shape[0], cap.shape[1], outputs.device)
    return DetrWordLossFn.apply(outputs, cap, int(pad_idx), float(eos_coef), float(cost_class), qot)
