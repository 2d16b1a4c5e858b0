"""Oracle of the critic-training tests: the segment critic from torch's own nn.LSTM / nn.GRU / nn.Linear plus the
three-line AReLU, on the CPU, in the dtype asked for (float64 = the oracle, float32 = the yardstick of the rounding
error).  Loss: F.binary_cross_entropy_with_logits(pos_weight=, reduction='none') * mask, summed, over sum(mask).
Gradients come from torch autograd.  Nothing here touches the package under test."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F


class _AReLU(nn.Module):
    def __init__(self):
        super().__init__()
        self.alpha = nn.Parameter(torch.tensor([0.90]))
        self.beta = nn.Parameter(torch.tensor([2.0]))

    def forward(self, x):
        return F.relu(x) * (1 + torch.sigmoid(self.beta)) - F.relu(-x) * torch.clamp(self.alpha, min=0.01, max=0.99)


class CriticRef(nn.Module):
    """same attribute names as SegmentCritic, so its state dict loads here key for key"""

    def __init__(self, d):
        super().__init__()
        self.lstm = nn.LSTM(d, 2 * d, num_layers=4, batch_first=True)
        self.gru = nn.GRU(2 * d, 2 * d, num_layers=2, batch_first=True)
        self.lin = nn.Linear(2 * d, 1)
        self.relu = _AReLU()
        self.relu2 = _AReLU()

    def forward(self, emb):
        h, _ = self.lstm(emb)
        h, _ = self.gru(self.relu(h))
        return self.lin(self.relu2(h))


PARAM_NAMES = [n for n, _ in CriticRef(4).named_parameters()]


def masked_bce(score, labels, mask, pos_weight):
    pw = None if pos_weight is None else torch.tensor(float(pos_weight), dtype=score.dtype)
    l = F.binary_cross_entropy_with_logits(score.squeeze(-1), labels.to(score.dtype), pos_weight=pw, reduction="none")
    m = mask.to(score.dtype)
    return (l * m).sum() / m.sum()


def closed_form_bce(score, labels, mask, pos_weight):
    """l = (1 - y) s + (1 + (pw - 1) y) (log1p(exp(-|s|)) + max(-s, 0)); sum(mask l) / sum(mask)"""
    s, y, m = score.squeeze(-1), labels.to(score.dtype), mask.to(score.dtype)
    pw = 1.0 if pos_weight is None else float(pos_weight)
    l = (1 - y) * s + (1 + (pw - 1) * y) * (torch.log1p(torch.exp(-s.abs())) + torch.clamp(-s, min=0))
    return (l * m).sum() / m.sum()


def random_state(d, seed):
    """weights uniform in +-3/sqrt(H) (no layer's gradient vanishes), AReLU parameters at their defaults"""
    g = torch.Generator().manual_seed(seed)
    ref = CriticRef(d)
    k = 3.0 / math.sqrt(2 * d)
    sd = {}
    for n, p in ref.state_dict().items():
        sd[n] = p.clone() if n.startswith("relu") else (torch.rand(p.shape, generator=g) * 2 - 1) * k
    return sd


def random_case(d, B, L, seed, pad_idx=1):
    """emb ~ 3 N(0, 1); tokens with about 20 % pad positions (column 0 always valid); 0/1 labels"""
    g = torch.Generator().manual_seed(1000 + seed)
    emb = 3.0 * torch.randn(B, L, d, generator=g)
    tokens = torch.randint(2, 20, (B, L), generator=g)
    pad = torch.rand(B, L, generator=g) < 0.2
    pad[:, 0] = False
    tokens[pad] = pad_idx
    labels = (torch.rand(B, L, generator=g) < 0.4).float()
    return emb, tokens, labels


def loss_and_grads(state, emb, labels, mask, pos_weight, dtype, emb_grad=False):
    """(loss, score, {name: grad}) of the oracle in `dtype` on the CPU; the dict has key "emb" when emb_grad"""
    d = emb.shape[-1]
    ref = CriticRef(d).to(dtype)
    ref.load_state_dict({k: v.detach().cpu().to(dtype) for k, v in state.items()})
    x = emb.detach().cpu().to(dtype).requires_grad_(emb_grad)
    score = ref(x)
    loss = masked_bce(score, labels.cpu(), mask.cpu(), pos_weight)
    loss.backward()
    grads = {n: p.grad.detach() for n, p in ref.named_parameters()}
    if emb_grad:
        grads["emb"] = x.grad.detach()
    return loss.detach(), score.detach(), grads


def rel_err(g, g64):
    """max |g - g64| / max |g64| (0 / 0 = 0: a gradient that is exactly zero must be exactly zero)"""
    num = float((g.detach().cpu().double() - g64.double()).abs().max())
    den = float(g64.double().abs().max())
    return 0.0 if num == 0.0 else (num / den if den > 0 else float("inf"))
