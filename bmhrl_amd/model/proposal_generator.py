"""MultimodalProposalGenerator: the temporal proposal generator the reference's proposal loops, data set and sample script
call (`from model.proposal_generator import MultimodalProposalGenerator`) but whose source is not part of the reference.

Nothing here can therefore be pinned to the reference.  It is written after the YOLO-style anchor heads of the reference's
parent project (Iashin & Rahtu, "A Better Use of Audio-Visual Cues: Dense Video Captioning with Bi-modal Transformer", BMVC
2020) to the contract the reference's loops call: `forward(feature_stacks, targets, masks)` returns `(predictions (B, N_total,
3), loss, losses_A, losses_V)`, `targets` are the (N, 4) rows `[video index in batch, centre s, length s, meta index]` of the
reference's proposal data set, and `model.anchors` is what `save_model` stores.  What IS pinned: the post-processing of the
predictions (bmhrl_amd.proposal_utils, tests/golden/proposals.json / .npz).

The bimodal encoder is the agent's (positional encoders + BMEncoder with the agent's cfg fields, as BMHrlAgent.encode_memory
runs them); each head is Conv1d(k, 'same') -> ReLU -> Dropout -> Conv1d(1) -> ReLU -> Dropout -> Conv1d(1) to 3 channels per
anchor, with the convolutions on the GEMM kernels (functional.Conv1dSameFn / LinearFn) and decode + loss + gradient of a head
in one launch (functional.ProposalLossFn, csrc/proposal.hip).  Padded positions are not masked in the loss, as the reference's
loops pass no mask to it.  A unimodal ProposalGenerator is outside the bimodal hot path, like the unimodal agents.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..functional import Conv1dSameFn, LinearFn, ProposalLossFn
from .blocks import PositionalEncoder
from .bm_hrl_agent import BMEncoder, _OutOfHotPath

LOSS_NAMES = ("loss_x", "loss_w", "loss_obj", "loss_noobj")


class ProposalGenerationHead(nn.Module):
    """(B, S, d_in) -> raw (B, S, 3 A): channel 3 a + {0, 1, 2} = (centre offset, log length factor, objectness logit) of
    anchor a.  The three nn.Conv1d modules hold the parameters under nn.Conv1d's names and shapes (a state dict loads into
    the same three layers of plain torch and back); the arithmetic runs on the HIP kernels."""

    def __init__(self, d_in, d_hidden, n_anchors, kernel_size, dout_p):
        super().__init__()
        if kernel_size % 2 != 1:
            raise ValueError("ProposalGenerationHead: kernel_size must be odd ('same' padding on both sides)")
        self.n_anchors, self.kernel_size, self.dout_p = n_anchors, kernel_size, dout_p
        self.conv1 = nn.Conv1d(d_in, d_hidden, kernel_size, padding=kernel_size // 2)
        self.conv2 = nn.Conv1d(d_hidden, d_hidden, 1)
        self.conv3 = nn.Conv1d(d_hidden, 3 * n_anchors, 1)

    @staticmethod
    def _pointwise(x, conv, relu, p):
        co, ci, _ = conv.weight.shape
        return LinearFn.apply(x, conv.weight.view(co, ci), conv.bias, relu, p)

    def forward(self, x):
        p = self.dout_p if self.training else 0.0
        if self.kernel_size == 1:
            h = self._pointwise(x, self.conv1, True, p)
        else:
            h = F.dropout(torch.relu(Conv1dSameFn.apply(x, self.conv1.weight, self.conv1.bias)), p, training=p > 0)
        h = self._pointwise(h, self.conv2, True, p)
        return self._pointwise(h, self.conv3, False, 0.0)


class MultimodalProposalGenerator(nn.Module):
    """cfg: the agent's encoder fields (d_vid, d_aud, d_model_video, d_model_audio, d_model, rl_ff_v, rl_ff_a, rl_att_heads,
    rl_att_layers, dout_p) and kernel_sizes = {"video": [...], "audio": [...]}, strides = {"video": seconds per video
    position, "audio": seconds per audio position}, conv_hidden, obj_coeff (1), noobj_coeff (100).
    anchors = {"video": [...], "audio": [...]}: anchor lengths in seconds (proposal_utils.anchors_from_segments), kept as
    buffers and, as given, in `self.anchors`."""

    def __init__(self, cfg, anchors):
        super().__init__()
        self.name = "multimodal_proposal_generator"
        self.anchors = {k: [float(a) for a in v] for k, v in anchors.items()}
        self.strides = {k: float(v) for k, v in cfg.strides.items()}
        self.kernel_sizes = {k: list(v) for k, v in cfg.kernel_sizes.items()}
        self.obj_coeff = float(getattr(cfg, "obj_coeff", 1.0))
        self.noobj_coeff = float(getattr(cfg, "noobj_coeff", 100.0))
        self.pos_enc_A = PositionalEncoder(cfg.d_model_audio, cfg.dout_p)
        self.pos_enc_V = PositionalEncoder(cfg.d_model_video, cfg.dout_p)
        self.bm_enc = BMEncoder(cfg.d_vid, cfg.d_aud, cfg.d_model, cfg.rl_ff_v, cfg.rl_ff_a, cfg.dout_p, cfg.rl_att_heads,
                                cfg.rl_att_layers)
        self.register_buffer("anchors_A", torch.tensor(self.anchors["audio"], dtype=torch.float32))
        self.register_buffer("anchors_V", torch.tensor(self.anchors["video"], dtype=torch.float32))
        self.heads_A = nn.ModuleList([ProposalGenerationHead(cfg.d_aud, cfg.conv_hidden, len(self.anchors["audio"]), k, cfg.dout_p)
                                      for k in self.kernel_sizes["audio"]])
        self.heads_V = nn.ModuleList([ProposalGenerationHead(cfg.d_vid, cfg.conv_hidden, len(self.anchors["video"]), k, cfg.dout_p)
                                      for k in self.kernel_sizes["video"]])

    def encode(self, feature_stacks, masks):
        """(Va, Av): the video and the audio stream out of the bimodal encoder, as BMHrlAgent.encode_memory"""
        rgb, flow = feature_stacks["rgb"], feature_stacks.get("flow")
        V = self.pos_enc_V(rgb, flow) if flow is not None else self.pos_enc_V(rgb)
        return self.bm_enc((V, self.pos_enc_A(feature_stacks["audio"])), masks)

    def forward(self, feature_stacks, targets, masks):
        Va, Av = self.encode(feature_stacks, masks)
        B, dev = Va.shape[0], Va.device
        groups = ((Av, self.heads_A, self.anchors_A, self.strides["audio"]), (Va, self.heads_V, self.anchors_V, self.strides["video"]))
        n_total = sum(len(heads) * anc.numel() * feat.shape[1] for feat, heads, anc, _ in groups)
        n_heads = len(self.heads_A) + len(self.heads_V)
        pred = torch.empty(B, n_total, 3, device=dev)
        if targets is not None:
            targets = targets.to(device=dev, dtype=torch.float32).contiguous()
            sums = torch.empty(n_heads, 5, device=dev)
        loss, row_off, h = 0, 0, 0
        for feat, heads, anc, cell_sec in groups:
            S, A = feat.shape[1], anc.numel()
            assigned = ops.proposal_assign(targets, anc, cell_sec, B, S) if targets is not None else None
            for head in heads:
                x = head(feat)
                if assigned is None:
                    ops.proposal_head(x.detach().float().contiguous(), anc, cell_sec, pred, row_off)
                else:
                    loss = loss + ProposalLossFn.apply(x, anc, cell_sec, pred, row_off, *assigned, self.obj_coeff, self.noobj_coeff,
                                                       sums[h])
                row_off += A * S
                h += 1
        if targets is None:
            return pred, 0, {}, {}
        nA = len(self.heads_A)
        per_A, per_V = sums[:nA, :4].sum(0), sums[nA:, :4].sum(0)
        return pred, loss, {n: per_A[i] for i, n in enumerate(LOSS_NAMES)}, {n: per_V[i] for i, n in enumerate(LOSS_NAMES)}


class ProposalGenerator(_OutOfHotPath):
    """the unimodal variant: out of scope, as the unimodal agents (model/bm_hrl_agent.py)"""
