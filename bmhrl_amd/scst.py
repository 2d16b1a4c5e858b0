"""Self-critical sequence training on sampled rollouts: REINFORCE on whole captions the model wrote
itself, with a baseline from its own other captions of the same clip (leave-one-out mean), from its greedy caption, or none.

  rollout()             n free-running samples per clip through SampleDecoder (captured token steps), every step's model
                        log-prob kept;
  prefix_scores()       the reward launch's fp64 per-prefix table of the sampled captions;
  self_critical_loss()  bmhrl_rollout_advantage (lengths, rewards, baseline, per-token weights: one launch, nothing read on
                        the host) and functional.PolicyLossFn on the log-probs of the teacher-forced training forward over
                        the sampled captions.

The step that puts them together is epoch_loops/captioning_scst_loops.train_bmhrl_scst."""
from __future__ import annotations

from collections import namedtuple

import torch

from . import ops

# toks (B * n, m + 1) int64 sample-major, column 0 the start token, pad after a row's first end token; step_logp / step_logq
# (B * n, m) fp32: the model's / the truncated sampling distribution's log-prob of every drawn token (0 behind the end);
# m: the steps decoded; n: rollouts per clip
Rollouts = namedtuple("Rollouts", "toks step_logp step_logq m n end_idx")

BASELINES = {"none": ops.BASELINE_NONE, "mean": ops.BASELINE_LEAVE_ONE_OUT, "greedy": ops.BASELINE_GIVEN}


def check_args(baseline="mean", n=4, clip=0.0, entropy=0.0):
    """ValueError for arguments self_critical_loss / train_bmhrl_scst refuse, before anything is launched"""
    if baseline not in BASELINES:
        raise ValueError(f"baseline must be one of {sorted(BASELINES)}, got {baseline!r}")
    n = int(n)
    if not 1 <= n <= ops.ROLLOUT_MAX_N:
        raise ValueError(f"n must lie in [1, {ops.ROLLOUT_MAX_N}], got {n}")
    if baseline == "mean" and n == 1:
        raise ValueError('baseline "mean" (leave-one-out) needs n >= 2 rollouts per clip')
    if not float(clip) >= 0:
        raise ValueError(f"clip must be >= 0, got {clip}")
    if not float(entropy) >= 0:
        raise ValueError(f"entropy must be >= 0, got {entropy}")


def rollout(model, feature_stacks, max_len, start_idx, end_idx, pad_idx, modality, n=4, temperature=1.0, top_k=0, top_p=1.0,
            seed=None):
    """n sampled captions per clip of the model's CURRENT weights -> Rollouts.  The agent is put into eval() for the decode
    (the incremental decoders require it; dropout off is also what a rollout should see) and its previous mode is restored.
    temperature = 0 is the greedy rollout."""
    from .decode import sample_decode
    n = int(n)
    if not 1 <= n <= ops.ROLLOUT_MAX_N:
        raise ValueError(f"n must lie in [1, {ops.ROLLOUT_MAX_N}], got {n}")
    was_training = model.training
    model.eval()
    try:
        _, toks, _, slp, slq = sample_decode(model, feature_stacks, max_len, start_idx, end_idx, pad_idx, modality, n=n,
                                             temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, return_samples=True)
    finally:
        model.train(was_training)
    B, _, m1 = toks.shape
    m = m1 - 1
    return Rollouts(toks.reshape(B * n, m1).contiguous(), slp.reshape(B * n, m).contiguous(), slq.reshape(B * n, m).contiguous(),
                    m, n, int(end_idx))


def prefix_scores(scorer, toks, captions, score_fn=None):
    """the fp64 per-prefix score table (rows, m) of the rollouts toks (rows, m + 1) (column 0 the start token) against the
    clips' captions: every clip's caption is repeated for its n = rows / len(captions) rollouts and bound.  score_fn
    (toks_without_start, captions) -> (rows, m) fp64 replaces the scorer (cfg.scst_score_fn: tests, synthetic runs)."""
    captions = list(captions)
    rows = toks.shape[0]
    if not captions or rows % len(captions):
        raise ValueError(f"{rows} rollouts do not divide into {len(captions)} clips")
    n = rows // len(captions)
    rep = [c for c in captions for _ in range(n)]
    hyp = toks[:, 1:]
    if score_fn is not None:
        out = score_fn(hyp, rep)
        if out.dtype != torch.float64 or tuple(out.shape) != tuple(hyp.shape):
            raise ValueError(f"score_fn must return a {tuple(hyp.shape)} fp64 table")
        return out
    if scorer is None:
        raise ValueError("prefix_scores needs a scorer or a score_fn")
    return scorer.prefix_scores(hyp.contiguous(), rep)


def final_rewards(rollouts, scores):
    """(rows,) fp64: every rollout's reward r_i = scores[i, len_i - 1] (rules R1 / R2), e.g. the greedy rollout's for
    baseline="greedy"; on the device, nothing read on the host"""
    return ops.rollout_advantage(rollouts.toks, 1, rollouts.m, rollouts.end_idx, scores, ops.BASELINE_NONE)[1]


def self_critical_loss(prediction, rollouts, scores, baseline="mean", clip=0.0, entropy=0.0, greedy_scores=None):
    """prediction (B * n, m, V): the train-mode forward's log-probs over the inputs rollouts.toks[:, :-1]; scores (B * n, m)
    fp64: prefix_scores of the rollouts; greedy_scores (B,) fp64 with baseline="greedy": the greedy captions' rewards
    (final_rewards).  clip > 0: the clipped-ratio form against the rollout's own log-probs; entropy > 0: an entropy bonus of
    that weight, averaged over the live tokens.  -> (loss, stats): loss = the sum of the row losses = -(1 / N) sum over
    the live tokens of adv logp[a] without clip and entropy; stats (4,) fp64 on the device = mean reward, mean baseline, mean
    length, N."""
    n, m = rollouts.n, rollouts.m
    check_args(baseline, n, clip, entropy)
    R = rollouts.toks.shape[0]
    if prediction.dim() != 3 or prediction.shape[0] != R or prediction.shape[1] != m:
        raise ValueError(f"prediction must be ({R}, {m}, V), got {tuple(prediction.shape)}")
    base = None
    if baseline == "greedy":
        if greedy_scores is None:
            raise ValueError('baseline "greedy" needs greedy_scores')
        base = greedy_scores.reshape(-1).double().contiguous()
    ln, _, _, weight, stats = ops.rollout_advantage(rollouts.toks, n, m, rollouts.end_idx, scores, BASELINES[baseline], base)
    ent_weight = None
    if entropy > 0:
        live = torch.arange(m, device=ln.device).unsqueeze(0) < ln.unsqueeze(1)
        ent_weight = (live.double() * (float(entropy) / stats[3])).float()
    logq = rollouts.step_logp if clip > 0 else None
    from .functional import PolicyLossFn
    row_loss, _ = PolicyLossFn.apply(prediction, rollouts.toks[:, 1:], weight, logq, float(clip), ent_weight)
    # (the few hundred row losses are added in fp64: the sum then carries one rounding, not one per row)
    return row_loss.double().sum().float(), stats
