"""Self-critical RL on sampled rollouts (bmhrl_amd/scst.py) with the loops' signature
(cfg, models, scorer, loader, epoch, log_prefix, TBoard, *extra) and the conventions of train_bmhrl_bl.  The reference has the
free-running decode (get_iterative_pred, epoch_loops/captioning_bmrl_loops.py:543-583) but calls it from no loop; this is the
loop it never had.  Worker phase only, no value network: the baseline comes from the model's own other captions.

cfg keys (all optional): scst_samples (4) rollouts per clip; scst_temperature (1.0), scst_top_k (0), scst_top_p (1.0) of the
sampling; scst_baseline ("mean": leave-one-out, "greedy", "none"); scst_clip (0.0) the ratio clip; scst_entropy (0.0) the entropy
bonus; scst_seed (None: a fresh seed per batch; an integer: seed + the batch's index); scst_score_fn
(toks_without_start, captions) -> (rows, m) fp64 in place of the scorer."""
import contextlib

import torch

from .. import scst
from ..decode import _rerun_setup
from ..model.masking import make_masks
from .captioning_bmrl_loops import _unwrap

_step_streams = {}


def _step_stream(device):
    """one stream per device and process for the eager forward / backward (torch's pool of 32 streams wraps)"""
    s = _step_streams.get(device)
    if s is None:
        s = _step_streams[device] = torch.cuda.Stream(device=device)
    return s


@contextlib.contextmanager
def off_default_stream(device):
    """run the body off the legacy default stream (forked from and joined into it), the way CaptionTrainer.step does: an
    autograd graph built on the legacy default stream and still alive when a HIP graph is captured later makes
    hipStreamEndCapture of this runtime fault.  On any other current stream: nothing to do."""
    cur = torch.cuda.current_stream(device)
    if cur != torch.cuda.default_stream(device):
        yield
        return
    side = _step_stream(device)
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        yield
    cur.wait_stream(side)


def rollout_forward(cap_model, feature_stacks, rollouts, modality, pad_idx):
    """the training forward over the sampled captions -> log-probs (B * n, m, V): every clip's features n times, sample-major
    (as the decoders' re-run path lays them out), the sampled captions toks[:, :-1] as the input, masks built from them"""
    rep, x = _rerun_setup(feature_stacks, rollouts.n)
    trg = rollouts.toks[:, :-1].contiguous()
    masks = make_masks(rep, trg, modality, pad_idx)
    return cap_model(x, trg, masks)[0]


def _scst_args(cfg):
    a = dict(n=int(getattr(cfg, "scst_samples", 4)), temperature=float(getattr(cfg, "scst_temperature", 1.0)),
             top_k=int(getattr(cfg, "scst_top_k", 0)), top_p=float(getattr(cfg, "scst_top_p", 1.0)),
             baseline=getattr(cfg, "scst_baseline", "mean"), clip=float(getattr(cfg, "scst_clip", 0.0)),
             entropy=float(getattr(cfg, "scst_entropy", 0.0)))
    scst.check_args(a["baseline"], a["n"], a["clip"], a["entropy"])
    return a


def scst_step(cfg, cap_model, cap_optimizer, scorer, batch, ds, args, seed=None):
    """one batch: rollouts -> scores -> training forward on the sampled captions -> PolicyLossFn -> backward -> Adam.
    Returns (loss, [mean reward, mean baseline, mean length, tokens]) as host floats: nothing of the step's autograd graph
    outlives the call."""
    agent = _unwrap(cap_model)
    fs = batch['feature_stacks']
    pad_idx, start_idx, end_idx = ds.pad_idx, ds.start_idx, ds.end_idx
    n = args["n"]
    score_fn = getattr(cfg, "scst_score_fn", None)
    # 1. rollouts FIRST: a decoder captures its token step the first time a clip-batch shape bucket appears, and no autograd
    #    graph of this step exists yet (the previous step's is gone: it returned floats)
    ro = scst.rollout(agent, fs, cfg.max_len, start_idx, end_idx, pad_idx, cfg.modality, n, args["temperature"], args["top_k"],
                      args["top_p"], seed)
    greedy = None
    if args["baseline"] == "greedy":
        greedy = scst.rollout(agent, fs, cfg.max_len, start_idx, end_idx, pad_idx, cfg.modality, 1, temperature=0.0, seed=0)
    # 2. scores
    scores = scst.prefix_scores(scorer, ro.toks, batch['captions'], score_fn)
    greedy_scores = None
    if greedy is not None:
        greedy_scores = scst.final_rewards(greedy, scst.prefix_scores(scorer, greedy.toks, batch['captions'], score_fn))
    # 3. / 4. training forward and backward, off the legacy default stream (as CaptionTrainer.step: an autograd graph built
    #    there and still alive at a later capture makes hipStreamEndCapture of this runtime fault)
    with off_default_stream(ro.toks.device):
        cap_optimizer.zero_grad()
        prediction = rollout_forward(cap_model, fs, ro, cfg.modality, pad_idx)
        loss, stats = scst.self_critical_loss(prediction, ro, scores, args["baseline"], args["clip"], args["entropy"], greedy_scores)
        loss.backward()
        cap_optimizer.step()
        if getattr(cfg, "grad_clip", None) is not None:                # (after the step, as train_bmhrl_bl and the reference)
            torch.nn.utils.clip_grad_norm_(cap_model.parameters(), cfg.grad_clip)
        out = float(loss.detach()), [float(v) for v in stats.tolist()]          # host reads: the stream's work has finished
        del prediction, loss, stats
    return out


def train_bmhrl_scst(cfg, models, scorer, loader, epoch, log_prefix, TBoard, *extra):
    """One epoch of self-critical training of the worker.  Returns the mean loss; the mean reward of the epoch's rollouts goes
    to TBoard ('debug/scst_reward_epoch')."""
    args = _scst_args(cfg)                                             # (ValueError before any launch)
    if scorer is None and getattr(cfg, "scst_score_fn", None) is None:
        raise ValueError("train_bmhrl_scst needs a scorer or cfg.scst_score_fn")
    cap_model, cap_optimizer, _ = models["captioning"]
    cap_model.train()
    loader.dataset.update_iterator()
    agent = _unwrap(cap_model)
    agent.teach_worker()
    base_seed = getattr(cfg, "scst_seed", None)
    total, reward, k = 0.0, 0.0, 0
    for batch in loader:
        seed = None if base_seed is None else int(base_seed) + (int(epoch) << 20) + k
        loss, stats = scst_step(cfg, cap_model, cap_optimizer, scorer, batch, loader.dataset, args, seed)
        total += loss
        reward += stats[0]
        k += 1
    if TBoard is not None and k:
        TBoard.add_scalar('debug/train_loss_epoch', total / k, epoch)
        TBoard.add_scalar('debug/scst_reward_epoch', reward / k, epoch)
    return total / max(k, 1)
