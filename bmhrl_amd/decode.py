"""Greedy decoding with the reference's decoder signature (epoch_loops/captioning_bmrl_loops.py:41-43,127-152):
arg-max autoregressive decode that stops when every sample has produced </s> or at max_len.

Three forms, same tokens:

  * memoise=False -- the reference's own schedule: the whole agent (encoder included) re-run for every token;
  * memoise=True  -- encoder output and the fusion layers' memory K|V projections computed once per clip batch, the caption
    side re-run over the whole prefix for every token;
  * incremental   -- IncrementalDecoder below: on top of the per-clip memory K|V, every caption-side
    layer keeps the K|V rows of the tokens decoded so far, the frozen critic carries its LSTM / GRU state, and a token costs
    one row per sample through both fusion stacks, the manager and the worker.  All shapes of a token step are static, the
    position is a device word, so the step is captured once into a HIP graph and replayed max_len times.

beam_decode / beam_decoder: beam search over the same token step on B*K rows (BeamDecoder), or over full re-runs.
sample_decode / sample_decoder: temperature / top-k / top-p sampling, n samples per clip, over the same token step on B*n rows
(SampleDecoder), or over full re-runs.
Every decoder takes no_repeat_ngram / min_len / repetition_penalty (the constraints section): the rules edit the step's
log-probs before the choice, in the captured step through one HIP launch.
Every decoder takes context / context_ngram / context_penalty (the context rules C1-C5 of the same section): the tokens of
a video's earlier captions, whose n-grams are banned and whose words are penalised, through the same one launch.
beam_decode / sample_decode take select="consensus" (the consensus section): the returned caption is the hypothesis that
agrees most with the clip's other hypotheses, one HIP launch after the token loop.
beam_decode takes beam_groups / diversity_penalty (the group beam search section): diverse beam search, the beams in groups
that choose one after another (GroupBeamDecoder: one grouped selection launch in place of the plain one, or re-runs).
"""
import math
import random

import torch

from . import ops
from .functional import SHADOWS, ExpandGoalsFn, GateFn, LayerNormFn, LinearFn, WorkerHeadFn, _attn_core_fwd, pad8
from .model.masking import make_masks

_BF16 = torch.bfloat16


def greedy_decode(model, feature_stacks, max_len, start_idx, end_idx, pad_idx, modality, return_first=False, memoise=True,
                  incremental=None, no_repeat_ngram=0, min_len=0, repetition_penalty=1.0, context=None, context_ngram=0,
                  context_penalty=1.0):
    """memoise=True (default) runs the encoder and the fusion layers' memory projections once per clip batch instead of
    once per generated token; the tokens and log-probs are the same as with the reference's full re-run (memoise=False).
    incremental (default: on for the HIP agent in eval mode on a GPU with both modalities) additionally decodes through
    IncrementalDecoder.  Models without encode_memory() (anything but the HIP BMHrlAgent) always take the full re-run.
    no_repeat_ngram / min_len / repetition_penalty: the constraints section's rules, on every path; with a rule set,
    return_first returns the first step's adjusted log-probs, and a max_len + 1 above ops.LOGIT_RULES_MAX_HIST (256, the
    kernel's history capacity) takes the re-run path.
    context / context_ngram / context_penalty: the context rules C1-C5 of that section -- context is a (B, C <= 1024) int64
    tensor or a list of B integer lists, per clip the tokens of the video's earlier captions."""
    rules = _rule_args(no_repeat_ngram, min_len, repetition_penalty, max_len)
    with torch.no_grad():
        B = feature_stacks['audio'].shape[0]
        device = feature_stacks['audio'].device
        context = _context(context, context_ngram, context_penalty, B, pad_idx, device)
        memoise = memoise and hasattr(model, "encode_memory") and not model.training
        dec = _incremental(IncrementalDecoder, model, feature_stacks, modality, max_len, start_idx, end_idx, pad_idx,
                           incremental=incremental if memoise else False, rules=rules, context=context)
        if dec is not None:
            return dec.run(return_first)
        done = torch.zeros(B, 1, dtype=torch.bool, device=device)
        trg = torch.full((B, 1), start_idx, dtype=torch.long, device=device)
        first = None
        rep, x = _rerun_setup(feature_stacks, 1)
        memory, kv_cache = None, {}
        while trg.size(-1) <= max_len and not bool(done.all()):
            if memoise:
                masks = make_masks(feature_stacks, trg, modality, pad_idx)
                if memory is None:
                    memory = model.encode_memory(x, masks)
                last = model.inference_from_memory(memory, trg, masks, kv_cache)[:, -1]
            else:
                last = _rerun_logp(model, x, rep, trg, modality, pad_idx)
            if context is not None:
                last = _apply_context_rules(last.float(), trg, trg.size(-1) - 1, rules, end_idx, pad_idx, context[0], 1,
                                            context[1])
            elif rules is not None:
                last = _apply_rules(last.float(), trg, trg.size(-1) - 1, *rules, end_idx, pad_idx)
            if first is None:
                first = last.clone()
            nxt = last.argmax(dim=-1, keepdim=True)
            trg = torch.cat([trg, nxt], dim=-1)
            done = done | (nxt == end_idx)
    return (trg, first) if return_first else trg


def _incremental(cls, model, fs, modality, max_len, start_idx, end_idx, pad_idx, rows=1, incremental=None, params=None,
                 rules=None, context=None):
    """the decoder of class `cls` (`rows` rows per clip) with the clip batch begun, or None: take the re-run path.
    incremental=None: the class's `enabled`; params: SampleDecoder.set_params arguments, rules: what _rule_args returned
    (IncrementalDecoder.set_rules arguments, None: all off), context: what _context returned (the clips' contexts and
    the set_context_rules arguments, None: off), all set before begin()"""
    if incremental is None:
        incremental = cls.enabled
    if not (incremental and hasattr(model, "encode_memory") and not model.training and fs['audio'].device.type == "cuda"
            and modality == "audio_video" and max_len >= 1 and cls._fits(model, rows)):
        return None
    if (rules is not None or context is not None) and max_len + 1 > ops.LOGIT_RULES_MAX_HIST:
        return None
    if context is not None and getattr(model, "voc_size", 0) > ops.LOGIT_RULES_CTX_MAX_V:
        return None
    dec = cls.for_batch(model, fs, max_len, start_idx, end_idx, pad_idx, rows)
    if params is not None:
        dec.set_params(*params)
    dec.set_rules(*(rules or _NO_RULES))
    dec.set_context_rules(*(context[1] if context is not None else _NO_CONTEXT_RULES))
    dec.set_context(context[0] if context is not None else None)
    return dec if dec.begin(fs) else None


def _rerun_setup(fs, rows):
    """(the feature dict with every clip's tensors repeated `rows` times, sample-major; the agent's input x of it)"""
    B = fs['audio'].shape[0]
    rep = fs if rows == 1 else {k: v.repeat_interleave(rows, 0) if torch.is_tensor(v) and v.dim() and v.shape[0] == B else v
                                for k, v in fs.items()}
    return rep, ((rep['rgb'], rep['flow']), rep['audio'])


def _rerun_logp(model, x, rep, hist, modality, pad_idx):
    """fp32 log-probs (rows, V) of the token after the prefixes `hist`: a full re-run of model.inference"""
    return model.inference(x, hist, make_masks(rep, hist, modality, pad_idx))[:, -1].float()


def bimodal_decoder(model, feature_stacks, max_len, start_idx, end_idx, pad_idx, modality):
    return greedy_decode(model, feature_stacks, max_len, start_idx, end_idx, pad_idx, modality)


def greedy_decoder(no_repeat_ngram=0, min_len=0, repetition_penalty=1.0, context_ngram=0, context_penalty=1.0):
    """a greedy decoder with the reference's signature (model, feature_stacks, max_len, start_idx, end_idx, pad_idx, modality)
    under the constraints section's rules, e.g. validation_1by1_loop(cfg, model, loader, greedy_decoder(3, min_len=5), epoch,
    TBoard).  context_ngram / context_penalty: the context rules, for the clips' contexts that a caller such as
    predict.caption_segments(paragraph=True) hands over with the optional keyword context=; without it the call is the
    reference's."""
    rules = _rule_args(no_repeat_ngram, min_len, repetition_penalty) or _NO_RULES
    crules = _context_args(context_ngram, context_penalty) or _NO_CONTEXT_RULES

    def decoder(model, feature_stacks, max_len, start_idx, end_idx, pad_idx, modality, context=None):
        return greedy_decode(model, feature_stacks, max_len, start_idx, end_idx, pad_idx, modality, no_repeat_ngram=rules[0],
                             min_len=rules[1], repetition_penalty=rules[2], context=context, context_ngram=crules[0],
                             context_penalty=crules[1])
    return decoder


bmhrl_greedy_decoder = bimodal_decoder


class IncrementalDecoder:
    """One decoded token = one row per sample through the caption side of BMHrlAgent (model/bm_hrl_agent.py:596-661),
    with everything that does not depend on the newest token kept in HBM between tokens:

      mem_kv[stack][layer][A|V]  (B, cap, 2*d_model) bf16   K|V projections of the encoder output (per clip)
      self_kv[stack][layer]      (B, Lc, 2*d_model)  bf16   K|V rows of the caption self attention (one row appended per token)
      goal_kv                    (B, Lc, 2*d_model)  bf16   K|V rows of the worker's goal attention over the worker features
      critic h / c               6 x (B, 600) fp32          LSTM(4) / GRU(2) state of the frozen segment critic
      labels (B, Lc) int32, goals_raw (B, Lc, d_goal) fp32  the manager's inputs to expand_goals (which reads whole rows)

    The fusion stack is causal (C_mask = key padding & lower triangle, model/masking.py:13-15), the critic is a forward
    recurrence and the memory attentions / LayerNorms / gate act per position, so position t of every intermediate only
    depends on tokens <= t: appending rows reproduces the full re-run.  expand_goals is not causal (a segment's last goal is
    copied back over the segment, with the row-transition quirks of the reference's loop, :415-429); it runs over the whole
    (B, Lc) label buffer every token -- positions after t carry label 0, which is what the re-run sees as "no later token".

    Static shapes (memory padded to a capacity with masked tails, Lc = padded max_len + 1, the position a device word)
    make the token step one HIP graph.  begin() returns False when a sample has no valid memory key at all (softmax of a
    fully masked row is uniform over the UNPADDED keys in the reference, :22) and the caller falls back."""

    enabled = True
    use_graph = True
    check_every = 4             # host looks at `done` every this many tokens (the result is trimmed to the exact length)
    _cache_attr = "_incremental_decoders"

    @classmethod
    def for_batch(cls, agent, fs, max_len, start_idx, end_idx, pad_idx, rows=1):
        """the class's cached decoder for a clip batch of these shapes; rows: rows per clip (beams, samples)"""
        B, Tv = fs['rgb'].shape[:2]
        Ta = fs['audio'].shape[1]
        key = (B, -(-Tv // 64) * 64, -(-Ta // 64) * 64, int(max_len), int(start_idx), int(end_idx), int(pad_idx), int(rows),
               fs['rgb'].device)
        cache = agent.__dict__.setdefault(cls._cache_attr, {})
        dec = cache.get(key)
        if dec is None:
            if len(cache) >= 8:                         # shapes of a validation set fall into a few capacity buckets
                cache.pop(next(iter(cache)))
            dec = cache[key] = cls(agent, *key[:7], device=key[8], beams=key[7])
        return dec

    @classmethod
    def _fits(cls, model, rows):
        """the class's own limit on top of the conditions of _incremental"""
        return rows == 1

    def __init__(self, agent, B, tv_cap, ta_cap, max_len, start_idx, end_idx, pad_idx, device, beams=1):
        self.agent = agent
        self.B, self.tv_cap, self.ta_cap, self.max_len = B, tv_cap, ta_cap, max_len
        # rows of every token-dependent buffer: `beams` consecutive rows per sample (BeamDecoder); the per-clip memory K|V and
        # its masks keep one row per sample, and its attentions take a sample's rows as `beams` queries
        self.K = beams
        self.R = R = B * beams
        self.start_idx, self.end_idx, self.pad_idx = start_idx, end_idx, pad_idx
        self.dev = dev = torch.device(device)
        self.dC, self.D = agent.d_model_caps, agent.d_model
        self.Lc = Lc = pad8(max_len + 1)
        D, dC = self.D, self.dC
        z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=dev)
        self.t = z(1, dtype=torch.int64)
        self.tok = z(R, dtype=torch.int64)
        self.out = z(R, max_len + 1, dtype=torch.int64)
        self.done = z(R, dtype=torch.bool)
        self.valid = z(R, 1, Lc, dtype=torch.uint8)
        self.a_mask = z(B, 1, ta_cap, dtype=torch.uint8)
        self.v_mask = z(B, 1, tv_cap, dtype=torch.uint8)
        self.labels = z(R, Lc, dtype=torch.int32)
        self.goals_raw = z(R, Lc, agent.d_goal)
        self.logp = z(R, 1, agent.voc_size)
        self.emb_scale = math.sqrt(dC)
        self.pe = agent.pos_enc_C.table(dev)
        n_layers = len(agent.bm_worker_fus.decoder.layers)
        mk = lambda n, rows: z(n, rows, 2 * D, dtype=_BF16)
        self.stacks = []
        for fus in (agent.bm_worker_fus, agent.bm_manager_fus):
            self.stacks.append(dict(fus=fus, self_kv=[mk(R, Lc) for _ in range(n_layers)],
                                    mem_a=[mk(B, ta_cap) for _ in range(n_layers)], mem_v=[mk(B, tv_cap) for _ in range(n_layers)]))
        self.goal_kv = z(R, Lc, 2 * agent.worker.goal_attention.d_model, dtype=_BF16)
        cr = agent.critic
        Hc = cr.lstm.hidden_size
        self.critic_layers = []
        for rnn, gates, n, act in ((cr.lstm, 4, 4, cr.relu), (cr.gru, 3, 2, cr.relu2)):
            for l in range(n):
                self.critic_layers.append(dict(
                    gates=gates, w_ih=getattr(rnn, f"weight_ih_l{l}"), w_hh=getattr(rnn, f"weight_hh_l{l}"),
                    b_ih=getattr(rnn, f"bias_ih_l{l}"), b_hh=getattr(rnn, f"bias_hh_l{l}"),
                    act=act if l == n - 1 else None, h=z(R, Hc), c=z(R, Hc), h_new=z(R, Hc), c_new=z(R, Hc),
                    # the step kernel reads the carried state only at positions > 0 of its window: the newest token is
                    # position 1 of a two-position window whose position 0 is never touched
                    xproj=z(R, 2, gates * Hc), seq=z(R, 2, Hc)))
        self.labels2 = z(R, 2, dtype=torch.int32)
        self.Hc = Hc
        self.graph = None
        self._shadow_sig = None
        self.steps_run = 0
        self.rules = None               # set_rules: (no_repeat_ngram, min_len, repetition_penalty) while a rule is set
        self.ctx_rules = None           # set_context_rules: (context_ngram, context_penalty) while one is set
        self.has_context = False        # set_context: do the rows of self.ctx hold the clips' contexts?
        self.ctx = torch.full((B, ops.LOGIT_RULES_MAX_CTX), pad_idx, dtype=torch.int64, device=dev)
        self._init_search()
        with torch.no_grad():
            self._reset()
            self._token_step()                      # eager once: weight shadows, allocator warm-up
            if self.use_graph:
                self._capture()
            self._reset()

    def _init_search(self):
        """buffers of the token choice (greedy: none beyond `out` / `done`)"""

    def set_rules(self, no_repeat_ngram=0, min_len=0, repetition_penalty=1.0):
        """the constraints section's rules for the decodes that follow; they are launch arguments, so the step is captured
        again when they change (the first decode under rules on a new shape therefore captures twice: __init__ without
        rules, then here).  Not while a clip batch is being decoded.  The rules stay on the decoder, as SampleDecoder's
        set_params values do: whoever takes the cached decoder from for_batch directly inherits what the last caller set --
        _incremental sets them before every clip batch, the defaults included."""
        rules = _rule_args(no_repeat_ngram, min_len, repetition_penalty, self.max_len)
        if rules is not None and self.max_len + 1 > ops.LOGIT_RULES_MAX_HIST:
            raise ValueError(f"set_rules: a history of {self.max_len + 1} tokens exceeds {ops.LOGIT_RULES_MAX_HIST}")
        if rules != self.rules:
            self.rules = rules
            if self.graph is not None:
                if rules is not None:
                    # eager once: the kernel's first launch is not one under capture.  It edits self.logp and reads self.t
                    # and self.out as the last decode left them; begin() resets all three before they are used again
                    self._constrain()
                self._capture()

    def _context_on(self):
        """does the token step run the context rules?  Only with a rule set AND a context present (rule C4)"""
        return self.ctx_rules is not None and self.has_context

    def set_context_rules(self, context_ngram=0, context_penalty=1.0):
        """the context rules C1-C2 for the decodes that follow: launch arguments as set_rules' are, so the step is captured
        again when they change while a context is present.  Not while a clip batch is being decoded; they stay on the
        decoder as set_rules' do, and _incremental sets them before every clip batch, the defaults included."""
        crules = _context_args(context_ngram, context_penalty)
        if crules is not None and self.max_len + 1 > ops.LOGIT_RULES_MAX_HIST:
            raise ValueError(f"set_context_rules: a history of {self.max_len + 1} tokens exceeds {ops.LOGIT_RULES_MAX_HIST}")
        if crules is not None and self.logp.shape[-1] > ops.LOGIT_RULES_CTX_MAX_V:
            raise ValueError(f"set_context_rules: a vocabulary of {self.logp.shape[-1]} exceeds {ops.LOGIT_RULES_CTX_MAX_V}")
        if crules != self.ctx_rules:
            was = self._context_on()
            self.ctx_rules = crules
            self._context_changed(was, True)

    def set_context(self, context=None):
        """the clips' contexts (B, C <= LOGIT_RULES_MAX_CTX) int64 for the decodes that follow, or None: copied into the
        static (B, LOGIT_RULES_MAX_CTX) buffer the captured step reads, the rest filled with pad_idx, so a new context
        needs no capture; the step is captured again only when a context appears or goes while context rules are set
        (another launch: bmhrl_logit_rules_ctx in place of the plain one, or of none)."""
        was = self._context_on()
        if context is None:
            self.has_context = False
        else:
            if context.dim() != 2 or context.shape[0] != self.B or context.shape[1] > ops.LOGIT_RULES_MAX_CTX:
                raise ValueError(f"set_context: a ({self.B}, C <= {ops.LOGIT_RULES_MAX_CTX}) tensor expected, got "
                                 f"{tuple(context.shape)}")
            self.ctx.fill_(self.pad_idx)
            self.ctx[:, :context.shape[1]] = context
            self.has_context = True
        self._context_changed(was, False)

    def _context_changed(self, was, new_rules):
        now = self._context_on()
        if (now != was or (now and new_rules)) and self.graph is not None:
            if now or self.rules is not None:
                # eager once, as in set_rules: the kernel's first launch is not one under capture
                self._constrain()
            self._capture()

    def _constrain(self):
        """rules 1-3 on self.logp, rows' sequences from self.out -- with context rules set and a context present, rules
        1, C1, 2, C2, 3 through the one launch that replaces the plain one.  An end_idx that is no token id (callers that
        never stop) leaves rule 3 nothing to ban."""
        n, m, theta = self.rules or _NO_RULES
        V = self.logp.shape[-1]
        ends = 0 <= self.end_idx < V
        if self._context_on():
            ops.logit_rules_ctx(self.logp, V, self.R, V, self.out, self.t, n, m if ends else 0, theta,
                                self.end_idx if ends else self.pad_idx, self.pad_idx, self.ctx, self.R // self.B,
                                *self.ctx_rules)
            return
        ops.logit_rules(self.logp, V, self.R, V, self.out, self.t, n, m if ends else 0, theta,
                        self.end_idx if ends else self.pad_idx, self.pad_idx)

    # ------------------------------------------------------------------ per clip
    def _reset(self):
        self.t.zero_()
        self.tok.fill_(self.start_idx)
        self.out.fill_(self.pad_idx)
        self.out[:, 0] = self.start_idx
        self.done.zero_()
        self.valid.zero_()
        self.labels.zero_()
        self.goals_raw.zero_()
        torch._foreach_zero_([l[k] for l in self.critic_layers for k in ("h", "c")])
        self.steps_run = 0

    def begin(self, fs) -> bool:
        """encoder + memory K|V projections of a clip batch into the static buffers; False = take the re-run path"""
        ag, B, D = self.agent, self.B, self.D
        masks = make_masks(fs, None, "audio_video", self.pad_idx)
        am, vm = masks['A_mask'], masks['V_mask']
        if not bool((am.any(-1) & vm.any(-1)).all()):
            return False
        Ta, Tv = am.shape[-1], vm.shape[-1]
        self.a_mask.zero_(); self.a_mask[:, :, :Ta] = am
        self.v_mask.zero_(); self.v_mask[:, :, :Tv] = vm
        x = ((fs['rgb'], fs['flow']), fs['audio'])
        Va, Av = ag.encode_memory(x, masks)                    # (B, Tv, d_vid), (B, Ta, d_aud)
        for mem, T, cap, name, att_name in ((Av, Ta, self.ta_cap, "mem_a", "enc_att_A"), (Va, Tv, self.tv_cap, "mem_v", "enc_att_V")):
            d = mem.shape[-1]
            mb = torch.zeros(B, cap, pad8(d), dtype=_BF16, device=self.dev)
            mb[:, :T, :d] = mem
            for st in self.stacks:
                for li, layer in enumerate(st["fus"].decoder.layers):
                    att = getattr(layer, att_name)
                    w_kv = SHADOWS.weight(att.linear_K2d.weight, att.linear_V2d.weight)
                    ops.gemm(mb, w_kv, B * cap, 2 * D, d, lda=mb.shape[-1], ldb=w_kv.shape[1], C_bf16=st[name][li], ldcb=2 * D,
                             bias=SHADOWS.bias(att.linear_K2d.bias, att.linear_V2d.bias))
        self._reset()
        if self.graph is not None and self._shadows() != self._shadow_sig:
            self._capture()                # weights were re-materialised since the capture (new shadow buffers)
        return True

    def run(self, return_first=False):
        """steps until max_len or, looked at every check_every tokens, until everything has finished -> result();
        return_first: also the first step's log-probs (the adjusted ones while a rule is set)"""
        first = None
        for i in range(self.max_len):
            self.step()
            if i == 0 and return_first:
                first = self.logp[:, 0].clone()
            if (i + 1) % self.check_every == 0 and i + 1 < self.max_len and self._all_done(i):
                break
        trg = self.result()
        return (trg, first) if return_first else trg

    def _all_done(self, i):
        """has every row finished after step i? (one host read)"""
        return bool(self.done.all())

    def step(self):
        if self.graph is not None:
            self.graph.replay()
        else:
            self._token_step()
        self.steps_run += 1

    def _steps_to_end(self):
        """the step at which every row had produced </s> (the reference's loop condition, :61-76), else the steps run"""
        n = self.steps_run
        is_end = self.out[:, 1:n + 1] == self.end_idx
        if n and bool(is_end.any(1).all()):
            n = int(is_end.to(torch.uint8).argmax(1).max()) + 1
        return n

    def result(self):
        """tokens up to the step at which every sample had produced </s>"""
        return self.out[:, :self._steps_to_end() + 1].clone()

    # ------------------------------------------------------------------ graph
    def _weights(self):
        """(weight groups, bias groups) whose bf16 / concatenated shadows the token step reads"""
        ag = self.agent
        ws, bs = [], []
        for st in self.stacks:
            for layer in st["fus"].decoder.layers:
                a = layer.self_att
                ws += [(a.linear_Q2d.weight, a.linear_K2d.weight, a.linear_V2d.weight), (a.linear_d2Q.weight,)]
                bs += [(a.linear_Q2d.bias, a.linear_K2d.bias, a.linear_V2d.bias)]
                for m in (layer.enc_att_A, layer.enc_att_V):
                    ws += [(m.linear_Q2d.weight,), (m.linear_d2Q.weight,), (m.linear_K2d.weight, m.linear_V2d.weight)]
                    bs += [(m.linear_K2d.bias, m.linear_V2d.bias)]
        g = ag.worker.goal_attention
        ws += [(g.linear_Q2d.weight,), (g.linear_K2d.weight, g.linear_V2d.weight), (g.linear_d2Q.weight,),
               (ag.manager.linear.weight,)]
        bs += [(g.linear_K2d.bias, g.linear_V2d.bias)]
        return ws, bs

    def _shadows(self):
        """refreshes the shadows the captured kernels read (bf16 weights are re-cast in place when a parameter changed,
        concatenated biases are rebuilt) and returns their addresses: a different address means the graph holds a dead
        pointer and is captured again"""
        ws, bs = self._weights()
        # (+ the parameters the step reads directly -- LayerNorm, biases, embedding table, critic weights: their storages
        # move when the module is re-materialised, e.g. by .to(device) or by a trainer that re-points them into its bucket)
        return tuple(SHADOWS.weight(*w).data_ptr() for w in ws) + tuple(SHADOWS.bias(*b).data_ptr() for b in bs) + \
            (SHADOWS.weight_split3(self.agent.worker.core.projection.weight).data_ptr(),) + \
            tuple(p.data_ptr() for p in self.agent.parameters())

    def _capture(self):
        self._shadow_sig = self._shadows()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._token_step()
        self.graph = g

    # ------------------------------------------------------------------ one token
    def _attend(self, att, norm, x, kv, mask, Sk, residual, append, sq=1):
        """x (R, dq) fp32 -> [x +] d2Q(attention(Q2d(LN?(x)), K|V rows in `kv`)) (R, dq) fp32.  append: this is a self
        attention -- the K|V projection of the (normalised) row is written at position t of `kv` first.  sq: query rows per
        batch entry of `kv` (the per-sample memory: the sample's beams; 1: one K|V batch entry per row)."""
        B, dev = self.R, self.dev
        D, H = att.d_model, att.H
        dq = x.shape[1]
        ldx = pad8(dq)
        xb = ops.bf16_zeros(B, dq, dev)
        if norm is not None:
            ops.layernorm_fwd(x, norm.weight.detach(), norm.bias.detach(), xb, ldx, None, None, None, B, dq)
        else:
            ops.cast_bf16(x, dq, xb, ldx, B, dq)
        if append is not None:
            w = SHADOWS.weight(att.linear_Q2d.weight, *append[0])
            n_out = w.shape[0]
            bias = SHADOWS.bias(att.linear_Q2d.bias, *append[1])
            q = torch.empty(B, n_out, dtype=_BF16, device=dev)
            ops.gemm(xb, w, B, n_out, dq, lda=ldx, ldb=w.shape[1], C_bf16=q, ldcb=n_out, bias=bias)
            kv.index_copy_(1, self.t, q[:, D:].unsqueeze(1))
            ldq = n_out
        else:
            w = SHADOWS.weight(att.linear_Q2d.weight)
            q = torch.empty(B, D, dtype=_BF16, device=dev)
            ops.gemm(xb, w, B, D, dq, lda=ldx, ldb=w.shape[1], C_bf16=q, ldcb=D, bias=att.linear_Q2d.bias.detach())
            ldq = D
        o, _ = _attn_core_fwd(q, 0, ldq, kv, 0, 2 * D, kv, D, 2 * D, mask, Sk, 0, B // sq, H, sq, Sk, D // H, 0.0, 0)
        w_o = SHADOWS.weight(att.linear_d2Q.weight)
        y = torch.empty(B, dq, device=dev)
        ops.gemm(o, w_o, B, dq, D, lda=D, ldb=w_o.shape[1], C_f32=y, ldc=dq, bias=att.linear_d2Q.bias.detach(),
                 residual=x if residual else None, ldr=dq)
        return y

    def _critic_step(self, emb):
        B, Hc = self.R, self.Hc
        x = emb
        for l in self.critic_layers:
            g = l["gates"]
            ops.gemm_f32(x, l["w_ih"], l["b_ih"], l["b_hh"] if g == 4 else None, l["xproj"][:, 1], B, g * Hc, x.shape[1])
            act = l["act"]
            ops.rnn_step(g, l["xproj"], l["w_hh"], l["b_hh"] if g == 3 else None, l["h"], l["c"], l["h_new"],
                         l["c_new"] if g == 4 else None, l["seq"], act.alpha if act is not None else None,
                         act.beta if act is not None else None, B, 2, Hc, 1)
            x = l["seq"][:, 1]
        torch._foreach_copy_([l[k] for l in self.critic_layers for k in ("h", "c")],
                             [l[k] for l in self.critic_layers for k in ("h_new", "c_new")])
        cr = self.agent.critic
        ops.critic_head(self.critic_layers[-1]["seq"], cr.lin.weight, cr.lin.bias, float(self.agent.critic_score_threshhold),
                        None, self.labels2, 2 * B, Hc)
        self.labels.index_copy_(1, self.t, self.labels2[:, 1:2])

    def _token_step(self):
        ag, B, t = self.agent, self.R, self.t
        emb = ag.emb_C.embedder.weight.detach().index_select(0, self.tok) * self.emb_scale     # (B, dC): the critic's input
        C0 = emb + self.pe.index_select(0, t)
        self.valid.index_copy_(2, t, (self.tok != self.pad_idx).to(torch.uint8).view(B, 1, 1))
        self._critic_step(emb.contiguous())
        feats = []
        for st in self.stacks:
            C = C0
            for li, layer in enumerate(st["fus"].decoder.layers):
                a = layer.self_att
                C = self._attend(a, layer.res_layer_self_att.norm, C, st["self_kv"][li], self.valid, self.Lc, True,
                                 ((a.linear_K2d.weight, a.linear_V2d.weight), (a.linear_K2d.bias, a.linear_V2d.bias)))
                Ca = self._attend(layer.enc_att_A, layer.res_layer_enc_att_A.norm, C, st["mem_a"][li], self.a_mask, self.ta_cap,
                                  True, None, self.K)
                Cv = self._attend(layer.enc_att_V, layer.res_layer_enc_att_V.norm, C, st["mem_v"][li], self.v_mask, self.tv_cap,
                                  True, None, self.K)
                C = layer._tail(Cv, Ca)            # normCA, normCV, gate: the kernel of the full forward (bit-identical)
            feats.append(C)
        w_feat, m_feat = feats
        # manager (:437-454, exploration off while decoding): the newest raw goal joins the buffer, expand_goals reads whole rows
        g = LinearFn.apply(m_feat, ag.manager.linear.weight, ag.manager.linear.bias, False, 0.0)
        self.goals_raw.index_copy_(1, t, g.unsqueeze(1))
        goal = ExpandGoalsFn.apply(self.goals_raw, self.labels).index_select(1, t).squeeze(1)      # (B, d_goal)
        # worker (:480-487): goal attention over the worker features decoded so far, then the vocabulary head
        ga = ag.worker.goal_attention
        xb = ops.bf16_zeros(B, self.dC, self.dev)
        ops.cast_bf16(w_feat, self.dC, xb, xb.shape[1], B, self.dC)
        w_kv = SHADOWS.weight(ga.linear_K2d.weight, ga.linear_V2d.weight)
        kv_t = torch.empty(B, w_kv.shape[0], dtype=_BF16, device=self.dev)
        ops.gemm(xb, w_kv, B, w_kv.shape[0], self.dC, lda=xb.shape[1], ldb=w_kv.shape[1], C_bf16=kv_t, ldcb=w_kv.shape[0],
                 bias=SHADOWS.bias(ga.linear_K2d.bias, ga.linear_V2d.bias))
        self.goal_kv.index_copy_(1, t, kv_t.unsqueeze(1))
        gc = self._attend(ga, None, goal.contiguous(), self.goal_kv, self.valid, self.Lc, False, None)
        logp = WorkerHeadFn.apply(w_feat.view(B, 1, -1), gc.view(B, 1, -1), ag.worker.core.projection.weight,
                                  ag.worker.core.projection.bias)
        self.logp.copy_(logp)
        if self.rules is not None or self._context_on():
            self._constrain()
            logp = self.logp
        self._choose(logp)
        t.add_(1)

    def _choose(self, logp):
        """greedy: the arg-max token of every row is the next input"""
        B, t = self.R, self.t
        nxt = logp.view(B, -1).argmax(-1)
        self.out.index_copy_(1, t + 1, nxt.view(B, 1))
        self.done.logical_or_(nxt == self.end_idx)
        self.tok.copy_(nxt)


# ---------------------------------------------------------------------------------------------------------- constraints
# Rules (both paths -- bmhrl_logit_rules in the captured token step, _apply_rules in the re-runs -- implement exactly
# these).  Inputs: no_repeat_ngram = n >= 0, min_len = m >= 0, repetition_penalty = theta (finite, > 0; the fp32 value of
# the host float).  A row's sequence at step t is s = out[row, 0..t]: the start token and the t tokens generated so far
# (a beam's own history; pad_idx after a finished row's end).  lp: the model's fp32 log-probs of that row (V values).
#  1. penalty.  theta != 1: for every distinct token id v of s with v != pad_idx, lp[v] = lp[v] * theta -- one fp32 multiply,
#     once per id however often it occurs.  Log-probs are <= 0, so theta > 1 lowers them;
#  2. n-gram ban.  n >= 1 and t + 1 >= n: for every j in [0, t + 1 - n] with s[j .. j+n-2] == s[t-n+2 .. t],
#     lp[s[j+n-1]] = -inf.  The compared slice is empty for n = 1: every token of s is banned.  t + 1 < n: nothing is;
#  3. minimum length.  t < m: lp[end_idx] = -inf (an end_idx that is no token id, e.g. -1 for "never stop": nothing);
#  4. the adjusted lp replaces the model's log-probs in everything downstream, without renormalising: the greedy arg-max,
#     beam rules 2-3 (scores are sums of adjusted values), sampling rules 2-5 (q, the recorded step_logp / sum_logp and
#     step_logq are computed from adjusted values).  A row whose every entry is -inf falls under the choosers' own rules for
#     such rows (arg-max: token 0);
#  5. with n = 0, m = 0, theta = 1 nothing is touched and the token step has no launch more than without this section.
#     Finished rows are adjusted like live ones; their choice ignores lp already.
# A token id of s outside [0, V) takes part in the comparisons of rule 2 but selects no entry of lp.
# Refused with ValueError: n < 0, m < 0, n or m not an integer, theta non-finite or <= 0, m > max_len.
#
# Context rules (paragraph-aware decoding; both paths -- bmhrl_logit_rules_ctx in the captured token step,
# _apply_context_rules in the re-runs -- implement exactly these).  Inputs: context_ngram = n_c >= 0, context_penalty =
# theta_c (finite, > 0; the fp32 value of the host float), and per clip a context ctx of C <= 1024 int64 entries
# (ops.LOGIT_RULES_MAX_CTX): the tokens of the video's earlier captions.  An entry is a WORD when 0 <= id < V and
# id != pad_idx; anything else is a GAP -- a sentence separator or filler.  All rows of a clip (beams, samples) share the
# clip's context.
#  C1. penalty.  theta_c != 1: for every distinct word id v of the context, lp[v] = lp[v] * theta_c -- one fp32 multiply,
#      once per id however often it occurs.  It is applied after rule 1: an id that is both in s and in the context takes
#      rule 1's multiply first and then this one.  The order is fixed, so the bits are too;
#  C2. ban.  n_c >= 1 and t >= n_c - 1: the tail is s[t-n_c+2 .. t], the last n_c - 1 GENERATED tokens -- s[0], the start
#      token, is never part of it; for n_c = 1 the tail is empty.  For every j in [0, C - n_c] such that ctx[j .. j+n_c-1]
#      are all words and ctx[j .. j+n_c-2] equals the tail, lp[ctx[j+n_c-1]] = -inf.  A window that holds a gap matches
#      nothing, so n-grams never span two context sentences;
#  C3. order.  The rules run as 1, C1, 2, C2, 3: bans come after penalties, so a banned entry is -inf whatever was
#      multiplied into it.  Rule 4 (no renormalising; everything downstream reads the adjusted values) holds unchanged;
#  C4. off state.  With no context given, or with n_c = 0 and theta_c = 1, nothing of these rules runs and the step has
#      the launches it has without them: the plain bmhrl_logit_rules when rules 1-3 are set, none otherwise.  With them,
#      bmhrl_logit_rules_ctx REPLACES the plain launch: still one rules launch per token;
#  C5. refused with ValueError: n_c < 0 or not an integer, theta_c non-finite or <= 0, a context with more than 1024
#      columns, a context whose row count is not the clip count.
# The ban guarantees that no returned hypothesis shares an n_c-gram with the sentences of its context, and nothing more.
# A vocabulary above ops.LOGIT_RULES_CTX_MAX_V (65536, the kernel's bit map) takes the re-run path.

_NO_RULES = (0, 0, 1.0)
_NO_CONTEXT_RULES = (0, 1.0)


def _rule_args(no_repeat_ngram=0, min_len=0, repetition_penalty=1.0, max_len=None):
    """(n, m, theta as the fp32 value the kernel sees) of valid arguments, None when they are the defaults (no rule set)"""
    for name, v in (("no_repeat_ngram", no_repeat_ngram), ("min_len", min_len)):
        try:
            whole = not isinstance(v, bool) and int(v) == v
        except (TypeError, ValueError, OverflowError):
            whole = False
        if not whole:
            raise ValueError(f"{name} must be an integer, got {v!r}")
    n, m, theta = int(no_repeat_ngram), int(min_len), float(repetition_penalty)
    if n < 0:
        raise ValueError(f"no_repeat_ngram must be >= 0, got {no_repeat_ngram}")
    if m < 0 or (max_len is not None and m > max_len):
        raise ValueError(f"min_len must lie in [0, max_len], got {min_len}")
    if not (math.isfinite(theta) and theta > 0 and math.isfinite(_f32(theta)) and _f32(theta) > 0):
        raise ValueError(f"repetition_penalty must be finite and > 0, got {repetition_penalty}")
    rules = (n, m, _f32(theta))
    return None if rules == _NO_RULES else rules


def _apply_rules(lp, hist, t, ngram, min_len, penalty, end_idx, pad_idx):
    """rules 1-3 in fp32 torch ops: lp (R, V) fp32 log-probs, hist (R, >= t + 1) int64 sequences -> the adjusted (R, V)"""
    R, V = lp.shape
    s = hist[:, :t + 1]
    neg = torch.full_like(lp, float("-inf"))
    entry = lambda ids: ((ids >= 0) & (ids < V), ids.clamp(0, V - 1))     # ids outside [0, V) select no entry of lp
    if penalty != 1:
        ok, idx = entry(s)
        seen = torch.zeros(R, V, dtype=torch.int32, device=lp.device).scatter_add_(1, idx, (ok & (s != pad_idx)).to(torch.int32)) > 0
        lp = torch.where(seen, lp * torch.tensor(penalty, dtype=lp.dtype, device=lp.device), lp)
    if ngram >= 1 and t + 1 >= ngram:
        grams = s.unfold(1, ngram, 1)                                         # (R, t + 2 - n, n): s[j .. j+n-1]
        match = (grams[..., :ngram - 1] == s[:, t + 2 - ngram:].unsqueeze(1)).all(-1)
        ok, idx = entry(grams[..., -1])
        banned = torch.zeros(R, V, dtype=torch.int32, device=lp.device).scatter_add_(1, idx, (match & ok).to(torch.int32)) > 0
        lp = torch.where(banned, neg, lp)
    if t < min_len and 0 <= end_idx < V:
        lp = lp.clone()
        lp[:, end_idx] = float("-inf")
    return lp


def _context_args(context_ngram=0, context_penalty=1.0):
    """(n_c, theta_c as the fp32 value the kernel sees) of valid arguments, None when they are the defaults (rule C4)"""
    try:
        whole = not isinstance(context_ngram, bool) and int(context_ngram) == context_ngram
    except (TypeError, ValueError, OverflowError):
        whole = False
    if not whole or int(context_ngram) < 0:
        raise ValueError(f"context_ngram must be an integer >= 0, got {context_ngram!r}")
    try:
        theta = float(context_penalty)
    except (TypeError, ValueError):
        raise ValueError(f"context_penalty must be finite and > 0, got {context_penalty!r}") from None
    if not (math.isfinite(theta) and theta > 0 and math.isfinite(_f32(theta)) and _f32(theta) > 0):
        raise ValueError(f"context_penalty must be finite and > 0, got {context_penalty}")
    crules = (int(context_ngram), _f32(theta))
    return None if crules == _NO_CONTEXT_RULES else crules


def _context(context, context_ngram, context_penalty, B, pad_idx, device):
    """the checked arguments of the context rules: ((B, C) int64 contexts on `device`, (n_c, theta_c)), or None in the
    off state of rule C4 (no context, or n_c = 0 and theta_c = 1).  context: a (B, C <= 1024) integer tensor, or B integer
    lists that are padded to a common width (at least 1) with pad_idx."""
    crules = _context_args(context_ngram, context_penalty)
    if context is None:
        return None
    if torch.is_tensor(context):
        if context.dim() != 2 or context.is_floating_point() or context.dtype == torch.bool:
            raise ValueError(f"context must be a (B, C) integer tensor, got {tuple(context.shape)} {context.dtype}")
        ctx = context
    else:
        rows = [[int(v) for v in row] for row in context]
        width = max([1] + [len(row) for row in rows])
        ctx = torch.tensor([row + [pad_idx] * (width - len(row)) for row in rows], dtype=torch.int64).view(len(rows), width)
    if ctx.shape[0] != B:
        raise ValueError(f"context holds {ctx.shape[0]} rows for {B} clips")
    if ctx.shape[1] > ops.LOGIT_RULES_MAX_CTX:
        raise ValueError(f"a context of {ctx.shape[1]} columns exceeds {ops.LOGIT_RULES_MAX_CTX}")
    if crules is None:
        return None
    if ctx.shape[1] == 0:
        ctx = torch.full((B, 1), pad_idx, dtype=torch.int64)
    return ctx.to(device=device, dtype=torch.int64).contiguous(), crules


def _apply_context_rules(lp, hist, t, rules, end_idx, pad_idx, ctx, rows_per_ctx, crules):
    """rules 1, C1, 2, C2, 3 (rule C3's order) in fp32 torch ops: lp (R, V) fp32 log-probs, hist (R, >= t + 1) int64
    sequences, rules = (n, m, theta) or None, ctx (R / rows_per_ctx, C) int64 contexts, crules = (n_c, theta_c) -> the
    adjusted (R, V)"""
    R, V = lp.shape
    n, m, theta = rules or _NO_RULES
    n_c, theta_c = crules
    c = ctx.to(hist.device).repeat_interleave(rows_per_ctx, 0)
    word = (c >= 0) & (c < V) & (c != pad_idx)
    idx = c.clamp(0, V - 1)
    lp = _apply_rules(lp, hist, t, 0, 0, theta, end_idx, pad_idx)                                   # rule 1
    if theta_c != 1:
        seen = torch.zeros(R, V, dtype=torch.int32, device=lp.device).scatter_add_(1, idx, word.to(torch.int32)) > 0
        lp = torch.where(seen, lp * torch.tensor(theta_c, dtype=lp.dtype, device=lp.device), lp)
    lp = _apply_rules(lp, hist, t, n, 0, 1.0, end_idx, pad_idx)                                     # rule 2
    if n_c >= 1 and t >= n_c - 1 and c.shape[1] >= n_c:
        tail = hist[:, t + 2 - n_c:t + 1]                                                           # (R, n_c - 1)
        match = (c.unfold(1, n_c, 1)[..., :n_c - 1] == tail.unsqueeze(1)).all(-1) & word.unfold(1, n_c, 1).all(-1)
        banned = torch.zeros(R, V, dtype=torch.int32, device=lp.device).scatter_add_(
            1, idx[:, n_c - 1:], match.to(torch.int32)) > 0
        lp = torch.where(banned, torch.full_like(lp, float("-inf")), lp)
    return _apply_rules(lp, hist, t, 0, m, 1.0, end_idx, pad_idx)                                   # rule 3


# ---------------------------------------------------------------------------------------------------------- beam search
# Rules (both paths below implement exactly these):
#  1. beam 0 of a sample starts live with score 0 and input start_idx; beams 1..K-1 start finished with score -inf;
#  2. at every step a live beam k offers V candidates (k, v) scored score_k + lp(k, v) (one fp32 add), a finished beam the
#     single candidate (k, pad_idx) with score_k;
#  3. per sample the K best candidates become the new beams, best first, ties to the smaller k*V + v (a stable sort of
#     -score); choosing end_idx finishes a beam;
#  4. stop after the step at which every beam of every sample is finished, or after max_len steps;
#  5. n_k = generated tokens up to and including the first end_idx (the steps run if none); the best hypothesis has the
#     largest score_k / ((5 + n_k) / 6) ** length_penalty, ties to the lower beam index;
#  6. the result is int64 (B, n + 1): start_idx, the chosen hypothesis, pad_idx after its end; n = max n_k of the chosen.
# With K = 1 this is greedy decoding with pad_idx after each sample's first end_idx (up to candidates whose fp32 sums
# round to the same score: rule 3 then takes the smaller token id).


def beam_decode(model, feature_stacks, max_len, start_idx, end_idx, pad_idx, modality, beam_size=4, length_penalty=0.0,
                return_scores=False, return_beams=False, incremental=None, no_repeat_ngram=0, min_len=0,
                repetition_penalty=1.0, select="logp", consensus_n=4, consensus_weight=None, beam_groups=1,
                diversity_penalty=0.0, return_groups=False, context=None, context_ngram=0, context_penalty=1.0):
    """Beam search with the reference decoder's arguments.  Returns tokens (B, n + 1) int64, then -- when asked -- the
    chosen hypotheses' raw scores (B,) fp32, then all K hypotheses sorted best first as tokens (B, K, m + 1) (m: the
    longest n_k of all of them, so that no hypothesis is cut) and raw scores (B, K).
    incremental (default: on under the conditions greedy_decode takes IncrementalDecoder, and K <= min(16, V)) decodes
    through BeamDecoder; otherwise, or with incremental=False, every step re-runs model.inference over the (B*K)-row prefix
    batch (any model with `inference`, CPU included).  no_repeat_ngram / min_len / repetition_penalty: the constraints
    section's rules; the scores are then sums of adjusted log-probs, and a max_len + 1 above ops.LOGIT_RULES_MAX_HIST (256)
    takes the re-run path.
    select="consensus" (with consensus_n = N in [1, 4] and consensus_weight = None or a (V,) tensor of token weights)
    replaces rule 5's choice by the consensus section's: the returned tokens and score are those of the hypothesis with the
    largest utility, and return_beams appends the utilities (B, K) fp64 of the returned hypotheses, in their order, as the
    LAST element of the tuple.  With select="logp" (the default) the tuple is as described above.
    beam_groups = G > 1 with diversity_penalty (the group beam search section): diverse beam search, the K beams in G groups
    of K / G that choose one after another, through GroupBeamDecoder under the conditions BeamDecoder is taken, else over
    re-runs.  With G = 1 (the default) the search is the plain one above whatever diversity_penalty is.  return_groups (only
    with return_beams) appends the group index (B, K) int64 of the returned hypotheses, in their order, after the beams'
    scores and before the consensus utilities.
    context / context_ngram / context_penalty: the context rules C1-C5 of the constraints section; the K beams of a clip
    share the clip's context."""
    K = int(beam_size)
    if K < 1:
        raise ValueError(f"beam_size must be >= 1, got {beam_size}")
    rules = _rule_args(no_repeat_ngram, min_len, repetition_penalty, max_len)
    consensus = _consensus_args(select, consensus_n, consensus_weight)
    G, lam = _group_args(K, beam_groups, diversity_penalty, return_groups, return_beams)
    with torch.no_grad():
        context = _context(context, context_ngram, context_penalty, feature_stacks['audio'].shape[0], pad_idx,
                           feature_stacks['audio'].device)
        if G == 1:
            dec = _incremental(BeamDecoder, model, feature_stacks, modality, max_len, start_idx, end_idx, pad_idx, K,
                               incremental, rules=rules, context=context)
            found = dec.run() if dec is not None else _beam_rerun(model, feature_stacks, max_len, start_idx, end_idx, pad_idx,
                                                                  modality, K, rules, context)
        else:
            dec = _incremental(GroupBeamDecoder, model, feature_stacks, modality, max_len, start_idx, end_idx, pad_idx, K,
                               incremental, params=(G, lam), rules=rules, context=context)
            found = dec.run() if dec is not None else _group_beam_rerun(model, feature_stacks, max_len, start_idx, end_idx,
                                                                        pad_idx, modality, K, G, lam, rules, context=context)
        util = None if consensus is None else _consensus_utilities(dec, found[0], found[2], end_idx, *consensus)
        return _beam_result(*found, end_idx, length_penalty, return_scores, return_beams, util,
                            K // G if return_groups else None)


def beam_decoder(beam_size=4, length_penalty=0.0, no_repeat_ngram=0, min_len=0, repetition_penalty=1.0, select="logp",
                 consensus_n=4, consensus_weight=None, beam_groups=1, diversity_penalty=0.0, context_ngram=0,
                 context_penalty=1.0):
    """a decoder with the reference's signature (model, feature_stacks, max_len, start_idx, end_idx, pad_idx, modality), e.g.
    validation_1by1_loop(cfg, model, loader, beam_decoder(4), epoch, TBoard); select / consensus_n / consensus_weight: the
    consensus section's choice among the K beams; beam_groups / diversity_penalty: the group beam search section's diverse
    beams, e.g. beam_decoder(8, beam_groups=4, diversity_penalty=0.5, select="consensus"); context_ngram / context_penalty:
    the context rules, for the contexts handed over with the optional keyword context= (as greedy_decoder)"""
    if int(beam_size) < 1:
        raise ValueError(f"beam_size must be >= 1, got {beam_size}")
    rules = _rule_args(no_repeat_ngram, min_len, repetition_penalty) or _NO_RULES
    _consensus_args(select, consensus_n, consensus_weight)
    _group_args(int(beam_size), beam_groups, diversity_penalty)
    crules = _context_args(context_ngram, context_penalty) or _NO_CONTEXT_RULES

    def decoder(model, feature_stacks, max_len, start_idx, end_idx, pad_idx, modality, context=None):
        return beam_decode(model, feature_stacks, max_len, start_idx, end_idx, pad_idx, modality, beam_size=beam_size,
                           length_penalty=length_penalty, no_repeat_ngram=rules[0], min_len=rules[1],
                           repetition_penalty=rules[2], select=select, consensus_n=consensus_n,
                           consensus_weight=consensus_weight, beam_groups=beam_groups, diversity_penalty=diversity_penalty,
                           context=context, context_ngram=crules[0], context_penalty=crules[1])
    return decoder


def _beam_rerun(model, fs, max_len, start_idx, end_idx, pad_idx, modality, K, rules=None, context=None):
    """rules 1-4 over full re-runs of model.inference on the prefix batch -> (tokens (B, K, n + 1), scores (B, K), n);
    rules: what _rule_args returned, context: what _context returned"""
    B = fs['audio'].shape[0]
    dev = fs['audio'].device
    rep, x = _rerun_setup(fs, K)
    scores = torch.full((B, K), float("-inf"), device=dev)
    scores[:, 0] = 0.0
    finished = torch.ones(B, K, dtype=torch.bool, device=dev)
    finished[:, 0] = False
    hist = torch.full((B * K, 1), start_idx, dtype=torch.long, device=dev)
    steps = 0
    while steps < max_len:
        lp = _rerun_logp(model, x, rep, hist, modality, pad_idx)
        if context is not None:
            lp = _apply_context_rules(lp, hist, steps, rules, end_idx, pad_idx, context[0], K, context[1])
        elif rules is not None:
            lp = _apply_rules(lp, hist, steps, *rules, end_idx, pad_idx)
        V = lp.shape[-1]
        cand = scores.unsqueeze(-1) + lp.view(B, K, V)
        only = torch.zeros_like(cand)
        only[..., pad_idx] = scores
        cand = torch.where(finished.unsqueeze(-1), only, cand).view(B, K * V)
        pick = _stable_top(cand, finished, pad_idx)
        parent, tok = pick // V, pick % V
        scores = cand.gather(1, pick)
        finished = finished.gather(1, parent) | (tok == end_idx)
        hist = hist.view(B, K, -1).gather(1, parent.unsqueeze(-1).expand(-1, -1, hist.shape[-1])).view(B * K, -1)
        hist = torch.cat([hist, tok.view(B * K, 1)], 1)
        steps += 1
        if bool(finished.all()):
            break
    return hist.view(B, K, -1), scores, steps


def _stable_top(cand, finished, pad_idx):
    """flat indices of the K best of the (B, K*V) candidates per sample, ties to the smaller index; the V - 1 entries of a
    finished beam other than (k, pad_idx) are not candidates.  Two stable sorts (score, then candidate-or-not) instead of a
    NaN filler: where NaN sorts depends on the device's sort."""
    B, K = finished.shape
    V = cand.shape[1] // K
    excluded = finished.unsqueeze(-1) & (torch.arange(V, device=cand.device) != pad_idx)
    by_score = torch.sort(-cand, dim=1, stable=True).indices
    by_kind = torch.sort(excluded.view(B, K * V).gather(1, by_score).to(torch.uint8), dim=1, stable=True).indices
    return by_score.gather(1, by_kind)[:, :K]


def _best_hypothesis(toks, scores, steps, end_idx, length_penalty):
    """beam rules 5-6 (sampling rules 6-7) over (B, K, >= steps + 1) hypotheses and their raw scores -> (n_k (B, K), the
    hypotheses' order (B, K) best first, the best ones' tokens (B, n + 1))"""
    B = scores.shape[0]
    is_end = toks[..., 1:steps + 1] == end_idx
    before = (is_end.cumsum(-1) == 0).sum(-1)
    n_k = torch.where(is_end.any(-1), before + 1, torch.full_like(before, steps))
    final = scores / ((5.0 + n_k.to(scores.dtype)) / 6.0) ** length_penalty
    order = torch.sort(-final, dim=1, stable=True).indices
    rows = torch.arange(B, device=scores.device)
    n = int(n_k[rows, order[:, 0]].max()) if B else 0
    return n_k, order, toks[rows, order[:, 0], :n + 1].clone()


def _beam_result(toks, scores, steps, end_idx, length_penalty, return_scores, return_beams, util=None, group_size=None):
    """rules 5-6 over (B, K, >= steps + 1) hypotheses and their raw scores; util: the hypotheses' consensus utilities (B, K),
    in the rows' order -- the choice is then consensus rule R7 over rule 5's order; group_size: K' of rule G1 when the
    returned hypotheses' group indices are asked for (return_groups)"""
    toks = toks[..., :steps + 1]
    n_k, order, best = _best_hypothesis(toks, scores, steps, end_idx, length_penalty)
    chosen = order[:, :1]
    if util is not None:
        pick, best = _consensus_choice(toks, n_k, order, util)
        chosen = pick.unsqueeze(1)
    out = [best]
    if return_scores:
        out.append(scores.gather(1, chosen).squeeze(1))
    if return_beams:
        m = int(n_k.max()) if scores.shape[0] else 0
        out += [toks.gather(1, order.unsqueeze(-1).expand(-1, -1, toks.shape[-1]))[..., :m + 1].clone(), scores.gather(1, order)]
        if group_size is not None:
            out.append(torch.div(order, group_size, rounding_mode="floor"))
        if util is not None:
            out.append(util.gather(1, order))
    return out[0] if len(out) == 1 else tuple(out)


class BeamDecoder(IncrementalDecoder):
    """IncrementalDecoder's token step on B*K rows (sample-major: the K beams of a sample are consecutive rows), followed
    by the HIP beam step inside the same captured graph:

      bmhrl_beam_select   per sample, the K best of the K*V candidates (rules 2-3): new scores, finished flags, parents,
                          next input tokens, history column t + 1, and the `last_live` word the host polls;
      bmhrl_beam_reorder  rows [0, t] of every per-beam buffer (caption self K|V of both stacks, goal K|V, the 12 critic
                          h / c tensors, labels, raw goals, the valid mask, the token history) from the parent beam, as a
                          gather into a scratch image and a copy-back (two launches over one table of buffers).

    The per-clip memory K|V is not replicated: its attentions take a sample's K beam rows as K queries."""

    _cache_attr = "_beam_decoders"

    @classmethod
    def _fits(cls, model, rows):
        return rows <= min(ops.BEAM_MAX, getattr(model, "voc_size", 0))

    def __init__(self, agent, B, tv_cap, ta_cap, max_len, start_idx, end_idx, pad_idx, device, beams=4):
        if not 1 <= beams <= min(ops.BEAM_MAX, agent.voc_size):
            raise ValueError(f"BeamDecoder: beam size {beams} outside [1, min(16, V)]")
        super().__init__(agent, B, tv_cap, ta_cap, max_len, start_idx, end_idx, pad_idx, device, beams=beams)

    def _init_search(self):
        R, dev = self.R, self.dev
        self.scores = torch.zeros(R, device=dev)
        self.finished = torch.zeros(R, dtype=torch.uint8, device=dev)
        self.parent = torch.zeros(R, dtype=torch.int32, device=dev)
        self.last_live = torch.zeros(1, dtype=torch.int32, device=dev)
        per_beam = [(kv, kv[0, 0].numel() * kv.element_size()) for st in self.stacks for kv in st["self_kv"]]
        per_beam += [(self.goal_kv, self.goal_kv[0, 0].numel() * self.goal_kv.element_size())]
        per_beam += [(l[k], 0) for l in self.critic_layers for k in ("h", "c")]
        per_beam += [(self.labels, 4), (self.goals_raw, self.goals_raw.shape[-1] * 4), (self.valid, 1), (self.out, 8)]
        self._scratch = [torch.empty_like(b) for b, _ in per_beam]
        self._table, self._n_blocks = ops.beam_reorder_table(
            [(b, s, pos) for (b, pos), s in zip(per_beam, self._scratch)], R, dev)
        self._n_buffers = len(per_beam)

    def _reset(self):
        super()._reset()
        s, f = self.scores.view(self.B, self.K), self.finished.view(self.B, self.K)
        s.fill_(float("-inf")); s[:, 0] = 0.0
        f.fill_(1); f[:, 0] = 0
        self.parent.zero_()
        self.last_live.zero_()

    def _choose(self, logp):
        V = self.logp.shape[-1]
        ops.beam_select(self.logp, V, self.scores, self.finished, self.parent, self.tok, self.out, self.t, self.last_live,
                        self.B, self.K, V, self.end_idx, self.pad_idx)
        for phase in (0, 1):
            ops.beam_reorder(self._table, self._n_buffers, self._n_blocks, self.parent, self.R, self.K, self.t, phase)

    def _all_done(self, i):
        return int(self.last_live) < i + 1

    def result(self):
        """(what run() returns) -> (tokens (B, K, n + 1), raw scores (B, K), n): the beams after the step at which every
        beam had finished"""
        n = self.steps_run
        last = int(self.last_live)
        if last < n:
            n = last + 1
        return self.out[:, :n + 1].view(self.B, self.K, n + 1).clone(), self.scores.view(self.B, self.K).clone(), n


# ---------------------------------------------------------------------------------------------------- group beam search
# Diverse beam search (Vijayakumar et al. 2018; elsewhere `num_beam_groups` with a diversity penalty).  Rules (both paths --
# bmhrl_group_beam_select in the captured token step, _group_beam_rerun over re-runs -- implement exactly these).  Inputs:
# K beams per sample, G groups (beam_groups; G divides K, K' = K / G), lambda = diversity_penalty (finite, >= 0; the fp32
# value of the host float).
#  G1. group g owns beams g*K' .. g*K' + K' - 1 of its sample.  The first beam of every group starts live with score 0 and
#      input start_idx, the group's other beams start finished with score -inf;
#  G2. at a step the groups choose in the order g = 0 .. G-1.  c_g(v) = the number of beams of groups 0 .. g-1 of the same
#      sample whose choice at this step was a candidate (k, v) of a live beam -- for any v, end_idx and pad_idx included; a
#      finished beam's pad candidate counts for nothing.  c_0 = 0;
#  G3. a live beam k of group g offers V candidates (k, v) with the score s = score_k + lp(k, v) (one fp32 add, as beam rule
#      2) and the selection value a = s - lambda * c_g(v): c converted to fp32, one fp32 multiply, then one fp32 subtract, no
#      FMA contraction.  Where c = 0, a is s bit for bit (-inf included); where the product overflows, IEEE decides.  A
#      finished beam offers the single candidate (k, pad_idx) with a = s = score_k, never penalised;
#  G4. the K' best candidates of group g by a become the group's beams, best first, ties to the smaller k*V + v (a stable
#      sort of -a over the group's candidates): a beam's parent is always in its own group.  The new beam's score is s, not
#      a -- the penalty steers the choice and is never added to a score, so scores stay sums of (rule-adjusted) log-probs and
#      beam rule 5, return_scores and the teacher-forced check keep their meaning.  Choosing end_idx finishes a beam;
#  G5. beam rules 4-6 then apply over all K beams of the sample (the stop, n_k, the choice by length-normalised score with
#      ties to the lower beam index, the result layout), and consensus R1-R7 with select="consensus".
# G = 1 is beam search for every lambda (and takes the beam search section's own code).  lambda = 0 makes every group the
# same K'-beam search: beam g*K' + j equals beam j of beam_size = K', tokens and scores bit for bit.
# Refused with ValueError: G < 1 or no integer, K % G != 0, lambda negative or non-finite (as fp32 too), return_groups
# without return_beams.


def _group_args(K, beam_groups=1, diversity_penalty=0.0, return_groups=False, return_beams=True):
    """(G, lambda as the fp32 value the kernel sees) of valid arguments"""
    try:
        whole = not isinstance(beam_groups, bool) and int(beam_groups) == beam_groups
    except (TypeError, ValueError, OverflowError):
        whole = False
    if not whole or int(beam_groups) < 1:
        raise ValueError(f"beam_groups must be an integer >= 1, got {beam_groups!r}")
    G = int(beam_groups)
    if K % G:
        raise ValueError(f"beam_groups must divide beam_size: {K} beams in {G} groups")
    try:
        lam = float(diversity_penalty)
    except (TypeError, ValueError):
        raise ValueError(f"diversity_penalty must be finite and >= 0, got {diversity_penalty!r}") from None
    if not (math.isfinite(lam) and lam >= 0 and math.isfinite(_f32(lam))):
        raise ValueError(f"diversity_penalty must be finite and >= 0, got {diversity_penalty}")
    if return_groups and not return_beams:
        raise ValueError("return_groups needs return_beams")
    return G, _f32(lam)


def _group_beam_rerun(model, fs, max_len, start_idx, end_idx, pad_idx, modality, K, G, penalty, rules=None, trace=None,
                      context=None):
    """rules G1-G4 and beam rule 4 over full re-runs of model.inference on the prefix batch -> (tokens (B, K, n + 1),
    scores (B, K), n); rules: what _rule_args returned, context: what _context returned.  trace: a list that receives one dict per step -- the step's log-probs
    `logp` (B, K, V), the `scores` / `finished` it started from and, after it, `parent`, `tok`, `new_scores`, `new_finished`
    (B, K) and the beams `hist` (B, K, step + 2)."""
    B = fs['audio'].shape[0]
    dev = fs['audio'].device
    Kp = K // G
    rep, x = _rerun_setup(fs, K)
    scores = torch.full((B, K), float("-inf"), device=dev)
    scores[:, ::Kp] = 0.0
    finished = torch.ones(B, K, dtype=torch.bool, device=dev)
    finished[:, ::Kp] = False
    hist = torch.full((B * K, 1), start_idx, dtype=torch.long, device=dev)
    lam = torch.tensor(penalty, dtype=torch.float32, device=dev)
    steps = 0
    while steps < max_len:
        lp = _rerun_logp(model, x, rep, hist, modality, pad_idx)
        if context is not None:
            lp = _apply_context_rules(lp, hist, steps, rules, end_idx, pad_idx, context[0], K, context[1])
        elif rules is not None:
            lp = _apply_rules(lp, hist, steps, *rules, end_idx, pad_idx)
        V = lp.shape[-1]
        cand = scores.unsqueeze(-1) + lp.view(B, K, V)
        only = torch.zeros_like(cand)
        only[..., pad_idx] = scores
        cand = torch.where(finished.unsqueeze(-1), only, cand)                 # s of every candidate (B, K, V)
        count = torch.zeros(B, V, device=dev)                                  # c_g(v), exact in fp32
        parent, tok, new_scores = [], [], []
        for g in range(G):
            s_g, fin_g = cand[:, g * Kp:(g + 1) * Kp], finished[:, g * Kp:(g + 1) * Kp]
            pen = count * lam                                                  # one multiply, then one subtract
            a = torch.where(fin_g.unsqueeze(-1) | (count == 0).unsqueeze(1), s_g, s_g - pen.unsqueeze(1))
            pick = _stable_top(a.reshape(B, Kp * V), fin_g, pad_idx)
            p_g, t_g = pick // V, pick % V
            count.scatter_add_(1, t_g, (~fin_g.gather(1, p_g)).to(count.dtype))
            parent.append(p_g + g * Kp)
            tok.append(t_g)
            new_scores.append(s_g.reshape(B, Kp * V).gather(1, pick))
        parent, tok, new_scores = torch.cat(parent, 1), torch.cat(tok, 1), torch.cat(new_scores, 1)
        step = dict(logp=lp.view(B, K, V), scores=scores, finished=finished) if trace is not None else None
        scores = new_scores
        finished = finished.gather(1, parent) | (tok == end_idx)
        hist = hist.view(B, K, -1).gather(1, parent.unsqueeze(-1).expand(-1, -1, hist.shape[-1])).view(B * K, -1)
        hist = torch.cat([hist, tok.view(B * K, 1)], 1)
        steps += 1
        if trace is not None:
            step.update(parent=parent, tok=tok, new_scores=scores, new_finished=finished, hist=hist.view(B, K, -1))
            trace.append(step)
        if bool(finished.all()):
            break
    return hist.view(B, K, -1), scores, steps


class GroupBeamDecoder(BeamDecoder):
    """BeamDecoder with bmhrl_group_beam_select (csrc/beam.hip, the grouped select: rules G2-G4 for all groups, one launch) in place of
    bmhrl_beam_select; the two reorder launches, the per-beam buffers, the constraints launch and the result are
    BeamDecoder's, so the token step has no launch more than plain beam search.  beam_groups / diversity_penalty are launch
    arguments: set_params() captures the step again when they change, as SampleDecoder's.  A decoder from for_batch starts
    with G = 1, lambda = 0; _incremental sets both before every clip batch."""

    _cache_attr = "_group_beam_decoders"

    def __init__(self, agent, B, tv_cap, ta_cap, max_len, start_idx, end_idx, pad_idx, device, beams=4, beam_groups=1,
                 diversity_penalty=0.0):
        self.params = _group_args(int(beams), beam_groups, diversity_penalty)
        super().__init__(agent, B, tv_cap, ta_cap, max_len, start_idx, end_idx, pad_idx, device, beams=beams)

    def set_params(self, beam_groups, diversity_penalty):
        """not while a clip batch is being decoded: the beams of rule G1 are laid out by the begin() that follows"""
        params = _group_args(self.K, beam_groups, diversity_penalty)
        if params != self.params:
            self.params = params
            if self.graph is not None:
                # eager once: another K' is another kernel, whose first launch is not one under capture.  It writes the
                # search state as the last decode left it; begin() resets all of it before it is used again
                self._select()
                self._capture()

    def _reset(self):
        super()._reset()
        Kp = self.K // self.params[0]
        self.scores.view(self.B, self.K)[:, ::Kp] = 0.0
        self.finished.view(self.B, self.K)[:, ::Kp] = 0

    def _select(self):
        V = self.logp.shape[-1]
        ops.group_beam_select(self.logp, V, self.scores, self.finished, self.parent, self.tok, self.out, self.t, self.last_live,
                              self.B, self.K, V, self.end_idx, self.pad_idx, *self.params)

    def _choose(self, logp):
        self._select()
        for phase in (0, 1):
            ops.beam_reorder(self._table, self._n_buffers, self._n_blocks, self.parent, self.R, self.K, self.t, phase)


# ------------------------------------------------------------------------------------------------------------- sampling
# Rules (both paths below implement exactly these).  Inputs: n >= 1 samples per clip, temperature T >= 0, top_k >= 0,
# 0 < top_p <= 1, seed, length_penalty.
#  1. clip b owns the n rows b*n .. b*n + n - 1 (sample-major, as beams); every row starts live with input start_idx and
#     sum_logp = 0;
#  2. at step t a live row has the model's fp32 log-probs lp (V values).  T = 0: the arg-max (the first maximum, as
#     torch.argmax).  T > 0: q_v = exp((lp_v - max lp) / T);
#  3. the order is lp descending, ties to the smaller token id.  top_k keeps the first k tokens of the order (k = 0 or
#     k >= V: all); top_p keeps the shortest prefix of the order whose q-mass is >= top_p * sum q (top_p = 1: all); with
#     both, the shorter prefix.  At least one token is kept;
#  4. u = uniform01(seed + seed_word, ((row_offset + row) << 16) + t), the generator of csrc/common.h.  Walking the kept
#     tokens in increasing token id and accumulating q, the pick is the first token of positive q whose inclusive sum is
#     > u * kept_mass; if rounding leaves none, the last kept token of positive q;
#  5. the pick's model log-prob lp_v (independent of T) is added to sum_logp and recorded with its sampling log-prob
#     log(q_v / kept_mass) (0 for an arg-max pick) and the token (history column t + 1).  Picking end_idx finishes the row;
#     a finished row emits pad_idx and adds nothing;
#  6. stop after the step at which every row has finished, or after max_len steps; n_k = generated tokens up to and
#     including the first end_idx (the steps run if none), as beam rule 5;
#  7. the result is int64 (B, m + 1): with n = 1 the sample itself, with n > 1 per clip the row with the largest
#     sum_logp / ((5 + n_k) / 6) ** length_penalty, ties to the lower row; pad_idx after its end; m = max n_k of the chosen.
# T = 0, top_k = 1 and a tiny top_p each give greedy's tokens with pad_idx after each row's first end token; T = 1, k = 0,
# p = 1 is the reference's Categorical(exp(lp)) draw (epoch_loops/captioning_bmrl_loops.py:543-583), padded after the end.
# Rows without a finite log-prob take the arg-max (their q is undefined).

_U64 = 2 ** 64


def uniform01(seed, idx):
    """numpy mirror of hash_u32 / uniform01 of csrc/common.h (uint64 wraparound): float64 values of the fp32 draws"""
    import numpy as np
    s = np.uint64(int(seed) % _U64)
    z = np.asarray(idx, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z * np.uint64(0x9E3779B97F4A7C15) + s
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(40)).astype(np.float64)) / 16777216.0          # (hash >> 32) >> 8, times 2^-24: exact in fp32


def _sample_args(n, temperature, top_k, top_p):
    n, top_k = int(n), int(top_k)
    temperature, top_p = float(temperature), float(top_p)
    if n < 1:
        raise ValueError(f"n must be >= 1, got {n}")
    if not (temperature >= 0 and math.isfinite(temperature)):
        raise ValueError(f"temperature must be finite and >= 0, got {temperature}")
    if top_k < 0:
        raise ValueError(f"top_k must be >= 0, got {top_k}")
    if not 0 < top_p <= 1:
        raise ValueError(f"top_p must lie in (0, 1], got {top_p}")
    return n, temperature, top_k, top_p


def _f32(x):
    """the fp32 value the kernel sees for a host float"""
    return torch.tensor(x, dtype=torch.float32).item()


def sample_decode(model, feature_stacks, max_len, start_idx, end_idx, pad_idx, modality, n=1, temperature=1.0, top_k=0,
                  top_p=1.0, seed=None, length_penalty=0.0, return_samples=False, incremental=None, no_repeat_ngram=0,
                  min_len=0, repetition_penalty=1.0, select="logp", consensus_n=4, consensus_weight=None, context=None,
                  context_ngram=0, context_penalty=1.0):
    """Sampled decoding with the reference decoder's arguments (rules above).  Returns tokens (B, m + 1) int64 (rule 7), then
    -- with return_samples -- all samples (B, n, m' + 1), their sum_logp (B, n) fp32 and the per-step model / sampling
    log-probs (B, n, m') fp32 (m': the steps of rule 6; zeros after a row's end).  seed=None draws one from `random`.
    incremental (default: on under the conditions beam_decode takes BeamDecoder, n <= 16) decodes through SampleDecoder;
    otherwise every step re-runs model.inference over the (B*n)-row prefix batch in float64 (any model, CPU included).
    no_repeat_ngram / min_len / repetition_penalty: the constraints section's rules; the draw and every returned log-prob
    are then taken from the adjusted values, and a max_len + 1 above ops.LOGIT_RULES_MAX_HIST (256) takes the re-run path.
    select="consensus" (with consensus_n = N in [1, 4] and consensus_weight = None or a (V,) tensor of token weights)
    replaces rule 7's choice by the consensus section's: the returned tokens are the sample with the largest utility, and
    return_samples appends the samples' utilities (B, n) fp64, in the samples' order, as the LAST (sixth) element of the
    tuple.  With select="logp" (the default) the tuple is as described above.
    context / context_ngram / context_penalty: the context rules C1-C5 of the constraints section; the n samples of a clip
    share the clip's context."""
    n, temperature, top_k, top_p = _sample_args(n, temperature, top_k, top_p)
    rules = _rule_args(no_repeat_ngram, min_len, repetition_penalty, max_len)
    consensus = _consensus_args(select, consensus_n, consensus_weight)
    seed = random.getrandbits(62) if seed is None else int(seed) % _U64
    with torch.no_grad():
        context = _context(context, context_ngram, context_penalty, feature_stacks['audio'].shape[0], pad_idx,
                           feature_stacks['audio'].device)
        dec = _incremental(SampleDecoder, model, feature_stacks, modality, max_len, start_idx, end_idx, pad_idx, n, incremental,
                           params=(temperature, top_k, top_p), rules=rules, context=context)
        found = dec.run(seed) if dec is not None else _sample_rerun(model, feature_stacks, max_len, start_idx, end_idx, pad_idx,
                                                                    modality, n, temperature, top_k, top_p, seed, rules,
                                                                    context)
        if consensus is None:
            return _sample_result(*found, end_idx, length_penalty, return_samples)
        util = _consensus_utilities(dec, found[0], found[4], end_idx, *consensus)
        return _sample_result(*found, end_idx, length_penalty, return_samples, util)


def sample_decoder(n=1, temperature=1.0, top_k=0, top_p=1.0, seed=None, length_penalty=0.0, no_repeat_ngram=0, min_len=0,
                   repetition_penalty=1.0, select="logp", consensus_n=4, consensus_weight=None, context_ngram=0,
                   context_penalty=1.0):
    """a decoder with the reference's signature (model, feature_stacks, max_len, start_idx, end_idx, pad_idx, modality), e.g.
    validation_1by1_loop(cfg, model, loader, sample_decoder(4, top_p=0.9), epoch, TBoard); seed=None: a fresh seed per call;
    select / consensus_n / consensus_weight: the consensus section's choice among the n samples, e.g.
    sample_decoder(8, top_p=0.9, select="consensus"); context_ngram / context_penalty: the context rules, for the contexts
    handed over with the optional keyword context= (as greedy_decoder)"""
    n, temperature, top_k, top_p = _sample_args(n, temperature, top_k, top_p)
    rules = _rule_args(no_repeat_ngram, min_len, repetition_penalty) or _NO_RULES
    _consensus_args(select, consensus_n, consensus_weight)
    crules = _context_args(context_ngram, context_penalty) or _NO_CONTEXT_RULES

    def decoder(model, feature_stacks, max_len, start_idx, end_idx, pad_idx, modality, context=None):
        return sample_decode(model, feature_stacks, max_len, start_idx, end_idx, pad_idx, modality, n=n,
                             temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, length_penalty=length_penalty,
                             no_repeat_ngram=rules[0], min_len=rules[1], repetition_penalty=rules[2], select=select,
                             consensus_n=consensus_n, consensus_weight=consensus_weight, context=context,
                             context_ngram=crules[0], context_penalty=crules[1])
    return decoder


def _sample_choose(lp, temperature, top_k, top_p, u):
    """rules 2-4 in float64 for every row of lp (R, V) with draws u (R,) -> (picks (R,) int64, sampling log-probs (R,))"""
    R, V = lp.shape
    lp = torch.nan_to_num(lp.double(), nan=float("-inf"), posinf=float("inf"))
    arg = lp.argmax(1)
    zero = torch.zeros(R, dtype=torch.float64, device=lp.device)
    T, p = _f32(temperature), _f32(top_p)
    if T == 0 or top_k == 1:
        return arg, zero
    M = lp.max(1, keepdim=True).values
    dead = ~torch.isfinite(M.squeeze(1))
    finite = torch.isfinite(lp)
    q = torch.where(finite, torch.exp((lp - M) / T), torch.zeros_like(lp))
    kept = torch.ones_like(finite)
    if 0 < top_k < V or p < 1:
        order = torch.sort(-lp, dim=1, stable=True).indices
        cum = q.gather(1, order).cumsum(1)
        c = torch.full((R,), V, dtype=torch.long, device=lp.device)
        if 0 < top_k < V:
            c.clamp_(max=top_k)
        if p < 1:
            c = torch.minimum(c, ((cum < p * cum[:, -1:]).sum(1) + 1).clamp(max=V))
        kept = torch.zeros_like(finite).scatter(1, order, torch.arange(V, device=lp.device).unsqueeze(0) < c.unsqueeze(1))
    incl = torch.where(kept, q, torch.zeros_like(q)).cumsum(1)
    mass = incl[:, -1]
    cand = kept & (q > 0)
    hit = cand & (incl > (u.double() * mass).unsqueeze(1))
    last = V - 1 - cand.flip(1).to(torch.uint8).argmax(1)
    pick = torch.where(hit.any(1), hit.to(torch.uint8).argmax(1), last)
    logq = (lp.gather(1, pick.unsqueeze(1)).squeeze(1) - M.squeeze(1)) / T - torch.log(mass)
    return torch.where(dead, arg, pick), torch.where(dead, zero, logq)


def _sample_rerun(model, fs, max_len, start_idx, end_idx, pad_idx, modality, n, temperature, top_k, top_p, seed, rules=None,
                  context=None):
    """rules 1-6 over full re-runs of model.inference on the (B*n)-row prefix batch -> (tokens (B, n, steps + 1),
    sum_logp (B, n), step logp (B, n, steps), step logq (B, n, steps), steps); rules: what _rule_args returned, context:
    what _context returned"""
    import numpy as np
    B = fs['audio'].shape[0]
    dev = fs['audio'].device
    R = B * n
    rep, x = _rerun_setup(fs, n)
    fin = torch.zeros(R, dtype=torch.bool, device=dev)
    hist = torch.full((R, 1), start_idx, dtype=torch.long, device=dev)
    sum_logp = torch.zeros(R, dtype=torch.float64, device=dev)
    slp, slq = [], []
    rows = np.arange(R, dtype=np.uint64) << np.uint64(16)
    steps = 0
    while steps < max_len:
        lp = _rerun_logp(model, x, rep, hist, modality, pad_idx)
        if context is not None:
            lp = _apply_context_rules(lp, hist, steps, rules, end_idx, pad_idx, context[0], n, context[1])
        elif rules is not None:
            lp = _apply_rules(lp, hist, steps, *rules, end_idx, pad_idx)
        lp = lp.double()
        u = torch.from_numpy(uniform01(seed, rows + np.uint64(steps))).to(dev)
        pick, logq = _sample_choose(lp, temperature, top_k, top_p, u)
        g = lp.gather(1, pick.unsqueeze(1)).squeeze(1)
        pick = torch.where(fin, torch.full_like(pick, pad_idx), pick)
        g, logq = torch.where(fin, torch.zeros_like(g), g), torch.where(fin, torch.zeros_like(logq), logq)
        sum_logp += g
        slp.append(g)
        slq.append(logq)
        hist = torch.cat([hist, pick.unsqueeze(1)], 1)
        fin |= pick == end_idx
        steps += 1
        if bool(fin.all()):
            break
    f32 = lambda a: a.float().view(B, n, -1)
    return (hist.view(B, n, -1), sum_logp.float().view(B, n), f32(torch.stack(slp, 1)), f32(torch.stack(slq, 1)), steps)


def _sample_result(toks, sum_logp, step_logp, step_logq, steps, end_idx, length_penalty, return_samples, util=None):
    """rules 6-7 over (B, n, >= steps + 1) samples; util: the samples' consensus utilities (B, n) -- the choice is then
    consensus rule R7 over rule 7's order"""
    toks = toks[..., :steps + 1]
    n_k, order, out = _best_hypothesis(toks, sum_logp, steps, end_idx, length_penalty)
    if util is not None:
        out = _consensus_choice(toks, n_k, order, util)[1]
    if not return_samples:
        return out
    found = (out, toks.clone(), sum_logp.clone(), step_logp[..., :steps].clone(), step_logq[..., :steps].clone())
    return found if util is None else found + (util,)


class SampleDecoder(IncrementalDecoder):
    """IncrementalDecoder's token step on B*n rows (sample-major; the per-clip memory K|V is shared, its attentions take a
    clip's n rows as n queries, as BeamDecoder's), followed by one bmhrl_sample_step launch inside the same captured graph
    (csrc/sample.hip: rules 2-5 for every row).  Rows never change parents, so nothing is reordered.  The draw's seed is a
    device word written before every decode: a cached graph draws fresh samples for a new seed and repeats them for the
    same seed.  temperature / top_k / top_p are launch arguments: set_params() captures the step again when they change."""

    _cache_attr = "_sample_decoders"

    @classmethod
    def _fits(cls, model, rows):
        return rows <= ops.BEAM_MAX and 1 <= getattr(model, "voc_size", 0) <= ops.SAMPLE_MAX_V

    def __init__(self, agent, B, tv_cap, ta_cap, max_len, start_idx, end_idx, pad_idx, device, beams=1, temperature=1.0,
                 top_k=0, top_p=1.0):
        if not 1 <= beams <= ops.BEAM_MAX:
            raise ValueError(f"SampleDecoder: {beams} samples per clip outside [1, 16]")
        if not 1 <= agent.voc_size <= ops.SAMPLE_MAX_V:
            raise ValueError(f"SampleDecoder: vocabulary of {agent.voc_size} outside [1, {ops.SAMPLE_MAX_V}]")
        self.params = _sample_args(beams, temperature, top_k, top_p)[1:]
        super().__init__(agent, B, tv_cap, ta_cap, max_len, start_idx, end_idx, pad_idx, device, beams=beams)

    def set_params(self, temperature, top_k, top_p):
        params = _sample_args(self.K, temperature, top_k, top_p)[1:]
        if params != self.params:
            self.params = params
            if self.graph is not None:
                self._capture()

    def _init_search(self):
        R, dev, L = self.R, self.dev, self.max_len + 1
        self.sum_logp = torch.zeros(R, device=dev)
        self.step_logp = torch.zeros(R, L, device=dev)          # column t: step t (same row stride as `out`)
        self.step_logq = torch.zeros(R, L, device=dev)
        self.seed_word = torch.zeros(1, dtype=torch.int64, device=dev)

    def _reset(self):
        super()._reset()
        self.sum_logp.zero_()
        self.step_logp.zero_()
        self.step_logq.zero_()

    def _choose(self, logp):
        V = self.logp.shape[-1]
        T, k, p = self.params
        ops.sample_step(self.logp, V, self.R, V, T, k, p, 0, self.seed_word, self.t, self.end_idx, self.pad_idx, self.done,
                        self.tok, self.out, self.sum_logp, self.step_logp, self.step_logq)

    def run(self, seed=0):
        s = int(seed) % _U64
        self.seed_word.fill_(s - _U64 if s >= 2 ** 63 else s)
        return super().run()

    def result(self):
        """(what run() returns) -> (tokens (B, n, m + 1), sum_logp (B, n), step logp (B, n, m), step logq (B, n, m), m): the
        samples after the step at which every row had finished"""
        m = self._steps_to_end()
        B, n = self.B, self.K
        return (self.out[:, :m + 1].reshape(B, n, m + 1).clone(), self.sum_logp.view(B, n).clone(),
                self.step_logp[:, :m].reshape(B, n, m).clone(), self.step_logq[:, :m].reshape(B, n, m).clone(), m)


# ------------------------------------------------------------------------------------------------------------ consensus
# Rules (both paths -- bmhrl_consensus after the incremental decoders' token loop, consensus_host after the re-runs --
# implement exactly these).  select="consensus" keeps, per clip, the hypothesis that agrees most with the clip's other
# hypotheses (minimum-Bayes-risk choice with an n-gram utility) instead of the one with the best length-normalised log-prob.
# Inputs: the hypotheses of a clip toks (B, K, m + 1) int64, column 0 the start token; end_idx; the largest gram length
# N in [1, 4] (consensus_n); optionally token_weight (V,) fp32 (consensus_weight).
#  R1. words.  The words of hypothesis k are the tokens of columns 1 .. m before its first end_idx; the end token itself is
#      not a word, and a hypothesis without one has all m tokens as words.  Every token before the end is a word whatever its
#      id, pad_idx included.  l_k = the number of words, possibly 0;
#  R2. grams and weights.  For g = 1 .. N the g-grams of k are its l_k - g + 1 runs of g consecutive words (none if l_k < g);
#      c_k(y) = how often gram y occurs in k.  Without token_weight w(y) = 1.  With it, in fp64,
#      w(y) = (w[y_0] + ... + w[y_{g-1}]) / g: the fp32 weights widened, added in token order, the division last.  A token
#      id outside [0, V) weighs 0 and still compares by its id.  Weights are finite and >= 0 (the caller's contract);
#  R3. gram mass.  W_k^g = sum of w(y) * c_k(y) over the distinct grams of k in the order of their first occurrence in k;
#  R4. clipped match.  M_g(i, j) = sum of w(y) * min(c_i(y), c_j(y)) over the distinct grams of i in the order of their
#      first occurrence in i;
#  R5. pairwise utility.  u(i, j) = (t_1 + ... + t_N) / N with t_g = M_g(i, j) / max(W_i^g, W_j^g) when that maximum is > 0,
#      else 0; the terms are added for g = 1 .. N in that order.  All arithmetic is fp64 without FMA contraction: one product,
#      then one add;
#  R6. utility.  U_i = (sum of u(i, j) over j != i, j ascending) / (K - 1); with K = 1, U_0 = 0.  Identical hypotheses vote
#      separately (the Monte-Carlo estimate of the expected utility, intended).  Every row of the clip is a hypothesis, a
#      beam that never came alive (score -inf: fewer candidates than beams) included;
#  R7. the choice.  The clip's hypotheses are arranged in the order of sampling rule 7 / beam rule 5, best first; the largest
#      U wins, ties to the earlier hypothesis of that order (a stable sort of -U over the arranged hypotheses).  The returned
#      caption is cut and padded as without the keyword: (B, n + 1), n = max n_k of the chosen.
# Without weights every product and sum of R3 / R4 is a small integer and u a sum of N quotients of integers; with weights the
# prescribed order fixes every rounding: the device and the host compute the same IEEE operations, and their results are
# compared for equality.  Refused with ValueError: a select other than "logp" / "consensus", consensus_n outside [1, 4] or no
# integer, a consensus_weight that is no 1-D floating-point tensor with at least one entry.  With select="logp" (the default)
# nothing of this section runs.


def _consensus_args(select, consensus_n, consensus_weight):
    """(N, weight) of valid arguments with select="consensus", None with select="logp" (the arguments are checked alike)"""
    if select not in ("logp", "consensus"):
        raise ValueError(f"select must be 'logp' or 'consensus', got {select!r}")
    try:
        whole = not isinstance(consensus_n, bool) and int(consensus_n) == consensus_n
    except (TypeError, ValueError, OverflowError):
        whole = False
    if not whole or not 1 <= int(consensus_n) <= ops.CONSENSUS_MAX_N:
        raise ValueError(f"consensus_n must be an integer in [1, {ops.CONSENSUS_MAX_N}], got {consensus_n!r}")
    w = consensus_weight
    if w is not None and not (torch.is_tensor(w) and w.dim() == 1 and w.numel() >= 1 and w.is_floating_point()):
        raise ValueError("consensus_weight must be None or a (V,) floating-point tensor of token weights")
    return None if select == "logp" else (int(consensus_n), w)


def _consensus_utilities(dec, toks, steps, end_idx, N, weight):
    """R1-R6 -> U (B, K) fp64 on the hypotheses' device.  dec: the incremental decoder whose run() produced toks (its history
    `out` still holds them: one bmhrl_consensus launch), None after a re-run (the host path; also for a history longer than
    the kernel's ops.CONSENSUS_MAX_STEPS)."""
    if dec is not None and steps <= ops.CONSENSUS_MAX_STEPS:
        w = None if weight is None else weight.detach().to(device=dec.dev, dtype=torch.float32).contiguous()
        return ops.consensus(dec.out, steps, dec.K, end_idx, N, w)
    return consensus_host(toks[..., :steps + 1], end_idx, N, weight)


def consensus_host(toks, end_idx, n=4, token_weight=None, pair=False):
    """R1-R6 on the host for hypotheses toks (B, K, m + 1) int64 -> U (B, K) fp64 on toks' device [, with pair=True, the
    pairwise utilities (B, K, K), u(i, i) = 0].  Python floats are IEEE doubles and `a + b * c` is one product, then one add,
    so this is the arithmetic of the rules; the grams of a hypothesis are the keys of a dict, which keeps them in the order
    of their first occurrence."""
    t = toks.detach().cpu().tolist()
    B, K = toks.shape[:2]
    w32 = None if token_weight is None else [float(x) for x in token_weight.detach().to("cpu", torch.float32).tolist()]
    V = 0 if w32 is None else len(w32)
    util = [[0.0] * K for _ in range(B)]
    pairs = [[[0.0] * K for _ in range(K)] for _ in range(B)]
    for b in range(B):
        words = []
        for k in range(K):
            row = t[b][k][1:]
            words.append(row[:row.index(end_idx)] if end_idx in row else row)
        u = pairs[b]
        for g in range(1, n + 1):
            weight, tables, mass = {}, [], []
            for ws in words:
                count = {}
                for p in range(len(ws) - g + 1):
                    gram = tuple(ws[p:p + g])
                    count[gram] = count.get(gram, 0) + 1
                    if gram not in weight:
                        s = 1.0
                        if w32 is not None:
                            s = 0.0 + (w32[gram[0]] if 0 <= gram[0] < V else 0.0)
                            for v in gram[1:]:
                                s = s + (w32[v] if 0 <= v < V else 0.0)
                            s = s / float(g)
                        weight[gram] = s
                W = 0.0
                for gram, c in count.items():
                    W = W + weight[gram] * float(c)
                tables.append(count)
                mass.append(W)
            for i in range(K):
                for j in range(K):
                    if j == i:
                        continue
                    M = 0.0
                    for gram, c in tables[i].items():
                        M = M + weight[gram] * float(min(c, tables[j].get(gram, 0)))
                    mx = max(mass[i], mass[j])
                    u[i][j] = u[i][j] + (M / mx if mx > 0 else 0.0)
        for i in range(K):
            s = 0.0
            for j in range(K):
                if j != i:
                    u[i][j] = u[i][j] / float(n)
                    s = s + u[i][j]
            util[b][i] = s / float(K - 1) if K > 1 else 0.0
    U = torch.tensor(util, dtype=torch.float64, device=toks.device).view(B, K)
    return (U, torch.tensor(pairs, dtype=torch.float64, device=toks.device).view(B, K, K)) if pair else U


def _consensus_choice(toks, n_k, order, util):
    """R7 over (B, K, >= n + 1) hypotheses, their n_k, their order (best first, of _best_hypothesis) and their utilities (B, K)
    -> (the chosen hypotheses' indices (B,), their tokens (B, n + 1))"""
    B = util.shape[0]
    by_util = torch.sort(-util.gather(1, order), dim=1, stable=True).indices[:, :1]
    pick = order.gather(1, by_util).squeeze(1)
    rows = torch.arange(B, device=util.device)
    n = int(n_k[rows, pick].max()) if B else 0
    return pick, toks[rows, pick, :n + 1].clone()


def idf_weights(counts, total=None):
    """token weights for consensus_weight from a (V,) tensor of token counts (e.g. train_vocab.freqs in vocabulary order):
    log(total / max(1, count)) computed in fp64, clamped at >= 0, as fp32; total=None: the sum of the counts.  Frequent
    tokens (function words) weigh little, tokens never seen weigh log(total)."""
    c = counts.detach().double()
    total = float(c.sum()) if total is None else float(total)
    if c.dim() != 1 or not total > 0:
        raise ValueError("idf_weights: counts must be a (V,) tensor and total > 0")
    return torch.log(total / c.clamp_min(1.0)).clamp_min(0.0).float()
