"""Captioning whole videos: features -> proposals -> crops -> any decoder of bmhrl_amd.decode -> the ActivityNet-captions
dictionary -- the reference's `learned_props` route, and what its sample/single_vid_bmhrl.py sketches,
without a second visit to the feature files.

The proposal generator needs the full-length, padded stacks of a video on the device.  A proposal's clip is rows `[a, b)` of
those same stacks (captioning_datasets/load_features.py:14-35), so `VideoFeatures.crop` cuts and pads all proposals of a chunk
with one ops.crop_segments call per stack (csrc/segment_crop.hip) instead of writing the proposals to a file, building a data
set over them and reading, padding and uploading overlapping slices of the same video once per proposal.

What is read on the host: the proposals themselves -- the one packed `.tolist()` of proposal_utils.device_proposal_rows; the
submission dictionary is host data -- the token ids of every chunk, and two status words per `caption_segments` call.  The
segment times are host floats when the crop sees them (rounded to 5 places, the doubles a JSON round trip of the proposal file
would hand the loader), so the width of a chunk's crop is computed there with loader.crop_bounds and the device never
truncates.
"""
from __future__ import annotations

import os
from typing import Dict, List, Sequence

import numpy as np
import torch

from . import loader as L
from .model.masking import make_masks
from .proposal_utils import rows_to_segments, select_rows

_STACKS = {"video": ("rgb", "flow"), "audio": ("audio",), "audio_video": ("rgb", "flow", "audio")}


def _unwrap(m):
    return m.module if hasattr(m, "module") else m


class VideoFeatures:
    """the full rgb / flow / audio stacks of V videos, padded to a common length per stream, with the true row counts:
    rgb, flow (V, S_video, D_video) and audio (V, S_audio, D_audio) fp32 on `device`; video_len, audio_len (V) int32 there and
    as host lists; durations (V) float64 there and as host floats.  A video whose file is missing has length 0 and a stack
    of padding: each of its segments is the loader's "missing clip" (one zero row)."""

    def __init__(self, video_ids, durations, rgb, flow, audio, video_len, audio_len, pad_idx):
        self.video_ids = list(video_ids)
        self.durations = [float(d) for d in durations]
        self.pad_idx = pad_idx
        self.stacks = {"rgb": rgb, "flow": flow, "audio": audio}
        self.device = next(t for t in self.stacks.values() if t is not None).device
        self.lens_host = {"rgb": [int(n) for n in video_len], "audio": [int(n) for n in audio_len]}
        self.lens_host["flow"] = self.lens_host["rgb"]
        video_len_dev = torch.tensor(self.lens_host["rgb"], dtype=torch.int32).to(self.device)
        self.lens = {"rgb": video_len_dev, "flow": video_len_dev,
                     "audio": torch.tensor(self.lens_host["audio"], dtype=torch.int32).to(self.device)}
        self.durations_dev = torch.tensor(self.durations, dtype=torch.float64).to(self.device)
        self.pads = {"rgb": float(pad_idx), "flow": 0.0, "audio": float(pad_idx)}

    def __len__(self):
        return len(self.video_ids)

    @classmethod
    def from_npy(cls, paths_or_cfg, video_ids, durations, pad_feats_up_to, pad_idx, device):
        """reads each feature file once.  paths_or_cfg: a config with video_features_path / audio_features_path (files
        <id>_rgb.npy, <id>_flow.npy, <id>.npy, as the loader), or per video a dict {'rgb', 'flow', 'audio'} of file paths.
        pad_feats_up_to = {'video', 'audio'}: the padded lengths.  Padding as load_features_from_npy(get_full_feat=True):
        rgb and audio with pad_idx, flow with 0; either of rgb / flow missing drops both."""
        V = len(video_ids)
        if V < 1 or len(durations) != V:
            raise ValueError("VideoFeatures.from_npy: one duration per video and at least one video expected")
        if isinstance(paths_or_cfg, (list, tuple)):
            if len(paths_or_cfg) != V:
                raise ValueError("VideoFeatures.from_npy: one dict of paths per video expected")
            paths = [dict(p) for p in paths_or_cfg]
        else:
            vp, ap = paths_or_cfg.video_features_path, paths_or_cfg.audio_features_path
            paths = [{"rgb": os.path.join(vp, f"{v}_rgb.npy"), "flow": os.path.join(vp, f"{v}_flow.npy"),
                      "audio": os.path.join(ap, f"{v}.npy")} for v in video_ids]
        files = []
        for p in paths:
            rgb, flow, aud = (L._open(p[k]) if p.get(k) else None for k in ("rgb", "flow", "audio"))
            if rgb is None or flow is None:
                rgb = flow = None
            elif rgb.shape != flow.shape:
                raise AssertionError(f"rgb / flow shapes differ: {p['rgb']} {rgb.shape} vs {p['flow']} {flow.shape}")
            files.append((rgb, flow, aud))
        pin = torch.device(device).type == "cuda"

        def stack(idx, S_pad, pad, width):
            present = [f[idx] for f in files if f[idx] is not None]
            D = present[0].shape[1] if present else width
            host = torch.full((V, S_pad, D), float(pad), dtype=torch.float32, pin_memory=pin)
            lens = []
            for v, f in enumerate(files):
                n = 0 if f[idx] is None else f[idx].shape[0]
                if n > S_pad:
                    raise ValueError(f"VideoFeatures.from_npy: {n} rows of {video_ids[v]} do not fit pad_feats_up_to = {S_pad}")
                if n:
                    host[v, :n] = torch.from_numpy(np.array(f[idx], dtype=np.float32))
                lens.append(n)
            return host.to(device, non_blocking=True), lens

        rgb, video_len = stack(0, int(pad_feats_up_to["video"]), pad_idx, L.D_VIDEO)
        flow, _ = stack(1, int(pad_feats_up_to["video"]), 0, L.D_VIDEO)
        audio, audio_len = stack(2, int(pad_feats_up_to["audio"]), pad_idx, L.D_AUDIO)
        return cls(video_ids, durations, rgb, flow, audio, video_len, audio_len, pad_idx)

    def feature_stacks(self) -> Dict[str, torch.Tensor]:
        """the full-length stacks, as the proposal generator takes them"""
        return dict(self.stacks)

    def crop(self, seg_video: Sequence[int], seg_times: Sequence[Sequence[float]], modality: str = "audio_video",
             return_status: bool = False):
        """the `feature_stacks` dictionary of the P clips (video seg_video[p], seg_times[p] = (start s, end s)) a decoder
        takes: per stack of the modality (P, T, D), T the longest crop of the chunk (loader.crop_bounds on the host; at least
        1), one ops.crop_segments call each -- loader.crop_segments_host when the stacks are on the CPU.  The status words
        are not read here: with return_status the (n_stacks, 2) int32 tensor of them comes back as well, for a caller that
        checks them once."""
        try:
            names = _STACKS[modality]
        except KeyError:
            raise ValueError(f"unknown modality {modality}") from None
        P, V = len(seg_video), len(self)
        if P < 1 or len(seg_times) != P:
            raise ValueError("VideoFeatures.crop: at least one segment, and one (start, end) per segment, expected")
        times = [(float(s), float(e)) for s, e in seg_times]
        on_device = self.device.type == "cuda"
        if on_device:
            from . import ops
            video = torch.tensor([int(v) for v in seg_video], dtype=torch.int32).to(self.device, non_blocking=True)
            times_dev = torch.tensor(times, dtype=torch.float64).to(self.device, non_blocking=True)
        feats, status = {}, []
        widths = {}
        for name in names:
            lens = self.lens_host[name]
            key = id(lens)                     # rgb and flow share their lengths
            if key not in widths:
                widths[key] = max([1] + [L.crop_rows(lens[v], s, e, self.durations[v])[1]
                                         for v, (s, e) in zip(seg_video, times) if 0 <= v < V])
            if on_device:
                out, _, _, st = ops.crop_segments(self.stacks[name], self.lens[name], self.durations_dev, video, times_dev,
                                                  self.pads[name], widths[key])
            else:
                out, _, _, st = L.crop_segments_host(self.stacks[name], lens, self.durations, seg_video, times, self.pads[name],
                                                     widths[key])
            feats[name] = out
            status.append(st)
        return (feats, torch.stack(status)) if return_status else feats


def _token_ids(cfg, vocab_or_dataset):
    """(itos, start_idx, end_idx, pad_idx) of a data set (the reference's: train_vocab and the three indices) or of a
    vocabulary with itos / stoi and the config's token strings"""
    x = vocab_or_dataset
    if hasattr(x, "train_vocab"):
        return x.train_vocab.itos, x.start_idx, x.end_idx, x.pad_idx
    return x.itos, x.stoi[cfg.start_token], x.stoi[cfg.end_token], x.stoi[cfg.pad_token]


PARAGRAPH_MAX_CONTEXT = 1024          # ops.LOGIT_RULES_MAX_CTX: the entries of a clip's context


def caption_tokens(row, end_idx, pad_idx):
    """the words of a decoded row as a context sentence: the generated tokens after the start token, up to but without the
    first end_idx, pads dropped"""
    words = [int(v) for v in row[1:]]
    if end_idx in words:
        words = words[:words.index(end_idx)]
    return [v for v in words if v != pad_idx]


def paragraph_context(sentences, pad_idx, context_sentences=None, limit=PARAGRAPH_MAX_CONTEXT):
    """the context of a clip from its video's earlier captions (lists of token ids, oldest first): only the last
    context_sentences of them when that is given, one pad_idx between sentences, and whole oldest sentences dropped until
    the result holds at most `limit` entries (a single sentence longer than that leaves an empty context)"""
    if context_sentences is not None:
        sentences = sentences[max(0, len(sentences) - int(context_sentences)):]
    sentences = list(sentences)
    while sentences and sum(len(x) for x in sentences) + len(sentences) - 1 > limit:
        sentences = sentences[1:]
    out = []
    for i, sent in enumerate(sentences):
        out += ([pad_idx] if i else []) + list(sent)
    return out


def caption_segments(cfg, cap_model, features: VideoFeatures, segments, decoder, vocab_or_dataset, batch_size=None,
                     paragraph=False, context_sentences=None, fill_chunks=False):
    """captions segments[v] = [(start s, end s), ...] of every video of `features`, in the given order and in chunks of at
    most batch_size (cfg.inference_batch_size) clips, with `decoder` -- any factory result of bmhrl_amd.decode -- and returns
    per video the list of {"sentence", "timestamp": [start, end]}.  The crops' status words are read once, at the end: a
    truncated or undefined crop raises.
    paragraph=True decodes in time order instead: each video's segments are ordered by (start, end,
    given index); wave w holds the w-th segment of every video that has one, videos in index order, in chunks of at most
    batch_size; and the decoder is called with the keyword context= a (clips, C) int64 tensor that holds, per clip, its
    video's w earlier captions (caption_tokens of each, oldest first, one pad_idx between sentences; only the last
    context_sentences of them when that is given; whole oldest sentences dropped until at most 1024 entries are left).  What
    the context does is the decoder's business: greedy_decoder(context_ngram=4) bans the earlier captions' 4-grams.  The
    returned lists are in the given order either way.  fill_chunks (paragraph mode only): a chunk smaller than batch_size is
    filled with copies of its last clip and the extra rows are thrown away, so that a decoder cached for the full batch
    is reused; rows are independent, so no token changes.  Off by default: section 34 measured no gain."""
    if paragraph:
        return _caption_paragraphs(cfg, cap_model, features, segments, decoder, vocab_or_dataset, batch_size,
                                   context_sentences, fill_chunks)
    from .epoch_loops.validation_loops import tokens_to_sentences
    if len(segments) != len(features):
        raise ValueError(f"caption_segments: {len(segments)} segment lists for {len(features)} videos")
    batch_size = int(cfg.inference_batch_size if batch_size is None else batch_size)
    if batch_size < 1:
        raise ValueError("caption_segments: batch_size must be >= 1")
    itos, start_idx, end_idx, pad_idx = _token_ids(cfg, vocab_or_dataset)
    flat = [(v, float(s), float(e)) for v, segs in enumerate(segments) for s, e in segs]
    results: List[List[dict]] = [[] for _ in segments]
    agent = _unwrap(cap_model)
    status = []
    with torch.no_grad():
        for i in range(0, len(flat), batch_size):
            chunk = flat[i:i + batch_size]
            fs, st = features.crop([c[0] for c in chunk], [c[1:] for c in chunk], cfg.modality, return_status=True)
            status.append(st)
            ints = decoder(agent, fs, cfg.max_len, start_idx, end_idx, pad_idx, cfg.modality)
            sentences = tokens_to_sentences(ints.cpu().numpy(), itos)
            for (v, s, e), sent in zip(chunk, sentences):
                results[v].append({"sentence": sent, "timestamp": [s, e]})
    if status:
        # (every stack of a chunk sees the same segments: the chunk's count is the largest of its stacks')
        truncated, undefined = torch.stack([st.amax(0) for st in status]).sum(0).tolist()
        if truncated or undefined:
            raise RuntimeError(f"caption_segments: {truncated} crops were truncated and {undefined} had no defined row range "
                               "(a duration that is not > 0 or a time that is not finite)")
    return results


def _caption_paragraphs(cfg, cap_model, features, segments, decoder, vocab_or_dataset, batch_size, context_sentences,
                        fill_chunks):
    """caption_segments(paragraph=True)"""
    from .epoch_loops.validation_loops import tokens_to_sentences
    if len(segments) != len(features):
        raise ValueError(f"caption_segments: {len(segments)} segment lists for {len(features)} videos")
    batch_size = int(cfg.inference_batch_size if batch_size is None else batch_size)
    if batch_size < 1:
        raise ValueError("caption_segments: batch_size must be >= 1")
    if context_sentences is not None and (isinstance(context_sentences, bool) or int(context_sentences) != context_sentences
                                          or int(context_sentences) < 0):
        raise ValueError(f"caption_segments: context_sentences must be None or an integer >= 0, got {context_sentences!r}")
    itos, start_idx, end_idx, pad_idx = _token_ids(cfg, vocab_or_dataset)
    # per video its segments in time order: (start, end, given index)
    ordered = [sorted((float(s), float(e), i) for i, (s, e) in enumerate(segs)) for segs in segments]
    results: List[List[dict]] = [[None] * len(segs) for segs in segments]
    said: List[List[List[int]]] = [[] for _ in segments]          # per video the captions so far, as token ids
    agent = _unwrap(cap_model)
    status = []
    with torch.no_grad():
        for w in range(max([0] + [len(o) for o in ordered])):
            wave = [(v, *o[w]) for v, o in enumerate(ordered) if len(o) > w]
            for i in range(0, len(wave), batch_size):
                chunk = wave[i:i + batch_size]
                n = len(chunk)
                if fill_chunks and n < batch_size:
                    chunk = chunk + [chunk[-1]] * (batch_size - n)
                fs, st = features.crop([c[0] for c in chunk], [c[1:3] for c in chunk], cfg.modality, return_status=True)
                status.append(st)
                rows = [paragraph_context(said[c[0]], pad_idx, context_sentences) for c in chunk]
                width = max([1] + [len(r) for r in rows])
                context = torch.tensor([r + [pad_idx] * (width - len(r)) for r in rows], dtype=torch.int64).view(len(rows), width)
                ints = decoder(agent, fs, cfg.max_len, start_idx, end_idx, pad_idx, cfg.modality,
                               context=context.to(features.device))
                ints = ints[:n].cpu().numpy()
                sentences = tokens_to_sentences(ints, itos)
                for (v, s, e, given), row, sent in zip(chunk[:n], ints, sentences):
                    results[v][given] = {"sentence": sent, "timestamp": [s, e]}
                    said[v].append(caption_tokens(row, end_idx, pad_idx))
    if status:
        truncated, undefined = torch.stack([st.amax(0) for st in status]).sum(0).tolist()
        if truncated or undefined:
            raise RuntimeError(f"caption_segments: {truncated} crops were truncated and {undefined} had no defined row range "
                               "(a duration that is not > 0 or a time that is not finite)")
    return results


class VideoCaptioner:
    """proposals and their captions for whole videos.  cfg: the captioning config (modality, max_len, inference_batch_size)
    with the post-processing fields of the proposal config (max_prop_per_vid, nms_tiou_thresh); prop_model: a
    MultimodalProposalGenerator; cap_model: the agent; dataset: the training data set (vocabulary and special tokens);
    decoder: a factory result of bmhrl_amd.decode, greedy when None; paragraph / context_sentences: caption_segments' -- the
    proposals of a video are captioned in time order, each with the video's earlier captions as its context."""

    def __init__(self, cfg, prop_model, cap_model, dataset, decoder=None, paragraph=False, context_sentences=None):
        if decoder is None:
            from .decode import greedy_decoder
            decoder = greedy_decoder()
        self.cfg, self.prop_model, self.cap_model, self.dataset, self.decoder = cfg, prop_model, cap_model, dataset, decoder
        self.paragraph, self.context_sentences = bool(paragraph), context_sentences

    def proposals(self, features: VideoFeatures):
        """per video the entries {"sentence": "", "proposal_score", "timestamp"} AnetPredictions.add_new_predictions would
        write for it (an empty list where it would write none)"""
        fs = features.feature_stacks()
        with torch.no_grad():
            masks = make_masks(fs, None, self.cfg.modality, self.dataset.pad_idx)
            predictions, _, _, _ = _unwrap(self.prop_model)(fs, None, masks)
        rows, _ = select_rows(predictions, self.cfg, {"duration_in_secs": features.durations})
        return [rows_to_segments(video_rows) for video_rows in rows]

    def caption(self, features: VideoFeatures, proposals, batch_size=None):
        """caption_segments on the proposals' (rounded) times; each entry keeps its proposal_score"""
        captions = caption_segments(self.cfg, self.cap_model, features, [[p["timestamp"] for p in props] for props in proposals],
                                    self.decoder, self.dataset, batch_size, paragraph=self.paragraph,
                                    context_sentences=self.context_sentences)
        for caps, props in zip(captions, proposals):
            for cap, prop in zip(caps, props):
                cap["proposal_score"] = prop["proposal_score"]
        return captions

    def predict(self, features: VideoFeatures):
        """the submission dictionary (version / external_data / results) of the videos of `features`; a video without
        proposals has no entry, as in the proposal file"""
        predictions = {"version": "VERSION 1.0", "external_data": {"used": True, "details": ""}, "results": {}}
        for video_id, caps in zip(features.video_ids, self.caption(features, self.proposals(features))):
            if caps:
                predictions["results"][video_id] = caps
        return predictions

    def predict_video(self, feature_paths: Dict[str, str], duration: float, device=None):
        """one video from its three feature files {'rgb', 'flow', 'audio'}: a list of {'start', 'end', 'sentence'}, the
        return format of the reference's sample script"""
        device = next(_unwrap(self.cap_model).parameters()).device if device is None else device
        features = VideoFeatures.from_npy([feature_paths], ["video"], [duration], self.cfg.pad_feats_up_to, self.dataset.pad_idx,
                                          device)
        caps = self.caption(features, self.proposals(features))[0]
        return [{"start": c["timestamp"][0], "end": c["timestamp"][1], "sentence": c["sentence"]} for c in caps]
