"""Counterpart of the reference's epoch_loops/validation_loops.py for the HIP-backed agent: the one-by-one (greedy decode)
validation pass and the next-word loss pass, with the reference's signatures and result format.

validation_1by1_loop (:13-137) is where the decoder spends its time: every batch is decoded token by token.  Here the
decoder is bmhrl_amd.decode (per-clip memory K|V, incremental caption K|V cache, one HIP graph per token); the host side --
ids -> words, cut at </s>, capitalise, the ActivityNet-captions result dictionary and its JSON file -- keeps the reference's
format so that its evaluator reads the file unchanged.  The file is scored by the reference's evaluator
(evaluation/evaluate.py: Java METEOR, PTB tokenizer) when that is on sys.path -- otherwise the loop returns after writing
the predictions -- or, with evaluator="device" / cfg.caption_evaluator = "device", by bmhrl_amd.evaluate on the device.

validation_learned_props_loop captions predicted proposals (the reference's `learned_props` phase) from the videos' full-length
feature stacks through bmhrl_amd.predict, and writes and scores its file the same way."""
import contextlib
import io
import json
import os
from time import time

import torch

from ..model.masking import make_masks


def _unwrap(m):
    return m.module if hasattr(m, "module") else m


def _phase_references(cfg, phase):
    """reference-caption files and tIoU thresholds of a validation phase (:34-50)"""
    single = {"val_1": 0, "val_2": 1, "vatex_val": 2, "msrvtt_val": 3}
    if phase in single:
        return [cfg.reference_paths[single[phase]]], [0.5]
    if phase == "learned_props":
        assert len(cfg.tIoUs) == 4
        return cfg.reference_paths, cfg.tIoUs
    raise ValueError(f"unknown validation phase {phase!r}")


def tokens_to_sentences(ints_stack, itos, end_token="</s>"):
    """(B, T) ids -> sentences the way the reference filters them (:63-86): drop <s>, cut at the first </s>, join, capitalise"""
    out = []
    for ints in ints_stack:
        words = [itos[int(i)] for i in ints][1:]
        if end_token in words:
            words = words[:words.index(end_token)]
        out.append(" ".join(words).capitalize())
    return out


def predict_1by1(cfg, model, loader, decoder):
    """decode every batch of the loader -> the ActivityNet-captions submission dictionary (:16-24, :53-102)"""
    predictions = {"version": "VERSION 1.0", "external_data": {"used": True, "details": ""}, "results": {}}
    ds = loader.dataset
    agent = _unwrap(model)
    for batch in loader:
        ints = decoder(agent, batch["feature_stacks"], cfg.max_len, ds.start_idx, ds.end_idx, ds.pad_idx, cfg.modality)
        sentences = tokens_to_sentences(ints.cpu().numpy(), ds.train_vocab.itos)
        for video_id, start, end, sent in zip(batch["video_ids"], batch["starts"], batch["ends"], sentences):
            seg = {"sentence": sent, "timestamp": [start.item(), end.item()]}
            predictions["results"].setdefault(video_id, []).append(seg)
    return predictions


def calculate_metrics(reference_paths, submission_path, tIoUs, max_prop_per_vid, verbose=True, only_proposals=False,
                      evaluator=None, evaluator_options=None):
    """per-tIoU and averaged scores (:160-183).  evaluator None: the reference's ANETcaptions, which needs the reference's
    evaluation package (and its Java METEOR) on sys.path -- not part of this package.  evaluator "device": this package's
    bmhrl_amd.evaluate.DenseCaptionEvaluator (what its METEOR and tokenizer are: see there), with evaluator_options as its
    keywords (device, tokenizer, stemmer, synonyms; soda=True adds SODA_c, SODA_c_Precision and SODA_c_Recall;
    proposal_recall=True adds AUC and AR@AN; tiou_backend="device" pairs and detects through the device tIoU tables;
    paragraph=True adds the paragraph-level Para_Bleu_1..4, Para_METEOR, Para_ROUGE_L, Para_CIDEr and the repetition /
    diversity figures Para_RE_4, Para_XRE_4, Para_Div_1, Para_Div_2, with paragraph_top=k reading only the k best-scored
    proposals of a video as its paragraph; bootstrap=R adds the key "Bootstrap intervals": {metric: [dict(value, lo, hi, se)
    per tIoU]} of R resamples of the videos, evaluate.bootstrap)."""
    fields = ["results", "version", "external_data"]
    if evaluator is None:
        try:
            from evaluation.evaluate import ANETcaptions
        except Exception as e:  # noqa: BLE001
            raise NotImplementedError("the reference's caption evaluator (evaluation/evaluate.py: PTB tokenizer, METEOR jar) is "
                                      "not importable; put the reference on sys.path, or score on the device with "
                                      "evaluator='device' (cfg.caption_evaluator)") from e
        ev = ANETcaptions(reference_paths, submission_path, tIoUs, max_prop_per_vid, fields, verbose, only_proposals)
    elif evaluator == "device":
        from ..evaluate import DenseCaptionEvaluator
        ev = DenseCaptionEvaluator(reference_paths, submission_path, tIoUs, max_prop_per_vid, fields, verbose, only_proposals,
                                   **(evaluator_options or {}))
    else:
        raise ValueError(f"unknown caption evaluator {evaluator!r} (None: the reference's, 'device': this package's)")
    ev.evaluate()
    metrics = {tiou: {name: scores[i] for name, scores in ev.scores.items()} for i, tiou in enumerate(tIoUs)}
    metrics["Average across tIoUs"] = {name: sum(scores) / float(len(scores)) for name, scores in ev.scores.items()}
    if getattr(ev, "intervals", None):            # the device evaluator ran with bootstrap=R (evaluator_options)
        metrics["Bootstrap intervals"] = ev.intervals
    return metrics


def _write_and_score(cfg, predictions, phase, epoch, reference_paths, tIoUs, evaluator):
    """writes captioning_results_<phase>_e<epoch>.json under cfg.log_path and scores it: the metrics dictionary, or
    `predictions` itself (with its "submission_path") when the evaluator is not importable"""
    os.makedirs(cfg.log_path, exist_ok=True)
    path = os.path.join(cfg.log_path, f"captioning_results_{phase}_e{epoch}.json")
    if os.path.exists(path):          # another loader / pretrained model in the same run: keep both files
        path = path.replace(".json", f"_{time()}.json")
    with open(path, "w") as f:
        json.dump(predictions, f)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            return calculate_metrics(reference_paths, path, tIoUs, cfg.max_prop_per_vid, evaluator=evaluator,
                                     evaluator_options=getattr(cfg, "caption_evaluator_options", None))
    except NotImplementedError:
        predictions["submission_path"] = path
        return predictions


def validation_1by1_loop(cfg, model, loader, decoder, epoch, TBoard, evaluator=None):
    """Greedy-decode the whole loader, write captioning_results_<phase>_e<epoch>.json under cfg.log_path and score it.
    Returns the metrics dictionary; None when cfg.log_path is None (as the reference); the predictions dictionary when the
    evaluator is not importable (see calculate_metrics).  evaluator: None takes cfg.caption_evaluator when the config has
    one (the reference's driver passes six positional arguments), and None there too scores with the reference's
    evaluator; "device" scores with bmhrl_amd.evaluate (keywords: cfg.caption_evaluator_options, a dict)."""
    if evaluator is None:
        evaluator = getattr(cfg, "caption_evaluator", None)
    t_start = time()
    model.eval()
    loader.dataset.update_iterator()
    phase = loader.dataset.phase
    reference_paths, tIoUs = _phase_references(cfg, phase)
    predictions = predict_1by1(cfg, model, loader, decoder)
    if cfg.log_path is None:
        return None
    val_metrics = _write_and_score(cfg, predictions, phase, epoch, reference_paths, tIoUs, evaluator)
    if val_metrics is predictions:
        return predictions
    if TBoard is not None and phase != "learned_props":
        avg = val_metrics["Average across tIoUs"]
        for tag, key in (("meteor", "METEOR"), ("bleu4", "Bleu_4"), ("bleu3", "Bleu_3"), ("precision", "Precision"),
                         ("recall", "Recall")):
            TBoard.add_scalar(f"{phase}/{tag}", avg[key] * 100, epoch)
        if "Para_METEOR" in avg:      # the evaluator ran with paragraph=True (cfg.caption_evaluator_options)
            for tag, key in (("para_meteor", "Para_METEOR"), ("para_cider", "Para_CIDEr"), ("para_re4", "Para_RE_4")):
                TBoard.add_scalar(f"{phase}/{tag}", avg[key] * 100, epoch)
        TBoard.add_scalar(f"{phase}/duration_of_1by1", (time() - t_start) / 60, epoch)
    return val_metrics


def validation_next_word_loop(cfg, model, loader, decoder, criterion, epoch, TBoard, exp_name):
    """teacher-forced validation loss per batch, averaged over the loader (:139-158); `criterion` reduces to a scalar here
    (the captioning-module loops of the reference pass a summing criterion)"""
    model.eval()
    loader.dataset.update_iterator()
    pad_idx = loader.dataset.pad_idx
    total = 0.0
    for batch in loader:
        cap = batch["caption_data"].caption
        cap_in, cap_y = cap[:, :-1], cap[:, 1:]
        masks = make_masks(batch["feature_stacks"], cap_in, cfg.modality, pad_idx)
        with torch.no_grad():
            pred = model(batch["feature_stacks"], cap_in, masks)
            n_tokens = (cap_y != pad_idx).sum()
            total += (criterion(pred, cap_y) / n_tokens).item()
    return total / len(loader)


def _video_durations(reference_paths):
    """video id -> duration in seconds from the ground-truth files (ActivityNet-captions layout: {id: {"duration", ...}})"""
    durations = {}
    for path in reference_paths:
        with open(path) as f:
            for video_id, entry in json.load(f).items():
                durations.setdefault(video_id, float(entry["duration"]))
    return durations


def validation_learned_props_loop(cfg, model, proposals, decoder, epoch, TBoard, dataset, evaluator=None, paragraph=False):
    """Captions predicted proposals -- the reference's `learned_props` phase -- from the videos' full-length feature files:
    `proposals` is a submission dictionary or the path of a prop_results_*.json.  Its segments are grouped by video in the
    file's order; cfg.inference_batch_size videos at a time are loaded whole (predict.VideoFeatures: each file read once,
    onto cfg.device) and their segments cropped there and captioned in chunks of cfg.inference_batch_size by
    predict.caption_segments.  Durations come from the ground-truth files cfg.reference_paths.  Writes
    captioning_results_learned_props_e<epoch>.json and scores it against cfg.reference_paths at cfg.tIoUs; returns as
    validation_1by1_loop: the metrics, None when cfg.log_path is None, the predictions dictionary when the evaluator is not
    importable.  dataset: vocabulary and special tokens (train_vocab.itos, start_idx, end_idx, pad_idx).  paragraph=True:
    predict.caption_segments' time-ordered mode -- a video's proposals are captioned in time order, each with the video's
    earlier captions as the decoder's context."""
    from ..predict import VideoFeatures, caption_segments
    mode = {"paragraph": True} if paragraph else {}
    if evaluator is None:
        evaluator = getattr(cfg, "caption_evaluator", None)
    model.eval()
    if isinstance(proposals, (str, os.PathLike)):
        with open(proposals) as f:
            proposals = json.load(f)
    reference_paths, tIoUs = _phase_references(cfg, "learned_props")
    durations = _video_durations(reference_paths)
    videos = list(proposals["results"].items())
    predictions = {"version": "VERSION 1.0", "external_data": {"used": True, "details": ""}, "results": {}}
    step = int(cfg.inference_batch_size)
    for i in range(0, len(videos), step):
        group = videos[i:i + step]
        ids = [video_id for video_id, _ in group]
        features = VideoFeatures.from_npy(cfg, ids, [durations[v] for v in ids], cfg.pad_feats_up_to, dataset.pad_idx,
                                          torch.device(cfg.device))
        segments = [[tuple(seg["timestamp"]) for seg in segs] for _, segs in group]
        for video_id, caps in zip(ids, caption_segments(cfg, model, features, segments, decoder, dataset, **mode)):
            if caps:
                predictions["results"].setdefault(video_id, []).extend(caps)
    if cfg.log_path is None:
        return None
    return _write_and_score(cfg, predictions, "learned_props", epoch, reference_paths, tIoUs, evaluator)
