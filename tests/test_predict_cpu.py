"""Host side of captioning whole videos (bmhrl_amd/predict.py) without a GPU: the host restatement of the
segment crop against FeaturePacker.pack, the proposal tail AnetPredictions shares with VideoCaptioner against the recorded
results of the reference (tests/golden/proposals.json), and validation_learned_props_loop with a stub decoder and model."""
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from bmhrl_amd import loader as L
from bmhrl_amd import proposal_utils as pu
from tests import segment_crop_cases as C
from tests.proposal_reference import load_golden


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    vp, ap, arrays = C.write_features(tmp_path_factory.mktemp("features"))
    return SimpleNamespace(vp=vp, ap=ap, arrays=arrays, stacks=C.padded_stacks(arrays))


def host_crops(files, segs, widths=None):
    video, times = [s[0] for s in segs], [s[1:] for s in segs]
    out = {}
    for name, lens, pad in (("rgb", C.VIDEO_LEN, C.PAD_IDX), ("flow", C.VIDEO_LEN, 0), ("audio", C.AUDIO_LEN, C.PAD_IDX)):
        T = max([1] + [L.crop_rows(lens[v], s, e, C.DURATIONS[v])[1] for v, s, e in segs]) if widths is None else widths[name]
        out[name] = L.crop_segments_host(files.stacks[name], lens, C.DURATIONS, video, times, pad, T)
    return out


def test_crop_rows_is_crop_bounds():
    rng = np.random.default_rng(3)
    for _ in range(2000):
        S, dur = int(rng.integers(1, 900)), float(rng.uniform(0.1, 300.0))
        start, end = float(rng.uniform(-0.1, 1.1) * dur), float(rng.uniform(-0.1, 1.3) * dur)
        r = L.crop_bounds(S, start, end, dur)
        assert L.crop_rows(S, start, end, dur) == ((r[0], r[1] - r[0], True) if r else (0, 0, True))
    assert L.crop_rows(7, 1.0, 2.0, 0.0) == (0, 0, False) and L.crop_rows(7, 1.0, 2.0, -3.0) == (0, 0, False)
    assert L.crop_rows(7, float("nan"), 2.0, 5.0) == (0, 0, False) and L.crop_rows(7, 1.0, float("inf"), 5.0) == (0, 0, False)
    assert L.crop_rows(7, 1e308, 2e308, 1e-300) == (0, 0, False)


def test_host_crop_equals_pack_on_every_constructed_case(files):
    segs = C.segments()
    want = C.packed_clips(files.vp, files.ap, segs)
    got = host_crops(files, segs)
    empty = 0
    for name in ("rgb", "flow", "audio"):
        out, lengths, lo, status = got[name]
        assert out.dtype == torch.float32 and lengths.dtype == lo.dtype == status.dtype == torch.int32
        assert torch.equal(out, want[name]), name
        assert status.tolist() == [0, 0]
        lens = C.AUDIO_LEN if name == "audio" else C.VIDEO_LEN
        for p, (v, s, e) in enumerate(segs):
            r = L.crop_bounds(lens[v], s, e, C.DURATIONS[v])
            assert int(lengths[p]) == (r[1] - r[0] if r else 0) and (r is None or int(lo[p]) == r[0])
            empty += r is None
    assert empty >= 3                                               # the n = 0 layout is among the compared clips
    assert got["rgb"][1].tolist() == [7, 1, 1, 0, 2, 2, 0, 2, 2, 3, 1, 7]     # every branch, by its row count
    # a single segment, a wider output, a narrower one
    one = host_crops(files, segs[10:11])
    assert torch.equal(one["rgb"][0], C.packed_clips(files.vp, files.ap, segs[10:11])["rgb"])
    wide = host_crops(files, segs, widths={"rgb": 9, "flow": 9, "audio": 33})
    for name, pad in (("rgb", C.PAD_IDX), ("flow", 0), ("audio", C.PAD_IDX)):
        T = want[name].shape[1]
        assert torch.equal(wide[name][0][:, :T], want[name]) and bool((wide[name][0][:, T:] == pad).all())
    narrow = host_crops(files, segs, widths={"rgb": 2, "flow": 2, "audio": 2})
    out, lengths, _, status = narrow["rgb"]
    assert torch.equal(out, want["rgb"][:, :2]) and lengths.tolist() == got["rgb"][1].tolist() and status.tolist() == [3, 0]


def test_host_crop_counts_undefined_segments(files):
    out, lengths, lo, status = L.crop_segments_host(files.stacks["rgb"], C.VIDEO_LEN, [7.0, 0.0], [0, 1, 0, 2, -1],
                                                    [(1.0, 3.0), (1.0, 3.0), (float("nan"), 3.0), (1.0, 3.0), (1.0, 3.0)], 1, 3)
    assert lengths.tolist() == [2, 0, 0, 0, 0] and lo.tolist() == [1, 0, 0, 0, 0] and status.tolist() == [0, 4]
    assert torch.equal(out[0, :2], files.stacks["rgb"][0, 1:3]) and bool((out[0, 2:] == 1).all())
    for p in range(1, 5):
        assert bool((out[p, 0] == 0).all()) and bool((out[p, 1:] == 1).all())
    with pytest.raises(ValueError):
        L.crop_segments_host(files.stacks["rgb"], C.VIDEO_LEN, C.DURATIONS, [0], [(1.0, 3.0)], 1, 0)


def test_video_features_on_the_cpu_crop_what_pack_packs(files):
    from bmhrl_amd.predict import VideoFeatures
    cfg = SimpleNamespace(video_features_path=files.vp, audio_features_path=files.ap)
    feats = VideoFeatures.from_npy(cfg, C.VIDEO_IDS, C.DURATIONS, C.PAD_TO, C.PAD_IDX, "cpu")
    for name in ("rgb", "flow", "audio"):
        assert torch.equal(feats.feature_stacks()[name], files.stacks[name]), name
    assert feats.lens_host["rgb"] == C.VIDEO_LEN and feats.lens_host["audio"] == C.AUDIO_LEN
    segs = C.segments()
    want = C.packed_clips(files.vp, files.ap, segs)
    fs, status = feats.crop([s[0] for s in segs], [s[1:] for s in segs], "audio_video", return_status=True)
    assert set(fs) == {"rgb", "flow", "audio"} and all(torch.equal(fs[k], want[k]) for k in fs)
    assert tuple(status.shape) == (3, 2) and int(status.sum()) == 0
    assert set(feats.crop([0], [(1.0, 2.0)], "audio")) == {"audio"} and set(feats.crop([0], [(1.0, 2.0)], "video")) == {"rgb", "flow"}
    # by explicit paths; a missing flow file drops rgb too: length 0, every clip the one-zero-row layout
    paths = [{"rgb": f"{files.vp}/v_a_rgb.npy", "flow": f"{files.vp}/nothing.npy", "audio": f"{files.ap}/v_a.npy"}]
    lone = VideoFeatures.from_npy(paths, ["x"], [7.0], C.PAD_TO, C.PAD_IDX, "cpu")
    assert lone.lens_host["rgb"] == [0] and lone.lens_host["audio"] == [19]
    clip = lone.crop([0], [(1.0, 3.0)])
    assert tuple(clip["rgb"].shape) == (1, 1, L.D_VIDEO) and not clip["rgb"].any() and not clip["flow"].any()
    assert torch.equal(clip["audio"], want["audio"][:1, :0].new_tensor(files.arrays["audio"][0][2:8]).unsqueeze(0))
    with pytest.raises(ValueError):
        VideoFeatures.from_npy(cfg, C.VIDEO_IDS, C.DURATIONS, {"video": 12, "audio": 40}, C.PAD_IDX, "cpu")


def test_shared_proposal_tail_reproduces_every_recorded_case():
    golden = load_golden()
    batch = {"duration_in_secs": golden["durations"], "video_ids": golden["video_ids"]}
    assert len(golden["cases"]) == 30
    for case in golden["cases"]:
        cfg = SimpleNamespace(max_prop_per_vid=case["k"], nms_tiou_thresh=case["nms_tiou"])
        pred = torch.from_numpy(golden["inputs"][case["N"]])
        rows, k = pu.select_rows(pred.clone(), cfg, batch)
        assert k == case["k_eff"] and len(rows) == len(golden["video_ids"])
        segments = [pu.rows_to_segments(r) for r in rows]
        results = {vid: segs for vid, segs in zip(golden["video_ids"], segments) if segs}
        assert json.loads(json.dumps(results)) == case["results"]
        assert sum(len(s) for s in segments) == case["segments_used"]
        # and AnetPredictions, which now calls the same two functions, still gives the recorded dictionary
        anet = pu.AnetPredictions(cfg, "val_1", 0)
        assert anet.add_new_predictions(pred.clone(), batch) == case["returned"]
        assert json.loads(json.dumps(anet.predictions["results"])) == case["results"]
    assert pu.rows_to_segments([[1.0, 1.2, 0.5], [1.0, 1.2000049, 0.5], [0.123456789, 5.0, 0.987654321]]) == \
        [{"sentence": "", "proposal_score": (0.98765,), "timestamp": [0.12346, 5.0]}]


ITOS = ["<unk>", "<blank>", "<s>", "</s>", "a", "man", "runs", "fast"]


def loop_setup(files, tmp_path, **over):
    ds = SimpleNamespace(start_idx=2, end_idx=3, pad_idx=C.PAD_IDX, train_vocab=SimpleNamespace(itos=ITOS))
    refs = []
    for i in range(4):
        refs.append(str(tmp_path / f"ref{i}.json"))
        with open(refs[-1], "w") as f:
            json.dump({vid: {"duration": d, "timestamps": [[0.0, d]], "sentences": ["a man runs"]}
                       for vid, d in zip(C.VIDEO_IDS, C.DURATIONS)}, f)
    cfg = SimpleNamespace(max_len=4, modality="audio_video", log_path=str(tmp_path / "log"), reference_paths=refs,
                          max_prop_per_vid=100, tIoUs=[0.3, 0.5, 0.7, 0.9], inference_batch_size=1, device="cpu",
                          video_features_path=files.vp, audio_features_path=files.ap, pad_feats_up_to=C.PAD_TO)
    for k, v in over.items():
        setattr(cfg, k, v)
    calls = []

    def decoder(model, fs, max_len, start, end, pad, modality):
        calls.append((model, {k: v.clone() for k, v in fs.items()}, max_len, start, end, pad, modality))
        return torch.tensor([[2, 4, 5, 3, 1], [2, 6, 7, 7, 7]])[:fs["rgb"].shape[0]]

    class Model:
        module = "the-agent"

        def eval(self):
            calls.append("eval")
    segs = C.segments()
    proposals = {"version": "VERSION 1.0", "external_data": {"used": True, "details": ""}, "results": {}}
    for v, s, e in [segs[7], segs[11], segs[10], segs[4], segs[0]]:          # videos interleaved: a, b, a, b, a
        proposals["results"].setdefault(C.VIDEO_IDS[v], []).append({"sentence": "", "proposal_score": [0.5], "timestamp": [s, e]})
    return cfg, ds, decoder, Model(), proposals, calls


def test_learned_props_loop_groups_by_video_and_keeps_the_order(files, tmp_path):
    from bmhrl_amd.epoch_loops.validation_loops import validation_learned_props_loop
    cfg, ds, decoder, model, proposals, calls = loop_setup(files, tmp_path, inference_batch_size=2)
    out = validation_learned_props_loop(cfg, model, proposals, decoder, 5, None, ds)
    path = tmp_path / "log" / "captioning_results_learned_props_e5.json"
    assert out["submission_path"] == str(path)                   # no evaluator importable here: the predictions come back
    saved = json.load(open(path))
    assert saved["version"] == "VERSION 1.0" and saved["external_data"] == {"used": True, "details": ""}
    segs = C.segments()
    # both videos load together; their five segments in the file's order (a, a, a, b, b) in chunks of two
    assert saved["results"] == {
        "v_a": [{"sentence": "A man", "timestamp": [3.0, 5.0]}, {"sentence": "Runs fast fast fast", "timestamp": [2.0, 2.05]},
                {"sentence": "A man", "timestamp": [0.0, 7.0]}],
        "v_b": [{"sentence": "Runs fast fast fast", "timestamp": [4.0, 18.0]}, {"sentence": "A man", "timestamp": [22.0, 45.0]}]}
    assert list(saved["results"]) == ["v_a", "v_b"]
    assert calls[0] == "eval" and [c[0] for c in calls[1:]] == ["the-agent"] * 3
    assert [c[2:] for c in calls[1:]] == [(4, 2, 3, C.PAD_IDX, "audio_video")] * 3
    order = [segs[7], segs[10], segs[0], segs[11], segs[4]]
    for c, chunk in zip(calls[1:], (order[0:2], order[2:4], order[4:5])):
        want = C.packed_clips(files.vp, files.ap, chunk)
        assert all(torch.equal(c[1][k], want[k]) for k in ("rgb", "flow", "audio"))
    # the same proposals from a file, one video at a time; a second file of the same epoch keeps both
    cfg.inference_batch_size = 1
    prop_path = tmp_path / "prop_results_val_1_e0_maxprop100.json"
    with open(prop_path, "w") as f:
        json.dump(proposals, f)
    del calls[:]
    out2 = validation_learned_props_loop(cfg, model, str(prop_path), decoder, 5, None, ds)
    assert out2["results"]["v_a"] == [{"sentence": "A man", "timestamp": s["timestamp"]} for s in saved["results"]["v_a"]]
    assert out2["submission_path"] != str(path) and out2["submission_path"].startswith(str(path)[:-5] + "_")
    assert len(calls) == 1 + 5
    cfg.log_path = None
    assert validation_learned_props_loop(cfg, model, proposals, decoder, 5, None, ds) is None


def test_learned_props_loop_ends_as_the_1by1_loop_with_the_device_evaluator(files, tmp_path):
    """evaluator="device": without a GPU both loops fail, in the same way; with one both return the metrics"""
    from bmhrl_amd.epoch_loops.validation_loops import validation_1by1_loop, validation_learned_props_loop
    cfg, ds, decoder, model, proposals, _ = loop_setup(files, tmp_path, caption_evaluator_options=dict(stemmer=False, synonyms=False))
    ds.phase, ds.update_iterator = "learned_props", lambda: None

    class Loader(list):
        dataset = ds
    batch = dict(feature_stacks={"rgb": torch.zeros(2, 1, 1)}, video_ids=C.VIDEO_IDS, starts=torch.tensor([[0.0], [1.5]]),
                 ends=torch.tensor([[2.0], [3.5]]))

    def outcome(fn):
        try:
            out = fn()
        except Exception as e:  # noqa: BLE001
            return "raised", type(e), str(e)
        return "returned", type(out), sorted(map(str, out))

    by1 = outcome(lambda: validation_1by1_loop(cfg, model, Loader([batch]), decoder, 0, None, evaluator="device"))
    learned = outcome(lambda: validation_learned_props_loop(cfg, model, proposals, decoder, 0, None, ds, evaluator="device"))
    print(by1)
    assert learned == by1
    assert by1[0] == ("returned" if torch.cuda.is_available() else "raised")
    if by1[0] == "returned":
        assert "Average across tIoUs" in by1[2] and "submission_path" not in by1[2]
    assert (tmp_path / "log" / "captioning_results_learned_props_e0.json").exists()      # written before it is scored
