"""bmhrl_amd/predict.py on the MI355X: caption_segments against the file route -- the same clips through
FeaturePacker.pack and an upload into the same decoder, chunk for chunk -- and the structure of VideoCaptioner.predict.

The configuration is the tiny one of tests/test_proposal_generator_gpu.py (tiny_cfg(d_model=1024), B = 2, 11 video and 19 audio
rows) with the feature widths of the files FeaturePacker lays out (1024 / 128); agent and generator are randomly initialised.
The clips of both routes are bit-equal (asserted), so their token ids must be equal."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from bmhrl_amd import loader as L
from bmhrl_amd import synthetic as syn

pytestmark = pytest.mark.gpu

B, TV, TA, VOCAB, PAD = 2, 11, 19, 40, 1
VIDEO_IDS, DURATIONS = ["v_0", "v_1"], [22.0, 20.5]
PAD_TO = {"video": 16, "audio": 24}
ANCHORS = {"video": [2.0, 4.0, 8.0, 14.0], "audio": [3.0, 6.0, 12.0]}
ITOS = ["<unk>", "<blank>", "<s>", "</s>"] + [f"w{i}" for i in range(VOCAB - 4)]
# three per video; (3.0, 3.4) is shorter than a video row (2 s) and an audio row (1.16 s)
SEGMENTS = [[(0.0, 22.0), (3.0, 3.4), (5.5, 16.25)], [(12.0, 20.5), (0.12346, 7.0), (20.5, 20.5)]]


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bmhrl_amd import _lib
    from bmhrl_amd.model.bm_hrl_agent import BMHrlAgent
    from bmhrl_amd.model.proposal_generator import MultimodalProposalGenerator
    from bmhrl_amd.predict import VideoFeatures
    _lib.load()
    dev = torch.device("cuda:0")
    folder = tmp_path_factory.mktemp("features")
    rng = np.random.default_rng(0)
    for vid in VIDEO_IDS:
        for name, shape in ((f"{vid}_rgb", (TV, L.D_VIDEO)), (f"{vid}_flow", (TV, L.D_VIDEO)), (vid, (TA, L.D_AUDIO))):
            np.save(os.path.join(str(folder), name + ".npy"), rng.standard_normal(shape).astype(np.float32))
    cfg = syn.tiny_cfg(d_model=1024, rl_att_heads=4, dout_p=0.0, d_vid=L.D_VIDEO, d_aud=L.D_AUDIO, d_model_video=L.D_VIDEO,
                       d_model_audio=L.D_AUDIO)
    cfg.device, cfg.max_len, cfg.inference_batch_size = "cuda:0", 6, 4
    cfg.video_features_path = cfg.audio_features_path = str(folder)
    cfg.pad_feats_up_to = PAD_TO
    cfg.kernel_sizes, cfg.strides = {"video": [1, 5], "audio": [3]}, {"video": 2.0, "audio": 1.2}
    cfg.conv_hidden, cfg.obj_coeff, cfg.noobj_coeff = 32, 1.0, 100.0
    cfg.max_prop_per_vid, cfg.nms_tiou_thresh = 5, 0.4
    ds = SimpleNamespace(trg_voc_size=VOCAB, train_vocab=SimpleNamespace(vectors=None, itos=ITOS), start_idx=2, end_idx=3, pad_idx=PAD)
    torch.manual_seed(3)
    agent = BMHrlAgent(cfg, ds).to(dev).eval()
    agent.set_inference_mode(True)
    generator = MultimodalProposalGenerator(cfg, ANCHORS).to(dev).eval()
    features = VideoFeatures.from_npy(cfg, VIDEO_IDS, DURATIONS, PAD_TO, PAD, dev)
    return SimpleNamespace(cfg=cfg, ds=ds, agent=agent, generator=generator, features=features, dev=dev, folder=str(folder))


def recording(decoder, log):
    def run(model, fs, *rest):
        ids = decoder(model, fs, *rest)
        log.append(({k: v.clone() for k, v in fs.items()}, ids.clone()))
        return ids
    return run


def decoders():
    from bmhrl_amd.decode import beam_decoder, greedy_decoder
    return {"greedy": greedy_decoder(), "beam2": beam_decoder(2)}


@pytest.mark.parametrize("which", ["greedy", "beam2"])
def test_caption_segments_equal_the_file_route(setup, which):
    from bmhrl_amd.epoch_loops.validation_loops import tokens_to_sentences
    from bmhrl_amd.predict import caption_segments
    s, decoder = setup, decoders()[which]
    log = []
    got = caption_segments(s.cfg, s.agent, s.features, SEGMENTS, recording(decoder, log), s.ds, batch_size=4)
    assert [len(g) for g in got] == [3, 3] and len(log) == 2 and [ids.shape[0] for _, ids in log] == [4, 2]

    packer = L.FeaturePacker(s.folder, s.folder, PAD, pin=False)
    flat = [(v, a, b) for v, segs in enumerate(SEGMENTS) for a, b in segs]
    sentences = []
    for (fs, ids), i in zip(log, (0, 4)):
        clips = [L.Clip(VIDEO_IDS[v], "", a, b, DURATIONS[v]) for v, a, b in flat[i:i + 4]]
        host = packer.pack(clips)
        packed = {k: t.to(s.dev) for k, t in host.items()}
        for k in ("rgb", "flow", "audio"):
            assert torch.equal(fs[k], packed[k]), (which, i, k)              # the crops ARE the packed clips
        with torch.no_grad():
            want = decoder(s.agent, packed, s.cfg.max_len, 2, 3, PAD, s.cfg.modality)
        assert torch.equal(ids, want), (which, i)
        sentences += tokens_to_sentences(want.cpu().numpy(), ITOS)
    assert log[0][0]["rgb"].shape[1] == TV and log[0][0]["audio"].shape[1] == TA        # the whole video is in the first chunk
    assert log[1][0]["rgb"].shape[1] == 3 and int(log[0][1][0, 0]) == 2
    want = [[], []]
    for (v, a, b), sent in zip(flat, sentences):
        want[v].append({"sentence": sent, "timestamp": [a, b]})
    assert got == want


def test_caption_segments_checks_the_status_once(setup):
    from bmhrl_amd.predict import caption_segments
    s = setup
    stub = lambda model, fs, *rest: torch.tensor([[2, 4, 3]] * fs["rgb"].shape[0])       # noqa: E731
    assert caption_segments(s.cfg, s.agent, s.features, [[], [(1.0, 2.0)]], stub, s.ds) == \
        [[], [{"sentence": "W0", "timestamp": [1.0, 2.0]}]]
    assert caption_segments(s.cfg, s.agent, s.features, [[], []], stub, s.ds) == [[], []]
    with pytest.raises(RuntimeError, match="1 had no defined row range"):
        caption_segments(s.cfg, s.agent, s.features, [[(1.0, 2.0)], [(float("nan"), 2.0)]], stub, s.ds, batch_size=1)
    with pytest.raises(ValueError):
        caption_segments(s.cfg, s.agent, s.features, [[(1.0, 2.0)]], stub, s.ds)


def test_video_captioner_predict(setup):
    from bmhrl_amd.model.masking import make_masks
    from bmhrl_amd.predict import VideoCaptioner
    from bmhrl_amd.proposal_utils import AnetPredictions
    s = setup
    captioner = VideoCaptioner(s.cfg, s.generator, s.agent, s.ds)
    fs = s.features.feature_stacks()
    assert tuple(fs["rgb"].shape) == (B, 16, L.D_VIDEO) and tuple(fs["audio"].shape) == (B, 24, L.D_AUDIO)
    with torch.no_grad():
        model_output = s.generator(fs, None, make_masks(fs, None, s.cfg.modality, PAD))[0]
    anet = AnetPredictions(s.cfg, "val_1", 0)
    anet.add_new_predictions(model_output, {"duration_in_secs": DURATIONS, "video_ids": VIDEO_IDS})
    proposals = captioner.proposals(s.features)
    assert {v: p for v, p in zip(VIDEO_IDS, proposals) if p} == anet.predictions["results"]

    out = captioner.predict(s.features)
    assert set(out) == {"version", "external_data", "results"} and out["version"] == "VERSION 1.0"
    assert out["external_data"] == {"used": True, "details": ""}
    assert set(out["results"]) == set(anet.predictions["results"])
    for vid, segs in out["results"].items():
        duration = DURATIONS[VIDEO_IDS.index(vid)]
        assert 1 <= len(segs) <= s.cfg.max_prop_per_vid
        for seg, prop in zip(segs, anet.predictions["results"][vid]):
            assert set(seg) == {"sentence", "timestamp", "proposal_score"} and isinstance(seg["sentence"], str)
            a, b = seg["timestamp"]
            assert a == round(a, 5) and b == round(b, 5) and 0.0 <= a < b <= duration and b - a > 0.2
            assert seg["timestamp"] == prop["timestamp"] and seg["proposal_score"] == prop["proposal_score"]
    # the single-video convenience: the first video alone, from its three files
    paths = {"rgb": os.path.join(s.folder, "v_0_rgb.npy"), "flow": os.path.join(s.folder, "v_0_flow.npy"),
             "audio": os.path.join(s.folder, "v_0.npy")}
    single = captioner.predict_video(paths, DURATIONS[0])
    assert all(set(r) == {"start", "end", "sentence"} for r in single) and len(single) <= s.cfg.max_prop_per_vid
    assert all(0.0 <= r["start"] < r["end"] <= DURATIONS[0] for r in single)
