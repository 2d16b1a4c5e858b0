"""Shared fixture of the segment-crop tests (tests/test_segment_crop_gpu.py, tests/test_predict_cpu.py): two videos written as
feature files, a dozen segments that take every branch of loader.crop_bounds, and the clips FeaturePacker.pack makes of them."""
import os

import numpy as np
import torch

from bmhrl_amd import loader as L

PAD_IDX = 1
VIDEO_IDS = ["v_a", "v_b"]
VIDEO_LEN, AUDIO_LEN = [7, 13], [19, 31]
PAD_TO = {"video": 16, "audio": 40}
DURATIONS = [7.0, 26.0]            # S and 2 S seconds of video rows: start / duration is j / S for whole seconds


def segments():
    """(video, start, end); the comment names the branch for the video stacks (S = 7 and 13)"""
    up, down = np.nextafter(3.0, np.inf), np.nextafter(3.0, -np.inf)
    return [
        (0, 0.0, 7.0),             # the whole video
        (0, 3.0, 3.0),             # start == end: one row
        (0, 7.0, 7.0),             # start == end == duration: a == S, the last row
        (1, 20.0, 10.0),           # start > end: empty (n = 0)
        (1, 22.0, 45.0),           # end > duration: clamped to S
        (1, -4.0, 26.0),           # start < 0: the slice wraps to S - 2
        (1, -4.0, 10.0),           # wrapped start behind the end: empty
        (0, 3.0, 5.0),             # quotients exactly 3 / 7 and 5 / 7
        (0, float(up), 5.0),       # one ulp above 3 / 7 ...
        (0, float(down), 5.0),     # ... and one below
        (0, 2.0, 2.05),            # shorter than a feature row
        (1, 4.0, 18.0),            # the longest crop of video 1 but the whole
    ]


def write_features(folder, d_video=L.D_VIDEO, d_audio=L.D_AUDIO, seed=0):
    """the .npy files of both videos under folder/video and folder/audio; returns {name: [array per video]}"""
    rng = np.random.default_rng(seed)
    vp, ap = os.path.join(str(folder), "video"), os.path.join(str(folder), "audio")
    os.makedirs(vp, exist_ok=True)
    os.makedirs(ap, exist_ok=True)
    arrays = {"rgb": [], "flow": [], "audio": []}
    for vid, sv, sa in zip(VIDEO_IDS, VIDEO_LEN, AUDIO_LEN):
        for name, shape, path in (("rgb", (sv, d_video), os.path.join(vp, f"{vid}_rgb.npy")),
                                  ("flow", (sv, d_video), os.path.join(vp, f"{vid}_flow.npy")),
                                  ("audio", (sa, d_audio), os.path.join(ap, f"{vid}.npy"))):
            a = rng.standard_normal(shape).astype(np.float32)
            np.save(path, a)
            arrays[name].append(a)
    return vp, ap, arrays


def padded_stacks(arrays):
    """the full-length stacks as load_features_from_npy(get_full_feat=True) pads them: {name: (2, S_pad, D) fp32}"""
    out = {}
    for name, pad, key in (("rgb", PAD_IDX, "video"), ("flow", 0, "video"), ("audio", PAD_IDX, "audio")):
        out[name] = torch.stack([L.pad_segment(torch.from_numpy(a), PAD_TO[key], pad) for a in arrays[name]])
    return out


def packed_clips(vp, ap, segs):
    """FeaturePacker.pack of the segments as clips: {name: (P, T, D)} (copies: pack reuses its staging)"""
    packer = L.FeaturePacker(vp, ap, PAD_IDX, pin=False, threads=1)
    clips = [L.Clip(VIDEO_IDS[v], "", s, e, DURATIONS[v]) for v, s, e in segs]
    return {k: t.clone() for k, t in packer.pack(clips).items()}
