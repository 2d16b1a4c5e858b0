"""ops.crop_segments (csrc/segment_crop.hip) on the MI355X: the row ranges against loader.crop_bounds,
exactly; the clips bit for bit against FeaturePacker.pack of the same segments read from feature files; truncation and the end
of the buffer; undefined segments; refused arguments; graph capture.  A pure copy with integer bounds: every comparison is
an equality."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from bmhrl_amd import loader as L
from tests import segment_crop_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bmhrl_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    vp, ap, arrays = C.write_features(tmp_path_factory.mktemp("features"))
    segs = C.segments()
    return SimpleNamespace(vp=vp, ap=ap, arrays=arrays, stacks=C.padded_stacks(arrays), segs=segs,
                           packed=C.packed_clips(vp, ap, segs))


STACKS = (("rgb", C.VIDEO_LEN, C.PAD_IDX), ("flow", C.VIDEO_LEN, 0), ("audio", C.AUDIO_LEN, C.PAD_IDX))


def device_args(dev, lens, durations, segs):
    return (torch.tensor(lens, dtype=torch.int32, device=dev), torch.tensor(durations, dtype=torch.float64, device=dev),
            torch.tensor([s[0] for s in segs], dtype=torch.int32, device=dev),
            torch.tensor([s[1:] for s in segs], dtype=torch.float64, device=dev))


def bound_cases():
    """(S, start, end, duration): 4096 random ones and the constructed ones"""
    rng = np.random.default_rng(11)
    cases = []
    for _ in range(4096):
        S, dur = int(rng.integers(1, 901)), float(rng.uniform(0.5, 400.0))
        start = float(rng.uniform(0.0, 1.0) * dur)
        cases.append((S, start, start + float(rng.uniform(0.0, 0.6) * dur), dur))
    for S in (1, 2, 7, 13, 300, 899, 900):
        for dur in (0.1, 1.0, 7.0, 26.0, 123.456, 1e4):
            cases += [(S, 0.3 * dur, 0.3 * dur, dur),               # start == end
                      (S, dur, dur, dur),                           # start == end == duration: a == S
                      (S, 0.0, 0.0, dur), (S, 0.0, dur, dur),
                      (S, 0.7 * dur, 0.2 * dur, dur),               # start > end
                      (S, 0.5 * dur, 1.7 * dur, dur),               # end > duration
                      (S, 1.2 * dur, 1.5 * dur, dur),               # both past the end
                      (S, -0.15 * dur, 0.9 * dur, dur),             # start < 0: the slice wraps
                      (S, -0.15 * dur, dur, dur), (S, -3.0 * dur, 0.5 * dur, dur), (S, -0.5 * dur, -0.1 * dur, dur)]
            for j in sorted({0, 1, S // 3, S // 2, S - 1, S}):
                x = dur * j / S                                     # start / duration at, or within an ulp of, j / S
                for start in (x, float(np.nextafter(x, np.inf)), float(np.nextafter(x, -np.inf))):
                    cases += [(S, start, dur, dur), (S, 0.0, start, dur), (S, start, start, dur)]
    for S in (7, 13, 64, 900):                                      # quotients that ARE j / S: whole seconds of an S-second video
        for j in range(0, S + 1, max(1, S // 16)):
            cases += [(S, float(j), float(S), float(S)), (S, 0.0, float(j), float(S)), (S, float(j), float(j), float(S)),
                      (S, float(2 * j), float(2 * S), float(2 * S))]
    return cases


def test_bounds_equal_crop_bounds_exactly(dev):
    from bmhrl_amd import ops
    cases = bound_cases()
    P, S_pad, D = len(cases), 900, 4
    want = [L.crop_bounds(*c) for c in cases]
    assert sum(w is None for w in want) > 50 and sum(w is not None and w[0] + 1 == w[1] for w in want) > 100
    src = torch.arange(S_pad * D, dtype=torch.float32, device=dev).view(1, S_pad, D).expand(P, S_pad, D).contiguous()
    src_len = torch.tensor([c[0] for c in cases], dtype=torch.int32, device=dev)
    durations = torch.tensor([c[3] for c in cases], dtype=torch.float64, device=dev)
    video = torch.arange(P, dtype=torch.int32, device=dev)
    times = torch.tensor([c[1:3] for c in cases], dtype=torch.float64, device=dev)
    out, lengths, lo, status = ops.crop_segments(src, src_len, durations, video, times, -1.0, S_pad)
    lengths, lo = lengths.tolist(), lo.tolist()
    bad = [(c, w, (lo[p], lengths[p])) for p, (c, w) in enumerate(zip(cases, want))
           if lengths[p] != (w[1] - w[0] if w else 0) or (w is not None and lo[p] != w[0])]
    assert not bad, (len(bad), bad[:5])
    assert status.tolist() == [0, 0]
    # the rows themselves: row r of src holds 4 r .. 4 r + 3, so column 0 of a clip is 4 (lo + r), then the padding
    first = out[:, :, 0].cpu()
    rows = torch.arange(S_pad).view(1, -1)
    n, a = torch.tensor(lengths).view(-1, 1), torch.tensor(lo).view(-1, 1)
    expect = torch.where(rows < n, 4.0 * (a + rows), torch.tensor(-1.0))
    expect[:, 0] = torch.where(n[:, 0] == 0, torch.tensor(0.0), expect[:, 0])
    assert torch.equal(first, expect.float())


@pytest.mark.parametrize("extra", [0, 5])
def test_contents_equal_pack_bit_for_bit(dev, files, extra):
    """T_out = pack's own width (extra = 0) and a larger one; D = 1024 (rgb, flow) and 128 (audio), 16-byte accesses"""
    from bmhrl_amd import ops
    empty = 0
    for name, lens, pad in STACKS:
        want = files.packed[name]
        T = want.shape[1]
        args = device_args(dev, lens, C.DURATIONS, files.segs)
        src = files.stacks[name].to(dev)
        assert src.data_ptr() % 16 == 0
        out, lengths, lo, status = ops.crop_segments(src, *args, pad, T + extra)
        assert torch.equal(out[:, :T].cpu(), want), name
        assert bool((out[:, T:] == pad).all()) and status.tolist() == [0, 0]
        assert max(lengths.tolist()) == T                          # pack's width is the longest crop
        empty += lengths.tolist().count(0)
        _, hl, hlo, _ = L.crop_segments_host(files.stacks[name], lens, C.DURATIONS, [s[0] for s in files.segs],
                                             [s[1:] for s in files.segs], pad, T + extra)
        assert torch.equal(lengths.cpu(), hl) and torch.equal(lo.cpu(), hlo)
    assert empty >= 3                                               # the one-zero-row layout is among them


def test_unaligned_base_takes_the_scalar_path(dev, files):
    from bmhrl_amd import ops
    for name, lens, pad in (STACKS[0], STACKS[2]):
        want = files.packed[name]
        stack = files.stacks[name]
        buf = torch.empty(stack.numel() + 1, device=dev)
        src = buf[1:].view(stack.shape)
        src.copy_(stack)
        assert src.data_ptr() % 16 == 4 and src.is_contiguous()
        out, _, _, status = ops.crop_segments(src, *device_args(dev, lens, C.DURATIONS, files.segs), pad, want.shape[1])
        assert torch.equal(out.cpu(), want) and status.tolist() == [0, 0]
        # and an output whose base is 4-byte aligned
        obuf = torch.empty(want.numel() + 1, device=dev)
        o = obuf[1:].view(want.shape)
        ops.crop_segments(stack.to(dev), *device_args(dev, lens, C.DURATIONS, files.segs), pad, want.shape[1], out=o)
        assert torch.equal(o.cpu(), want)


@pytest.mark.parametrize("D", [3, 1, 6])
def test_any_feature_width_against_the_host_restatement(dev, D):
    from bmhrl_amd import ops
    rng = np.random.default_rng(D)
    stack = torch.stack([L.pad_segment(torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32)), 16, C.PAD_IDX)
                         for n in C.VIDEO_LEN])
    segs = C.segments()
    video, times = [s[0] for s in segs], [s[1:] for s in segs]
    for T in (7, 9, 1500):                                          # 1500 rows of 3 floats: more than one tile per segment
        want = L.crop_segments_host(stack, C.VIDEO_LEN, C.DURATIONS, video, times, C.PAD_IDX, T)
        got = ops.crop_segments(stack.to(dev), *device_args(dev, C.VIDEO_LEN, C.DURATIONS, segs), C.PAD_IDX, T)
        assert all(torch.equal(g.cpu(), w) for g, w in zip(got, want)), (D, T)


def test_many_tiles_and_more_work_than_the_grid(dev):
    """D = 1024: four rows per tile; 2100 segments of up to 21 rows: more (segment, tile) pairs than the grid has blocks"""
    from bmhrl_amd import ops
    rng = np.random.default_rng(5)
    V, S_pad, D, P = 3, 24, 1024, 2100
    lens = [21, 24, 5]
    stack = torch.from_numpy(rng.standard_normal((V, S_pad, D)).astype(np.float32))
    durations = [10.0, 33.3, 2.5]
    segs = []
    for _ in range(P):
        v = int(rng.integers(0, V))
        s = float(rng.uniform(0, durations[v]))
        segs.append((v, s, s + float(rng.uniform(0, durations[v]))))
    want = L.crop_segments_host(stack, lens, durations, [s[0] for s in segs], [s[1:] for s in segs], 7.0, 21)
    got = ops.crop_segments(stack.to(dev), *device_args(dev, lens, durations, segs), 7.0, 21)
    assert all(torch.equal(g.cpu(), w) for g, w in zip(got, want))
    assert int(want[3][0]) > 0                                      # some crops of the 24-row video are cut at 21 rows


def test_truncation_stays_inside_the_buffer(dev, files):
    from bmhrl_amd import ops
    for name, lens, pad in (STACKS[0], STACKS[2]):
        want = files.packed[name]
        P, T_full, D = want.shape
        T = 2
        big = torch.full((P + 2, T, D), 12345.0, device=dev)
        out = big[1:P + 1]
        _, lengths, _, status = ops.crop_segments(files.stacks[name].to(dev), *device_args(dev, lens, C.DURATIONS, files.segs),
                                                  pad, T, out=out)
        assert bool((big[0] == 12345.0).all()) and bool((big[-1] == 12345.0).all())
        assert torch.equal(out.cpu(), want[:, :T])
        n = [L.crop_rows(lens[v], s, e, C.DURATIONS[v])[1] for v, s, e in files.segs]
        assert lengths.tolist() == n and max(n) == T_full > T      # not clipped
        assert status.tolist() == [sum(x > T for x in n), 0]


def test_undefined_segments_are_empty_and_counted(dev, files):
    from bmhrl_amd import ops
    src = files.stacks["rgb"].to(dev)
    src_len = torch.tensor(C.VIDEO_LEN, dtype=torch.int32, device=dev)
    durations = torch.tensor([7.0, 0.0], dtype=torch.float64, device=dev)
    video = torch.tensor([0, 1, 0, 2], dtype=torch.int32, device=dev)
    times = torch.tensor([(1.0, 3.0), (1.0, 3.0), (math.nan, 3.0), (1.0, 3.0)], dtype=torch.float64, device=dev)
    out, lengths, lo, status = ops.crop_segments(src, src_len, durations, video, times, C.PAD_IDX, 3)
    torch.cuda.synchronize()
    assert lengths.tolist() == [2, 0, 0, 0] and lo.tolist() == [1, 0, 0, 0] and status.tolist() == [0, 3]
    assert torch.equal(out[0, :2], src[0, 1:3]) and bool((out[0, 2] == C.PAD_IDX).all())
    for p in (1, 2, 3):
        assert bool((out[p, 0] == 0).all()) and bool((out[p, 1:] == C.PAD_IDX).all())
    want = L.crop_segments_host(files.stacks["rgb"], C.VIDEO_LEN, [7.0, 0.0], video.tolist(), times.tolist(), C.PAD_IDX, 3)
    assert all(torch.equal(g.cpu(), w) for g, w in zip((out, lengths, lo, status), want))
    # more: a negative duration, infinite times, a video index below zero, a row count beyond the stack
    durations = torch.tensor([-7.0, 26.0], dtype=torch.float64, device=dev)
    video = torch.tensor([0, 1, 1, -1, 1], dtype=torch.int32, device=dev)
    times = torch.tensor([(1.0, 3.0), (math.inf, 3.0), (1.0, -math.inf), (1.0, 3.0), (2.0, 6.0)], dtype=torch.float64, device=dev)
    _, lengths, _, status = ops.crop_segments(src, src_len, durations, video, times, C.PAD_IDX, 3)
    assert lengths.tolist() == [0, 0, 0, 0, 2] and status.tolist() == [0, 4]
    _, lengths, _, status = ops.crop_segments(src, torch.tensor([17, -1], dtype=torch.int32, device=dev), durations.abs(),
                                              video.abs(), times[[0, 4, 4, 0, 4]].contiguous(), C.PAD_IDX, 3)
    assert lengths.tolist() == [0] * 5 and status.tolist() == [0, 5]


def test_refused_arguments(dev, files):
    from bmhrl_amd import _lib, ops
    lib = _lib.load()
    src = files.stacks["rgb"].to(dev)
    V, S_pad, D = src.shape
    src_len, durations, video, times = device_args(dev, C.VIDEO_LEN, C.DURATIONS, files.segs)
    P, T = video.numel(), 7
    out = torch.full((P, T, D), 5.0, device=dev)
    lengths, lo = torch.zeros(P, dtype=torch.int32, device=dev), torch.zeros(P, dtype=torch.int32, device=dev)
    status = torch.full((2,), 9, dtype=torch.int32, device=dev)
    good = dict(src=src.data_ptr(), src_len=src_len.data_ptr(), durations=durations.data_ptr(), V=V, S_pad=S_pad, D=D,
                seg_video=video.data_ptr(), seg_times=times.data_ptr(), P=P, pad=1.0, T_out=T, out=out.data_ptr(),
                lengths=lengths.data_ptr(), lo=lo.data_ptr(), status=status.data_ptr())

    def call(**over):
        a = dict(good, **over)
        return lib.bmhrl_crop_segments(a["src"], a["src_len"], a["durations"], a["V"], a["S_pad"], a["D"], a["seg_video"],
                                       a["seg_times"], a["P"], a["pad"], a["T_out"], a["out"], a["lengths"], a["lo"],
                                       a["status"], ops.stream())

    for name in ("src", "src_len", "durations", "seg_video", "seg_times", "out", "lengths", "status"):
        assert call(**{name: None}) == -22, name
    for name in ("V", "P", "D", "T_out", "S_pad"):
        assert call(**{name: 0}) == -22 and call(**{name: -3}) == -22, name
    torch.cuda.synchronize()
    assert status.tolist() == [9, 9] and bool((out == 5.0).all())   # nothing was launched, not even the clear
    assert call(lo=None) == 0 and call() == 0                       # lo is optional
    torch.cuda.synchronize()
    assert status.tolist() == [0, 0] and torch.equal(out.cpu(), files.packed["rgb"])

    ok = (src, src_len, durations, video, times, 1.0, T)
    ops.crop_segments(*ok)
    for i, bad in ((0, src.double()), (0, src[:, :, :-1]), (0, src[0]), (1, src_len.long()), (1, src_len[:1]),
                   (2, durations.float()), (3, video.long()), (3, video[:-1]), (4, times.float()), (4, times[:, :1]),
                   (4, times.t().contiguous().t()), (6, 0), (6, -1)):
        args = list(ok)
        args[i] = bad
        with pytest.raises(ValueError):
            ops.crop_segments(*args)
    with pytest.raises(ValueError):
        ops.crop_segments(*ok, out=out[:, :-1])
    for i in range(5):
        args = list(ok)
        args[i] = args[i].cpu()
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.crop_segments(*args)
    torch.cuda.synchronize()


def test_capture_and_replay(dev, files):
    from bmhrl_amd import ops
    name, lens, pad = STACKS[2]
    src = files.stacks[name].to(dev)
    src_len, durations, video, times = device_args(dev, lens, C.DURATIONS, files.segs)
    T = 5                                                            # below the longest crop: status[0] counts on every run
    eager = [t.clone() for t in ops.crop_segments(src, src_len, durations, video, times, pad, T)]
    assert int(eager[3][0]) > 0
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g):
            got = ops.crop_segments(src, src_len, durations, video, times, pad, T)
    torch.cuda.current_stream().wait_stream(s)
    for i in range(2):                                               # (no synchronise in front of the first replay)
        got[0].fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        print("replay", i, "status", got[3].tolist())
        for what, a, b in zip(("out", "lengths", "lo", "status"), got, eager):
            assert torch.equal(a, b), (what, a, b)                  # (status: zeroed again by the graph's own clear)
    # new times in the same buffers: the replay crops those
    times.copy_(torch.tensor([(0.0, 1.0)] * times.shape[0], dtype=torch.float64))
    g.replay()
    torch.cuda.synchronize()
    want = ops.crop_segments(src, src_len, durations, video, times, pad, T)
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and got[3].tolist() == [0, 0]
