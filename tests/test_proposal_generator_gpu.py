"""MultimodalProposalGenerator (bmhrl_amd/model/proposal_generator.py) on the MI355X against a plain-torch restatement -- the
CPU oracle's bimodal encoder, nn.Conv1d heads and the float64 loss of tests/proposal_reference.py on the same state dict --
and the proposal train / validation loops end to end on a synthetic loader.

Bounds: the relative max-norm bounds of tests/test_detr_agent_gpu.py for quantities behind a bf16 stack: 3e-2 for the
predictions and the loss, 1.5e-2 for the gradients of the head weights (the incoming gradient is rounded to bf16 for the two
weight-gradient GEMMs)."""
import json
import math
import os
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

from bmhrl_amd import synthetic as syn
from tests import proposal_reference as R

pytestmark = pytest.mark.gpu

B, TV, TA = 2, 11, 19
ANCHORS = {"video": [2.0, 4.0, 8.0, 14.0], "audio": [3.0, 6.0, 12.0]}
TARGETS = [[0, 5.0, 4.0, 0], [0, 15.5, 8.0, 1], [1, 10.2, 3.0, 2], [1, 2.1, 12.0, 3], [1, 21.0, 2.5, 4]]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bmhrl_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def rel(a, b, floor=1e-6):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), floor))


def make_cfg(**over):
    cfg = syn.tiny_cfg(d_model=1024, rl_att_heads=4, dout_p=0.0)      # the encoder configuration of the agent's loop tests
    cfg.kernel_sizes = {"video": [1, 5], "audio": [3]}
    cfg.strides = {"video": 2.0, "audio": 1.2}                          # seconds per position: 22 s and 22.8 s of features
    cfg.conv_hidden, cfg.obj_coeff, cfg.noobj_coeff = 32, 1.0, 100.0
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def make_model(dev, cfg, seed=7):
    from bmhrl_amd.model.proposal_generator import MultimodalProposalGenerator
    torch.manual_seed(seed)
    model = MultimodalProposalGenerator(cfg, ANCHORS)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items() if k.startswith("bm_enc.")}
    model.load_state_dict(syn.fill_state_dict(shapes, seed=13), strict=False)
    return model.to(dev)


def make_batch(dev, seed=0):
    b = syn.synthetic_batch(B, TV, TA, 8, 40, seed=seed, d_vid=48, d_aud=24)
    return {k: b[k] for k in ("rgb", "flow", "audio")}


class PlainHead(nn.Module):
    """the head in plain torch: the same three nn.Conv1d, applied to (B, C, S)"""

    def __init__(self, head):
        super().__init__()
        k = head.kernel_size
        d_in, d_hidden = head.conv1.in_channels, head.conv1.out_channels
        self.conv1 = nn.Conv1d(d_in, d_hidden, k, padding=k // 2)
        self.conv2 = nn.Conv1d(d_hidden, d_hidden, 1)
        self.conv3 = nn.Conv1d(d_hidden, 3 * head.n_anchors, 1)
        self.load_state_dict({k_: v.detach().cpu() for k_, v in head.state_dict().items()})     # nn.Conv1d's names and shapes
        self.double()

    def forward(self, x):
        h = torch.relu(self.conv1(x.transpose(1, 2)))
        return self.conv3(torch.relu(self.conv2(h))).transpose(1, 2).contiguous()


def restated_forward(model, cfg, fs, targets):
    """(predictions, loss, per-head sums, plain heads) in float64 on the CPU"""
    from oracle import bmhrl_oracle as O
    sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    masks = O.make_masks(fs["rgb"], fs["audio"], None, 1)
    V = O.add_posenc((fs["rgb"] + fs["flow"]).double())
    A = O.add_posenc(fs["audio"].double())
    Va, Av = O.bm_encoder(sd, "bm_enc", V, A, masks, cfg.rl_att_heads, cfg.rl_att_layers)
    preds, sums, heads = [], [], []
    for feat, mod_heads, key in ((Av, model.heads_A, "audio"), (Va, model.heads_V, "video")):
        anchors = torch.tensor(ANCHORS[key], dtype=torch.float32)
        owner, tx, tw, _, _ = R.assign(targets, anchors, cfg.strides[key], B, feat.shape[1])
        for head in mod_heads:
            plain = PlainHead(head)
            p, s, _ = R.head(plain(feat), anchors.double(), cfg.strides[key], (owner, tx, tw), cfg.obj_coeff, cfg.noobj_coeff)
            preds.append(p)
            sums.append(s)
            heads.append(plain)
    return torch.cat(preds, dim=1), sum(s[4] for s in sums), sums, heads


def test_generator_against_the_plain_torch_restatement(dev):
    cfg = make_cfg()
    model = make_model(dev, cfg).train()                        # (dout_p = 0: training mode only selects the loss path)
    fs = make_batch(dev)
    targets = torch.tensor(TARGETS, dtype=torch.float32)
    from bmhrl_amd.model.masking import make_masks
    fs_dev = {k: v.to(dev) for k, v in fs.items()}
    masks = make_masks(fs_dev, None, "audio_video", 1)
    pred, loss, losses_A, losses_V = model(fs_dev, targets.to(dev), masks)
    n_total = 1 * 3 * TA + 2 * 4 * TV
    assert tuple(pred.shape) == (B, n_total, 3) and loss.dim() == 0
    assert set(losses_A) == set(losses_V) == {"loss_x", "loss_w", "loss_obj", "loss_noobj"}
    loss.backward()

    want_pred, want_loss, want_sums, plain = restated_forward(model, cfg, fs, targets)
    want_loss.backward()
    e_pred, e_loss = rel(pred, want_pred), rel(loss, want_loss)
    print(f"generator: predictions {e_pred:.2e}  loss {e_loss:.2e}")
    assert e_pred < 3e-2 and e_loss < 3e-2
    for name, i in (("loss_x", 0), ("loss_w", 1), ("loss_obj", 2), ("loss_noobj", 3)):
        assert math.isclose(float(losses_A[name]), float(want_sums[0][i]), rel_tol=3e-2, abs_tol=1e-6), name
        assert math.isclose(float(losses_V[name]), float(want_sums[1][i] + want_sums[2][i]), rel_tol=3e-2, abs_tol=1e-6), name
    for head, ref in zip(list(model.heads_A) + list(model.heads_V), plain):
        for (name, p), (_, q) in zip(head.named_parameters(), ref.named_parameters()):
            assert p.grad is not None and tuple(p.grad.shape) == tuple(q.grad.shape), name
            e = rel(p.grad, q.grad)
            print(f"  k={head.kernel_size} {name}: gradient {e:.2e}")
            assert e < 1.5e-2, (head.kernel_size, name, e)
    assert any(p.grad is not None and float(p.grad.abs().max()) > 0 for p in model.bm_enc.parameters())   # the encoder trains too

    # the return contract without targets: the same predictions, loss 0 and empty dictionaries
    with torch.no_grad():
        pred0, loss0, a0, v0 = model(fs_dev, None, masks)
        pred1 = model(fs_dev, targets.to(dev), masks)[0]
    assert loss0 == 0 and a0 == {} and v0 == {}
    assert torch.equal(pred0, pred1) and torch.equal(pred0, pred.detach())


class Loader:
    """a two-batch loader with the attributes the loops read"""

    def __init__(self, dev, phase):
        self.dataset = SimpleNamespace(pad_idx=1, phase=phase)
        self.batches = []
        for i in range(2):
            fs = {k: v.to(dev) for k, v in make_batch(dev, seed=i).items()}
            self.batches.append({"video_ids": [f"v_{i}_{b}" for b in range(B)], "feature_stacks": fs,
                                 "targets": torch.tensor(TARGETS, dtype=torch.float32, device=dev),
                                 "duration_in_secs": [22.0, 20.5]})

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


class Board:
    def __init__(self):
        self.scalars = {}

    def add_scalar(self, tag, value, step):
        self.scalars[tag] = float(value)


def test_train_and_validation_loops(dev, tmp_path):
    from bmhrl_amd.epoch_loops.proposal_epoch_loops import train_av_loop, validation_loop
    tious = [0.3, 0.5, 0.7, 0.9]
    gt = {f"v_{i}_{b}": {"duration": [22.0, 20.5][b], "timestamps": [[t[1] - t[2] / 2, t[1] + t[2] / 2] for t in TARGETS if t[0] == b],
                         "sentences": ["a segment ." for t in TARGETS if t[0] == b]} for i in range(2) for b in range(B)}
    paths = []
    for n, drop in (("val_1.json", None), ("val_2.json", "v_1_1")):
        paths.append(str(tmp_path / n))
        with open(paths[-1], "w") as f:
            json.dump({k: v for k, v in gt.items() if k != drop}, f)
    cfg = make_cfg(modality="audio_video", grad_clip=1.0, max_prop_per_vid=10, nms_tiou_thresh=0.4, log_path=str(tmp_path / "log"),
                   reference_paths=paths, tIoUs=tious, caption_evaluator="device", device=str(dev))
    model = make_model(dev, cfg)
    optimizer = torch.optim.Adam(model.parameters(), lr=1e-3)
    before = {n: p.detach().clone() for n, p in model.named_parameters() if n.startswith("heads_")}
    loader, board = Loader(dev, "val_1"), Board()
    for epoch in range(3):
        total, acc_A, acc_V = train_av_loop(cfg, model, optimizer, loader, epoch, board)
        assert math.isfinite(total) and all(math.isfinite(v) for v in list(acc_A.values()) + list(acc_V.values()))
    assert all(not torch.equal(p.detach(), before[n]) for n, p in model.named_parameters() if n in before)
    assert {"debug/loss_epoch", "debug/lr", "debug/train_loss_x_A", "debug/train_loss_noobj_V"} <= set(board.scalars)

    best = validation_loop(cfg, model, optimizer, None, loader, 2, -1.0, board)
    assert math.isfinite(best)
    for t in tious:
        assert 0.0 <= board.scalars[f"densevid_eval_k/precision_{t}"] <= 1.0 and 0.0 <= board.scalars[f"densevid_eval_k/recall_{t}"] <= 1.0
    assert "metrics/avg_F1_at_k" in board.scalars and os.path.exists(os.path.join(cfg.log_path, "best_prop_model.pt"))
    path = os.path.join(cfg.log_path, "submissions", "prop_results_val_1_e2_maxprop10.json")
    with open(path) as f:
        sub = json.load(f)
    assert set(sub) == {"version", "external_data", "results"} and sub["results"]
    for vid, segs in sub["results"].items():
        assert vid in gt and 1 <= len(segs) <= 10
        for seg in segs:
            assert set(seg) == {"sentence", "proposal_score", "timestamp"} and len(seg["proposal_score"]) == 1
            s, e = seg["timestamp"]
            assert 0.0 <= s < e <= gt[vid]["duration"] and e - s > 0.2
