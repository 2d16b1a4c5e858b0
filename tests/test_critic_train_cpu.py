"""Host side of critic training: segment_examples, CriticTrainer's argument checks, the saved state dict's keys and the
oracle's loss against the closed form the head + loss kernel implements."""
import json

import pytest
import torch

from bmhrl_amd import synthetic as syn
from tests import critic_reference as R

STOI = {"<s>": 2, "</s>": 3, "<pad>": 1, "<unk>": 0, "a": 4, "man": 5, "runs": 6, "then": 7, "he": 8, "stops": 9}
RECORDS = [{"captions": ["a man runs then he stops", "a dog runs"], "seg_labels": [[0, 0, 1, 0, 0, 1], [0, 0, 1]]},
           {"captions": ["he stops"], "seg_labels": [[0, 1]]}]


def _examples(records, max_len):
    from bmhrl_amd.critic_train import segment_examples
    return segment_examples(records, STOI, "<s>", "</s>", "<pad>", 0, max_len)


def test_segment_examples_end_token_leading_zero_pad_unk():
    tokens, labels = _examples(RECORDS, 7)
    assert tokens.dtype == torch.int64 and labels.dtype == torch.float32 and tokens.shape == labels.shape == (3, 8)
    assert tokens[0].tolist() == [2, 4, 5, 6, 7, 8, 3, 1]              # <s>, words, last word -> </s>, pad
    assert labels[0].tolist() == [0, 0, 0, 1, 0, 0, 1, 0]              # leading 0, the labels, pad label 0
    assert tokens[1].tolist() == [2, 4, 0, 3, 1, 1, 1, 1]              # "dog" is unknown
    assert labels[1].tolist() == [0, 0, 0, 1, 0, 0, 0, 0]
    assert tokens[2].tolist() == [2, 8, 3, 1, 1, 1, 1, 1]


def test_segment_examples_cut():
    tokens, labels = _examples(RECORDS, 3)
    assert tokens.shape == (3, 4)
    assert tokens[0].tolist() == [2, 4, 5, 6] and labels[0].tolist() == [0, 0, 0, 1]
    assert tokens[1].tolist() == [2, 4, 0, 3]


def test_segment_examples_mismatch_names_the_caption():
    bad = [{"captions": ["a man runs"], "seg_labels": [[0, 1]]}]
    with pytest.raises(ValueError, match="a man runs"):
        _examples(bad, 5)


def test_segment_examples_json_path(tmp_path):
    p = tmp_path / "segments.json"
    p.write_text(json.dumps(RECORDS))
    for path in (p, str(p)):
        tokens, labels = _examples(path, 7)
        ref_t, ref_l = _examples(RECORDS, 7)
        assert torch.equal(tokens, ref_t) and torch.equal(labels, ref_l)


def test_trainer_argument_errors():
    from bmhrl_amd.critic_train import CriticTrainer
    from bmhrl_amd.model.bm_hrl_agent import SegmentCritic
    embed = lambda tok: torch.zeros(*tok.shape, 12)
    with pytest.raises(ValueError, match="multiple of 4"):
        CriticTrainer(SegmentCritic(syn.default_cfg(d_model_caps=10)), embed, 1)
    good = SegmentCritic(syn.default_cfg(d_model_caps=12))
    with pytest.raises(TypeError, match="callable"):
        CriticTrainer(good, None, 1)
    for kw in (dict(lr=0.0), dict(pos_weight=0.0), dict(grad_clip=-1.0)):
        with pytest.raises(ValueError):
            CriticTrainer(good, embed, 1, **kw)
    assert not any(p.requires_grad for p in good.parameters())          # a refused constructor leaves the critic frozen
    tr = CriticTrainer(good, embed, 1)
    assert all(p.requires_grad for p in good.parameters())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tr.step(torch.full((2, 3), 5), torch.zeros(2, 3))
    tr.close()
    assert not any(p.requires_grad for p in good.parameters())


def test_saved_state_dict_has_the_reference_keys(tmp_path):
    from bmhrl_amd.critic_train import CriticTrainer
    from bmhrl_amd.model.bm_hrl_agent import SegmentCritic
    crit = SegmentCritic(syn.default_cfg(d_model_caps=12))
    tr = CriticTrainer(crit, lambda tok: torch.zeros(*tok.shape, 12), 1)
    path = str(tmp_path / "critic.cp")
    tr.save(path)
    tr.close()
    saved = torch.load(path)
    fresh = SegmentCritic(syn.default_cfg(d_model_caps=12))
    assert list(saved) == list(fresh.state_dict()) and set(saved) == set(syn.critic_shapes(12))
    assert [n for n, _ in crit.named_parameters()] == R.PARAM_NAMES
    assert [id(p) for p in crit.train_parameters()] == [id(dict(crit.named_parameters())[n]) for n in
                                                        R.PARAM_NAMES[:24] + ["relu.alpha", "relu.beta", "relu2.alpha", "relu2.beta",
                                                                              "lin.weight", "lin.bias"]]
    loaded = SegmentCritic(syn.default_cfg(d_model_caps=12, rl_critic_path=path))
    assert not any(p.requires_grad for p in loaded.parameters())


@pytest.mark.parametrize("pw", [None, 1.0, 3.0])
def test_oracle_loss_is_the_closed_form(pw):
    g = torch.Generator().manual_seed(0)
    score = 8.0 * torch.randn(5, 7, 1, generator=g, dtype=torch.float64)
    labels = (torch.rand(5, 7, generator=g) < 0.5).float()
    mask = torch.rand(5, 7, generator=g) < 0.8
    a, b = R.masked_bce(score, labels, mask, pw), R.closed_form_bce(score, labels, mask, pw)
    assert abs(float(a - b)) <= 1e-14 * abs(float(a))
    # and its derivative: ds = mask (sigmoid(s) (1 - y + pw y) - pw y) / sum(mask)
    s = score.clone().requires_grad_(True)
    R.masked_bce(s, labels, mask, pw).backward()
    p, y, m = 1.0 if pw is None else pw, labels.double(), mask.double()
    ds = m * (torch.sigmoid(score.squeeze(-1)) * (1 - y + p * y) - p * y) / m.sum()
    assert float((s.grad.squeeze(-1) - ds).abs().max()) <= 1e-15
