"""CPU checks of the DETR word loss: the float64 restatement (tests/word_loss_reference.py) reproduces the fixture recorded
from the reference (tests/golden/word_loss.npz), the C ABI carries the four entry points, and the wrappers refuse CPU tensors."""
import os

import numpy as np
import pytest

from tests import word_loss_reference as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "word_loss.npz")
NAMES = ("bmhrl_word_cost", "bmhrl_lsa_match", "bmhrl_word_loss", "bmhrl_word_loss_bwd")


def fixture_cases():
    z = np.load(GOLDEN)
    pad, eos = int(z["pad_eos"][0]), float(z["pad_eos"][1])
    return [dict(logits=z[f"c{c}_logits"].astype(np.float32), captions=z[f"c{c}_captions"], class_map=z[f"c{c}_class_map"],
                 loss=float(z[f"c{c}_loss"]), grad=z[f"c{c}_grad"], match_i=z[f"c{c}_match_i"], match_j=z[f"c{c}_match_j"],
                 match_n=z[f"c{c}_match_n"], pad=pad, eos=eos) for c in range(int(z["n_cases"]))]


def test_fixture_holds_the_cases_the_loss_is_pinned_on():
    cases = fixture_cases()
    assert sorted(c["logits"].shape for c in cases) == [(3, 100, 41), (3, 100, 173)]
    caps = np.concatenate([c["captions"] for c in cases])
    words = [row[row != 1] for row in caps]
    assert any(len(w) == 0 for w in words) and any(len(w) == caps.shape[1] for w in words)          # all-pad row, full row
    assert any(len(set(w.tolist())) < len(w) for w in words)                                        # a duplicated word
    assert any(0 < len(w) < len(r) and (r[:len(w)] != 1).all() for w, r in zip(words, caps))        # trailing pads only
    assert any(len(w) and (np.diff(np.nonzero(r != 1)[0]) > 1).any() for w, r in zip(words, caps))  # pads between words


def test_restatement_reproduces_the_reference_fixture():
    for c in fixture_cases():
        cls, loss, grad, qot, n = ref.word_loss(c["logits"], c["captions"], c["pad"], c["eos"])
        assert np.array_equal(cls, c["class_map"])
        assert np.array_equal(n, c["match_n"])
        assert abs(loss - c["loss"]) <= 1e-6 * abs(c["loss"])
        assert np.abs(grad - c["grad"]).max() <= 1e-6 * np.abs(c["grad"]).max()
        # the reference's tuples, scored directly, give the same map
        mq = np.full_like(qot, -1)
        for b in range(len(n)):
            k = int(c["match_n"][b])
            mq[b, c["match_j"][b, :k]] = c["match_i"][b, :k]
            assert (np.diff(c["match_i"][b, :k]) > 0).all()
        words, n2 = ref.compact(c["captions"], c["pad"], c["logits"].shape[2])
        assert np.array_equal(ref.class_map(words, n2, mq, 100, c["logits"].shape[2]), c["class_map"])


def test_restatement_drops_pads_anywhere_and_ids_outside_the_classes():
    words, n = ref.compact(np.array([[1, 5, 1, 9, 10, -3, 4, 1], [1, 1, 1, 1, 1, 1, 1, 1]]), 1, 11)
    assert words.tolist() == [[5, 9, 4, -1, -1, -1, -1, -1], [-1] * 8] and n.tolist() == [3, 0]


def test_prototypes_are_declared_and_exported():
    from bmhrl_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    # pure argument checks, nothing is launched: null pointers and the shape limits are refused
    assert lib.bmhrl_word_cost(None, 8, None, 4, 1, 1.0, 1, 4, 4, 8, None, None, None, None, None, None, None, None) == -22
    assert lib.bmhrl_lsa_match(None, 1, 1, 1, None, 1, 4, 4, None, None) == -22
    assert lib.bmhrl_word_loss(None, None, None, None, None, None, None, 0.1, 1, 4, 4, 8, None, None, None, None) == -22
    assert lib.bmhrl_word_loss_bwd(None, 8, None, None, None, None, None, None, None, 8, 1, 4, 8, None) == -22


def test_ops_refuse_cpu_tensors():
    import torch
    from bmhrl_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.word_cost(torch.zeros(1, 4, 8), torch.zeros(1, 3, dtype=torch.int64), 1, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.lsa_match(torch.zeros(1, 4, 3), torch.zeros(1, dtype=torch.int32))


def test_python_layers_export_the_reference_names():
    from bmhrl_amd.epoch_loops import captioning_bmrl_loops as loops
    from bmhrl_amd.loss.hungarian_matcher import HungarianMatcher, loss_labels
    assert loops.loss_labels is loss_labels
    m = HungarianMatcher()
    assert m.cost_class == 1 and callable(m.match)
