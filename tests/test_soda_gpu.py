"""SODA_c on the GPU (csrc/soda.hip through ops.meteor_matrix / ops.soda_dp and bmhrl_amd/evaluate.py; DESIGN.md section
25).  The matrix launch: every cell has the bits of the per-prefix launch's column L - 1 for the same pair (ops.meteor) and
lies within 1e-12 relative of the restatement, section 19's bound.  The DP launch uses IEEE +, -, x, /, min and max alone:
it equals the restatement (tests/soda_reference.py) bit for bit on the same S."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import meteor_reference as mr
from tests import soda_reference as sr
from tests.conftest import GOLDEN
from tests.test_loops_gpu import setup  # noqa: F401  (the synthetic loader and agent of the loop tests)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ST = mr.DictStemmer()
RTOL = 1e-12
STAGES = [(False, False), (True, False), (False, True), (True, True)]


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def offsets(groups):
    P = np.array([len(h) for h, _ in groups], dtype=np.int64)
    R = np.array([len(r) for _, r in groups], dtype=np.int64)
    off = lambda n, dt: np.concatenate([[0], np.cumsum(n)]).astype(dt)                                   # noqa: E731
    return off(P, np.int32), off(R, np.int32), off(P * R, np.int64)


class Sentences:
    """the distinct hypotheses (vocab ids) and references (strings) of a test on the device, with their tables"""

    def __init__(self, itos, hyp, caps, stem, syn):
        from bmhrl_amd.rewards import MeteorTables
        self.itos, self.hyp_np, self.caps = itos, np.asarray(hyp, dtype=np.int64), caps
        self.stem, self.syn = (ST.stem if stem else None), (mr.dict_synonyms if syn else None)
        t = MeteorTables(itos, ST if stem else False, mr.dict_synonyms if syn else False)
        ref_w, ref_s = t.encode(caps)
        R = max(1, max(len(r) for r in ref_w))
        w, s = np.zeros((len(caps), R), dtype=np.int32), np.zeros((len(caps), R), dtype=np.int32)
        for k, (rw, rs) in enumerate(zip(ref_w, ref_s)):
            w[k, :len(rw)], s[k, :len(rs)] = rw, rs
        self.vmap, self.vstem, self.syn_off, self.syn_ids = dev(t.vmap), dev(t.vstem), dev(t.syn_off), dev(t.syn_ids)
        self.hyp, self.ref, self.ref_stem = dev(self.hyp_np), dev(w), dev(s) if stem else None
        self.ref_len = dev(np.array([len(r) for r in ref_w], dtype=np.int32))

    def matrix(self, groups, S=None):
        """ops.meteor_matrix over groups [(hypothesis indices, reference indices)] -> the flat cells (device)"""
        from bmhrl_amd import ops
        hyp_off, ref_off, cell_off = offsets(groups)
        hyp_idx = np.array([i for h, _ in groups for i in h], dtype=np.int32)
        ref_idx = np.array([j for _, r in groups for j in r], dtype=np.int32)
        if S is None:
            S = torch.full((int(cell_off[-1]),), -3.0, dtype=torch.float64, device=DEV)
        ops.meteor_matrix(self.hyp, self.vmap, self.vstem, self.syn_off, self.syn_ids, self.ref, self.ref_stem, self.ref_len,
                          dev(hyp_idx), dev(ref_idx), dev(hyp_off), dev(ref_off), dev(cell_off), 0.9, 3.0, 0.5, S)
        return S

    def cells(self, groups):
        return [(i, j) for h, r in groups for i in h for j in r]

    def by_the_prefix_launch(self, cells):
        """column L - 1 of ops.meteor for the cells materialised as pairs"""
        from bmhrl_amd import ops
        hi, ri = torch.tensor([i for i, _ in cells], device=DEV), torch.tensor([j for _, j in cells], device=DEV)
        B, L = len(cells), self.hyp.shape[1]
        scores = torch.empty(B, L, dtype=torch.float64, device=DEV)
        delta = torch.empty(B, L, dtype=torch.float32, device=DEV)
        ops.meteor(self.hyp[hi], self.vmap, self.vstem, self.syn_off, self.syn_ids, self.ref[ri],
                   self.ref_stem[ri] if self.ref_stem is not None else None, self.ref_len[ri], 0.9, 3.0, 0.5, scores, delta)
        return scores[:, L - 1].cpu().numpy()

    def by_the_restatement(self, cells, reduced=False):
        V = len(self.itos)
        sent = [" ".join(self.itos[i] if 0 <= i < V else "" for i in row) for row in self.hyp_np.tolist()]
        if reduced:
            return np.array([mr.meteor_scores_reduced(self.itos, self.hyp_np[i], self.caps[j], self.stem, self.syn)[-1]
                             for i, j in cells])
        return np.array([mr.meteor_sentence(sent[i], self.caps[j], self.stem, self.syn) for i, j in cells])

    def check(self, groups, reduced=False):
        cells = self.cells(groups)
        got = self.matrix(groups).cpu().numpy()
        assert got.shape == (len(cells),)
        assert got.tobytes() == self.by_the_prefix_launch(cells).tobytes()
        np.testing.assert_allclose(got, self.by_the_restatement(cells, reduced), rtol=RTOL, atol=0)
        return got


@pytest.mark.parametrize("stem,syn", STAGES)
def test_matrix_on_the_random_cases(stem, syn):
    itos, caps, hyp = mr.random_case(3)
    B, L = hyp.shape
    V = len(itos)
    extra = np.full((3, L), -1, dtype=np.int64)                     # no word; one word; one word behind tokens without one
    extra[1, 0] = 25
    extra[2, :4] = [4, V + 3, 5, 10]
    s = Sentences(itos, np.concatenate([hyp, extra]), caps, stem, syn)
    assert caps[3] == "" and caps[11] == ""                         # references of 0 words
    rng = np.random.RandomState(1)
    pick = lambda n: rng.randint(0, B, n).tolist()                                                        # noqa: E731
    groups = [([5], [7]), ([], [1, 2, 3]), ([6], pick(17)), ([], []), (pick(17), [9]), ([1, 2], []),
              ([5, 30, 8], [3, 7, 11, 0, 31]),                      # hypothesis 5 again, two empty references
              ([B, B + 1, B + 2, 4], [3, 0, 6])]
    got = s.check(groups)
    off = offsets(groups)[2]
    assert (got != 0).mean() > 0.4
    deg = got[off[-2]:].reshape(4, 3)
    assert not deg[0].any() and not deg[:, 0].any() and deg[3, 1:].all()
    # a sentinel pattern around S survives, and two runs give equal bits
    n = len(got)
    buf = torch.full((n + 16,), -7.0, dtype=torch.float64, device=DEV)
    again = s.matrix(groups, buf[8:8 + n]).cpu().numpy()
    assert again.tobytes() == got.tobytes()
    assert (buf[:8] == -7.0).all() and (buf[8 + n:] == -7.0).all()


def test_matrix_past_a_wave_of_lanes():
    """reference lengths 64 / 65 / 129 and hypotheses of 64 / 65 words: one past a wave of reference lanes and of
    hypothesis slots"""
    itos = mr.case_vocab()
    rng = np.random.RandomState(65)
    pool = [w.lower() for w in itos[6:]] + ["walker", "great", "feline", "oov"]
    caps = [" ".join(pool[rng.randint(len(pool))] for _ in range(n)) for n in (64, 65, 129)]
    hyp = rng.randint(6, len(itos), (2, 65))
    hyp[0, 64] = -1
    for stem, syn in ((True, True), (False, False)):
        got = Sentences(itos, hyp, caps, stem, syn).check([([0, 1], [0, 1, 2])])
        assert got.all()


def test_matrix_at_the_limits():
    """L = 256, R = 512 (two waves per row), with shorter references in the same row"""
    from bmhrl_amd import ops
    assert (ops.REWARDS_MAX_L, ops.REWARDS_MAX_R) == (256, 512)
    itos = mr.case_vocab()
    rng = np.random.RandomState(512)
    pool = [w.lower() for w in itos[6:]] + ["walker", "great", "feline", "oov"]
    caps = [" ".join(pool[rng.randint(len(pool))] for _ in range(n)) for n in (512, 100, 64)]
    hyp = rng.randint(6, len(itos), (1, 256))
    got = Sentences(itos, hyp, caps, True, True).check([([0], [0, 1, 2])], reduced=True)
    assert got.all()


# ---- the DP launch
def run_dp(cases, tious):
    """ops.soda_dp over [(prediction segments, reference segments, S)] -> (G, T, 4) numpy"""
    from bmhrl_amd import ops
    hyp_off, ref_off, cell_off = offsets([(p, r) for p, r, _ in cases])
    flat = lambda rows: np.array([x for c in rows for x in c], dtype=np.float64)                         # noqa: E731
    pred = flat([p for p, _, _ in cases]).reshape(-1, 2)
    ref = flat([r for _, r, _ in cases]).reshape(-1, 2)
    S = np.array([v for _, _, s in cases for row in s for v in row], dtype=np.float64)
    out = ops.soda_dp(dev(pred), dev(ref), dev(hyp_off), dev(ref_off), dev(cell_off), dev(S),
                      dev(np.asarray(tious, dtype=np.float64)))
    assert out.dtype == torch.float64 and tuple(out.shape) == (len(cases), len(tious), 4)
    return out.cpu().numpy()


def want_dp(cases, tious):
    return np.array([sr.group_scores(p, r, s, tious) for p, r, s in cases], dtype=np.float64).reshape(len(cases), len(tious), 4)


def shaped_case(rng, P, R):
    """R references tiling [0, 100] with small overlaps, P predictions that are jittered copies of references, by time"""
    if P == 0 or R == 0:
        return [[0.0, 1.0]] * P, [[0.0, 1.0]] * R, [[0.0] * R for _ in range(P)]
    cuts = np.sort(rng.uniform(0.0, 100.0, R - 1)).tolist()
    refs = [[a, b + rng.uniform(0, 0.2)] for a, b in zip([0.0] + cuts, cuts + [100.0])]
    preds = []
    for k in np.sort(rng.randint(0, R, P)):
        a, b = refs[k]
        preds.append([a + rng.uniform(-0.2, 0.2) * (b - a), b + rng.uniform(-0.2, 0.2) * (b - a)])
    preds.sort(key=lambda s: (s[0], s[1]))
    S = rng.uniform(0.0, 1.0, (P, R))
    S[rng.rand(P, R) < 0.2] = 0.0
    return [[float(a), float(b)] for a, b in preds], [[float(a), float(b)] for a, b in refs], S.tolist()


DP_SHAPES = [(1, 1), (1, 9), (9, 1), (63, 3), (64, 3), (65, 3), (5, 63), (5, 64), (5, 65), (5, 256), (1000, 27)]


def test_dp_shapes_equal_the_restatement_bit_for_bit():
    rng = np.random.RandomState(25)
    shapes = DP_SHAPES[:3] + [(0, 4)] + DP_SHAPES[3:9] + [(3, 0), (0, 0)] + DP_SHAPES[9:]
    cases = [shaped_case(rng, P, R) for P, R in shapes]
    got, want = run_dp(cases, sr.CASE_TIOUS), want_dp(cases, sr.CASE_TIOUS)
    for k, (P, R) in enumerate(shapes):
        assert got[k].tobytes() == want[k].tobytes(), (P, R, got[k], want[k])
        if P == 0 or R == 0:
            assert not got[k].any()
        else:
            assert got[k, 0, 0] > 0                                  # (the shapes do match something at 0.3)
    assert got[-1, 0, 0] > 5 and got[-2, 0, 0] > 1
    assert run_dp(cases, sr.CASE_TIOUS).tobytes() == got.tobytes()


def test_dp_on_the_shared_random_cases():
    cases = sr.random_cases()
    got, want = run_dp(cases, sr.CASE_TIOUS), want_dp(cases, sr.CASE_TIOUS)
    assert got.tobytes() == want.tobytes()
    assert np.isfinite(got).all() and not got[13].any()              # the all-zero case: 0, never NaN
    assert (got[:, 0, 0] > got[:, 3, 0]).mean() > 0.5                # the thresholds matter


@pytest.mark.parametrize("T", [1, 16])
def test_dp_threshold_counts(T):
    cases = sr.random_cases()[:9]
    tious = np.linspace(0.05, 0.95, T).tolist() if T > 1 else [0.5]
    assert run_dp(cases, tious).tobytes() == want_dp(cases, tious).tobytes()


def test_the_two_launches_back_to_back():
    """S goes from the matrix launch to the DP launch on the device; the result against the restatement on its own S"""
    itos, caps, hyp = mr.random_case(3)
    s = Sentences(itos, hyp, caps, True, True)
    rng = np.random.RandomState(2)
    groups = [(rng.randint(0, 32, P).tolist(), rng.randint(0, 32, R).tolist()) for P, R in ((4, 3), (0, 2), (7, 5), (1, 1))]
    segs = [shaped_case(rng, len(h), len(r))[:2] for h, r in groups]
    from bmhrl_amd import ops
    hyp_off, ref_off, cell_off = offsets(groups)
    S = s.matrix(groups)
    flat = lambda k: np.array([x for sg in segs for x in sg[k]], dtype=np.float64).reshape(-1, 2)        # noqa: E731
    got = ops.soda_dp(dev(flat(0)), dev(flat(1)), dev(hyp_off), dev(ref_off), dev(cell_off), S,
                      dev(np.asarray(sr.CASE_TIOUS))).cpu().numpy()
    S_host = S.cpu().numpy()
    cases = [(p, r, S_host[cell_off[g]:cell_off[g + 1]].reshape(len(p), len(r)).tolist()) for g, (p, r) in enumerate(segs)]
    assert got.tobytes() == want_dp(cases, sr.CASE_TIOUS).tobytes() and got[:, 0, 0].any()


# ---- refusals
def test_matrix_refusals():
    from bmhrl_amd import _lib, ops
    lib = _lib.load()
    itos, caps, hyp = mr.random_case(5, B=4, L=8)
    s = Sentences(itos, hyp, caps, True, True)
    ld = ops.REWARDS_MAX_L + 1
    wide = torch.zeros(4, ld, dtype=torch.int64, device=DEV)
    refs = torch.zeros(2, 4, ops.REWARDS_MAX_R + 1, dtype=torch.int32, device=DEV)
    S = torch.zeros(64, dtype=torch.float64, device=DEV)
    good = dict(hyp_idx=[0, 1, 2], ref_idx=[3, 2, 1, 0], hyp_off=[0, 1, 1, 3], ref_off=[0, 2, 2, 4], cell_off=[0, 2, 2, 6])

    def call(null=(), L=8, R=20, Nh=4, Nr=4, ldh=ld, ldr=ops.REWARDS_MAX_R + 1, G=3, n_pred=None, n_ref=None, n_cells=None,
             V=None, **arrays):
        a = dict(good, **arrays)
        t = dict(hyp=wide, vmap=s.vmap, vstem=s.vstem, syn_off=s.syn_off, syn_ids=s.syn_ids, ref=refs[0], ref_stem=refs[1],
                 ref_len=s.ref_len, S=S)
        for k in ("hyp_idx", "ref_idx", "hyp_off", "ref_off"):
            t[k] = torch.tensor(a[k], dtype=torch.int32, device=DEV)
        t["cell_off"] = torch.tensor(a["cell_off"], dtype=torch.int64, device=DEV)
        p = {k: (None if k in null else v.data_ptr()) for k, v in t.items()}
        return lib.bmhrl_meteor_matrix(
            p["hyp"], ldh, Nh, L, p["vmap"], p["vstem"], s.vmap.numel() if V is None else V, p["syn_off"], p["syn_ids"],
            s.syn_ids.numel(), p["ref"], p["ref_stem"], ldr, p["ref_len"], Nr, R, p["hyp_idx"],
            len(a["hyp_idx"]) if n_pred is None else n_pred, p["ref_idx"], len(a["ref_idx"]) if n_ref is None else n_ref,
            p["hyp_off"], p["ref_off"], p["cell_off"], G, 0.9, 3.0, 0.5, p["S"], a["cell_off"][-1] if n_cells is None else n_cells,
            ops.stream())

    assert call() == 0 and call(L=ops.REWARDS_MAX_L, R=ops.REWARDS_MAX_R) == 0
    for name in ("hyp", "vmap", "ref", "ref_len", "hyp_idx", "ref_idx", "hyp_off", "ref_off", "cell_off", "S"):
        assert call(null=(name,)) == -22, name
    assert call(null=("syn_off",)) == -22 and call(null=("syn_ids",)) == -22 and call(null=("syn_off", "syn_ids")) == 0
    assert call(null=("ref_stem",)) == -22 and call(null=("vstem",)) == 0 and call(null=("vstem", "ref_stem")) == 0
    assert call(G=0) == -22 and call(G=-1) == -22
    assert call(L=ops.REWARDS_MAX_L + 1) == -22 and call(R=ops.REWARDS_MAX_R + 1) == -22 and call(L=0) == -22 and call(R=0) == -22
    assert call(ldh=7) == -22 and call(ldr=19) == -22 and call(Nh=0) == -22 and call(Nr=0) == -22 and call(V=0) == -22
    assert call(hyp_off=[0, 2, 1, 3]) == -22 and call(ref_off=[0, 3, 2, 4]) == -22              # descending
    assert call(hyp_off=[1, 1, 1, 3]) == -22 and call(ref_off=[1, 2, 2, 4]) == -22              # not from 0
    assert call(cell_off=[1, 3, 3, 7]) == -22 and call(cell_off=[0, 2, 2, 5]) == -22            # not from 0; not P x R
    assert call(cell_off=[0, 1, 2, 6]) == -22 and call(cell_off=[0, 2, 1, 6]) == -22
    assert call(n_pred=2) == -22 and call(n_ref=3) == -22 and call(n_cells=7) == -22            # not spanning the arrays
    assert call(hyp_idx=[0, 4, 2]) == -22 and call(hyp_idx=[0, -1, 2]) == -22                   # outside [0, Nh)
    assert call(ref_idx=[3, 2, 1, 4]) == -22 and call(ref_idx=[-1, 2, 1, 0]) == -22 and call(Nh=2) == -22 and call(Nr=3) == -22
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.meteor_matrix(s.hyp.int(), s.vmap, s.vstem, s.syn_off, s.syn_ids, s.ref, s.ref_stem, s.ref_len, dev(np.zeros(1, np.int32)),
                          dev(np.zeros(1, np.int32)), dev(np.array([0, 1], np.int32)), dev(np.array([0, 1], np.int32)),
                          dev(np.array([0, 1], np.int64)), 0.9, 3.0, 0.5, S[:1])


def test_dp_refusals():
    from bmhrl_amd import _lib, ops
    lib = _lib.load()
    f64 = dict(dtype=torch.float64, device=DEV)
    pred, ref = torch.zeros(3, 2, **f64), torch.zeros(ops.SODA_MAX_REFS + 1, 2, **f64)
    S, tious, out = torch.zeros(1024, **f64), torch.full((17,), 0.5, **f64), torch.zeros(3 * 17 * 4, **f64)
    good = dict(hyp_off=[0, 1, 1, 3], ref_off=[0, 2, 2, 4], cell_off=[0, 2, 2, 6])

    def call(null=(), G=3, T=4, n_pred=3, n_ref=4, n_cells=None, **arrays):
        a = dict(good, **arrays)
        t = dict(pred=pred, ref=ref, S=S, tious=tious, out=out)
        for k in ("hyp_off", "ref_off"):
            t[k] = torch.tensor(a[k], dtype=torch.int32, device=DEV)
        t["cell_off"] = torch.tensor(a["cell_off"], dtype=torch.int64, device=DEV)
        p = {k: (None if k in null else v.data_ptr()) for k, v in t.items()}
        return lib.bmhrl_soda_dp(p["pred"], n_pred, p["ref"], n_ref, p["hyp_off"], p["ref_off"], p["cell_off"], G, p["S"],
                                 a["cell_off"][-1] if n_cells is None else n_cells, p["tious"], T, p["out"], ops.stream())

    assert call() == 0 and call(T=1) == 0 and call(T=ops.SODA_MAX_T) == 0
    for name in ("pred", "ref", "hyp_off", "ref_off", "cell_off", "S", "tious", "out"):
        assert call(null=(name,)) == -22, name
    assert call(G=0) == -22 and call(T=0) == -22 and call(T=ops.SODA_MAX_T + 1) == -22
    assert call(hyp_off=[0, 2, 1, 3]) == -22 and call(ref_off=[0, 3, 2, 4]) == -22
    assert call(hyp_off=[1, 1, 1, 3]) == -22 and call(ref_off=[1, 2, 2, 4]) == -22
    assert call(cell_off=[1, 3, 3, 7]) == -22 and call(cell_off=[0, 2, 2, 5]) == -22 and call(cell_off=[0, 2, 1, 6]) == -22
    assert call(n_pred=2) == -22 and call(n_ref=5) == -22 and call(n_cells=5) == -22
    R = ops.SODA_MAX_REFS
    assert call(G=1, n_pred=1, n_ref=R, hyp_off=[0, 1], ref_off=[0, R], cell_off=[0, R]) == 0
    assert call(G=1, n_pred=1, n_ref=R + 1, hyp_off=[0, 1], ref_off=[0, R + 1], cell_off=[0, R + 1]) == -22
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.soda_dp(pred.float(), ref[:4], dev(np.array(good["hyp_off"], np.int32)), dev(np.array(good["ref_off"], np.int32)),
                    dev(np.array(good["cell_off"], np.int64)), S[:6], tious[:4])


# ---- the evaluator
def test_fixture_end_to_end_with_soda():
    from bmhrl_amd.evaluate import METRICS, SODA_METRICS, DenseCaptionEvaluator, tokenize
    with open(os.path.join(GOLDEN, "caption_eval.json")) as f:
        fx = json.load(f)
    ev = DenseCaptionEvaluator(fx["ground_truths"], fx["submission"], fx["tious"], fx["max_proposals"], device=DEV,
                               stemmer=ST, synonyms=mr.dict_synonyms, soda=True)
    ev.evaluate()
    assert list(ev.scores) == list(METRICS) + list(SODA_METRICS)
    for name in METRICS:                                             # the seven metrics as today
        np.testing.assert_allclose(ev.scores[name], fx["scores"][name], rtol=RTOL, atol=0, err_msg=name)
    want, per_video = sr.evaluate(fx["ground_truths"], fx["submission"], fx["tious"], fx["max_proposals"], tokenize, ST.stem,
                                  mr.dict_synonyms)
    for name in SODA_METRICS:
        print(name, ev.scores[name], want[name])
        assert len(ev.scores[name]) == len(fx["tious"])
        np.testing.assert_allclose(ev.scores[name], want[name], rtol=RTOL, atol=0, err_msg=name)
    assert list(ev.soda_per_video) == list(per_video)
    for vid, triples in per_video.items():
        np.testing.assert_allclose(ev.soda_per_video[vid], triples, rtol=RTOL, atol=0, err_msg=vid)
    assert any(f > 0 for t in per_video.values() for _, _, f in t) and any(t[0][2] == 0 for t in per_video.values())
    # the references by time; small chunks (one group per pair of launches) change nothing
    ev2 = DenseCaptionEvaluator(fx["ground_truths"], fx["submission"], fx["tious"], fx["max_proposals"], device=DEV,
                                stemmer=ST, synonyms=mr.dict_synonyms, soda=True, sort_references=True)
    want2, _ = sr.evaluate(fx["ground_truths"], fx["submission"], fx["tious"], fx["max_proposals"], tokenize, ST.stem,
                           mr.dict_synonyms, sort_references=True)
    got2 = ev2.evaluate_soda()
    for name in SODA_METRICS:
        np.testing.assert_allclose(got2[name], want2[name], rtol=RTOL, atol=0, err_msg=name)
    from bmhrl_amd import evaluate as E
    groups, _ = E.soda_groups(ev.ground_truths, ev.prediction)
    whole = E.soda_scores(groups, fx["tious"], ev.meteor_tables(), DEV, ev._tok)
    small = E.soda_scores(groups, fx["tious"], ev.meteor_tables(), DEV, ev._tok, max_cells=1)
    assert len(groups) > 2 and whole.tobytes() == small.tobytes()


def test_loop_reports_soda(setup, tmp_path):  # noqa: F811
    from epoch_loops.validation_loops import validation_1by1_loop
    from epoch_loops.captioning_bmrl_loops import bmhrl_greedy_decoder
    cfg, ds, loader, agent, wv, ls, bkl, dev_ = setup
    cfg.max_len, cfg.modality, cfg.log_path, cfg.max_prop_per_vid = 6, "audio_video", str(tmp_path), 100
    refs = []
    for k in range(2):                                    # references over the synthetic vocabulary's words
        gt = {f"v{j}": {"duration": 1.0, "timestamps": [[0.0, 1.0], [0.0, 0.6]],
                        "sentences": [" ".join(f"w{(7 * j + 3 * k + i) % 80}" for i in range(5)), f"W{j + 4} w{k + 5}."]}
              for j in range(4 if k else 5)}              # (v4 has no predictions)
        refs.append(str(tmp_path / f"ref{k}.json"))
        with open(refs[-1], "w") as f:
            json.dump(gt, f)
    cfg.reference_paths, cfg.tIoUs = refs, [0.3, 0.5, 0.7, 0.9]
    cfg.caption_evaluator_options = dict(device=dev_, stemmer=ST, synonyms=mr.dict_synonyms, soda=True)
    old_itos3 = ds.train_vocab.itos[3]
    ds.train_vocab.itos[3] = "</s>"
    wrapped = SimpleNamespace(module=agent, eval=agent.eval)
    agent.set_inference_mode(True)
    try:
        ds.phase = "learned_props"
        out = validation_1by1_loop(cfg, wrapped, loader, bmhrl_greedy_decoder, 0, None, evaluator="device")
        assert list(out) == cfg.tIoUs + ["Average across tIoUs"]
        for entry in out.values():
            for name in ("SODA_c", "SODA_c_Precision", "SODA_c_Recall", "METEOR"):
                assert 0.0 <= entry[name] <= 1.0, (name, entry[name])
        avg = out["Average across tIoUs"]
        assert avg["SODA_c"] == sum(out[t]["SODA_c"] for t in cfg.tIoUs) / 4.0
    finally:
        ds.phase = "train"
        ds.train_vocab.itos[3] = old_itos3
        del cfg.caption_evaluator_options
