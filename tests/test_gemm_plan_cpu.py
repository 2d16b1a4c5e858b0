"""bmhrl_gemm_plan / bmhrl_gemm_group_plan on the CPU: which main loop, tile, K split and epilogue store path bmhrl_gemm
takes for a descriptor (a pure host decision: the pointers below are never dereferenced, only their alignment counts),
which descriptors it refuses, and a self-check of the error bound tests/test_gemm_paths_gpu.py holds the kernels to."""
import os

import numpy as np
import pytest

from tests import gemm_reference as gr

BASE = 1 << 20          # fake, 256-byte aligned device addresses: the plan reads their low bits only
LOOP = {"reg": 0, "glds": 1, "glds8": 2}
TILE = {"64": 0, "128": 1, "128x64": 2}
SPLIT = {"none": 0, "atomic": 1, "ordered": 2}
EPI = {"bf16": 0, "pd": 1, "generic": 2}


@pytest.fixture(scope="module")
def lib():
    tuning = [k for k in os.environ if k.startswith("BMHRL_GEMM_")]
    if tuning:
        pytest.skip(f"the table is the default plan; tuning switches set: {tuning}")
    from bmhrl_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def desc(M, N, K, *, a_trans=0, b_trans=0, lda=None, ldb=None, batch=(1, 1), f32=True, bf16=False, ldc=None, ldcb=None,
         c_off=0, epilogue=0, mask_sm=None, split=False, ws=0, accumulate=0, colsum=False, dropout_p=0.0, aux_off=0, ldaux=None,
         bias=False):
    from bmhrl_amd import _lib
    pad = lambda n: (n + 7) & ~7  # noqa: E731
    d = _lib.GemmDesc()
    d.M, d.N, d.K = M, N, K
    d.batch1, d.batch2 = batch
    d.A, d.lda, d.a_trans = BASE, lda or pad(M if a_trans else K), a_trans
    d.B, d.ldb, d.b_trans = 2 * BASE, ldb or pad(N if b_trans else K), b_trans
    if f32:
        d.C, d.ldc = 3 * BASE + 4 * c_off, ldc or N
    if bf16:
        d.Cb, d.ldcb = 4 * BASE, ldcb or pad(N)
    d.epilogue, d.alpha = epilogue, 1.0
    if epilogue in (1, 2):
        d.rowvec = 5 * BASE
    if epilogue == 1:
        d.rowvec2 = 6 * BASE
    if epilogue in (2, 3):
        d.aux, d.ldaux = 7 * BASE + 2 * aux_off, ldaux or pad(N)
    if mask_sm is not None:
        d.mask, d.mask_sm = 8 * BASE, mask_sm
    if bias:
        d.bias = 9 * BASE
    d.allow_split_k = int(split)
    if ws:
        d.split_ws, d.split_ws_elems = 10 * BASE, ws
    d.accumulate = accumulate
    if colsum:
        d.colsum = 11 * BASE
    d.dropout_p = dropout_p
    return d


def plan(lib, d):
    import ctypes as C
    from bmhrl_amd import _lib
    p = (_lib.i32 * 8)()
    rc = lib.bmhrl_gemm_plan(C.byref(d), p)
    assert rc == 0, rc
    return tuple(p)


V = 1  # vec_ok
# (descriptor, (loop, tile, stages, splits, split form, epilogue path, vec_ok)), the colsum pass checked separately
TABLE = [
    # tails in M / N below 8: the register-staged loop whatever K is
    (dict(M=1, N=1024, K=1024), ("reg", "64", 2, 1, "none", "generic", V)),
    (dict(M=3, N=1024, K=300), ("reg", "64", 2, 1, "none", "generic", V)),
    (dict(M=7, N=64, K=64), ("reg", "64", 2, 1, "none", "generic", V)),
    (dict(M=64, N=7, K=64, a_trans=1, b_trans=1), ("reg", "64", 2, 1, "none", "generic", 0)),   # (ldc = N = 7: scalar)
    (dict(M=8, N=8, K=64), ("glds", "64", 4, 1, "none", "generic", V)),
    (dict(M=9, N=63, K=65), ("reg", "64", 2, 1, "none", "generic", 0)),
    (dict(M=9, N=63, K=65, ldc=64), ("reg", "64", 2, 1, "none", "generic", V)),
    (dict(M=65, N=65, K=128, a_trans=1), ("glds", "64", 4, 1, "none", "generic", 0)),
    (dict(M=65, N=130, K=203, b_trans=1), ("reg", "64", 2, 1, "none", "generic", 0)),      # (ldc % 4 == 2)
    # 4096 x 1024 projections: 256 tiles of 128 x 128, two stages
    (dict(M=4096, N=1024, K=1024), ("glds", "128", 2, 1, "none", "generic", V)),
    (dict(M=4100, N=1030, K=203, a_trans=1, b_trans=1, ldc=1032), ("reg", "128", 2, 1, "none", "generic", V)),
    # more than 448 small tiles: two stages
    (dict(M=1024, N=2048, K=128), ("glds", "64", 2, 1, "none", "generic", V)),
    # weight gradient that stores every element once (4 stages) and the vocabulary head's d cat[x, goal] (K split)
    (dict(M=1024, N=1024, K=4096, a_trans=1, b_trans=1, split=True), ("glds", "64", 4, 1, "none", "generic", V)),
    (dict(M=480, N=364, K=10176, b_trans=1, split=True), ("glds", "64", 2, 11, "atomic", "generic", V)),
    (dict(M=480, N=364, K=10176, b_trans=1, split=True, ws=11 * 480 * 364), ("glds", "64", 2, 11, "ordered", "generic", V)),
    (dict(M=480, N=364, K=10176, b_trans=1, split=True, ws=11 * 480 * 364, accumulate=1),
     ("glds", "64", 2, 11, "ordered", "generic", V)),
    (dict(M=480, N=364, K=10172, b_trans=1, split=True), ("reg", "64", 2, 11, "atomic", "generic", V)),
    # too small a workspace: atomics (accumulate is refused then, below)
    (dict(M=480, N=364, K=10176, b_trans=1, split=True, ws=8), ("glds", "64", 2, 11, "atomic", "generic", V)),
    # a K split needs allow_split_k and a plain fp32 output (unsplit, 48 tiles: four stages)
    (dict(M=480, N=364, K=10176, b_trans=1), ("glds", "64", 4, 1, "none", "generic", V)),
    (dict(M=480, N=364, K=10176, b_trans=1, split=True, bf16=True), ("glds", "64", 4, 1, "none", "generic", V)),
    # bf16-only linear output: fast path when aligned, generic vector at ldcb % 8 == 4, scalar at an odd ldcb
    (dict(M=480, N=300, K=1024, f32=False, bf16=True, bias=True, dropout_p=0.1), ("glds", "64", 4, 1, "none", "bf16", V)),
    (dict(M=480, N=300, K=1024, f32=False, bf16=True, ldcb=308), ("glds", "64", 4, 1, "none", "generic", V)),
    (dict(M=480, N=300, K=1024, f32=False, bf16=True, ldcb=301), ("glds", "64", 4, 1, "none", "generic", 0)),
    (dict(M=480, N=300, K=1024, f32=False, bf16=True, mask_sm=300), ("glds", "64", 4, 1, "none", "generic", V)),
    # fp32 output at a 4-byte offset / odd leading dimension: scalar
    (dict(M=70, N=200, K=256, c_off=1), ("glds", "64", 4, 1, "none", "generic", 0)),
    (dict(M=70, N=200, K=256, ldc=201), ("glds", "64", 4, 1, "none", "generic", 0)),
    # softmax epilogues: fast with a key mask (mask_sm == 0), generic with a per-(m, n) mask or an fp32 output
    (dict(M=30, N=200, K=256, f32=False, bf16=True, epilogue=1, mask_sm=0), ("glds", "64", 4, 1, "none", "pd", V)),
    (dict(M=30, N=200, K=256, f32=False, bf16=True, epilogue=1, mask_sm=200), ("glds", "64", 4, 1, "none", "generic", V)),
    (dict(M=30, N=200, K=256, epilogue=1), ("glds", "64", 4, 1, "none", "generic", V)),
    (dict(M=30, N=200, K=256, f32=False, bf16=True, epilogue=2, mask_sm=0), ("glds", "64", 4, 1, "none", "pd", V)),
    (dict(M=30, N=200, K=256, f32=False, bf16=True, epilogue=2, aux_off=4, ldaux=204), ("glds", "64", 4, 1, "none", "generic", V)),
    (dict(M=30, N=200, K=256, f32=False, bf16=True, epilogue=2, aux_off=2), ("glds", "64", 4, 1, "none", "generic", 0)),
    (dict(M=30, N=200, K=260, epilogue=3), ("reg", "64", 2, 1, "none", "generic", V)),
    (dict(M=30, N=200, K=256, epilogue=3, ldc=203), ("glds", "64", 4, 1, "none", "generic", 0)),
    # batched attention products (30 caption rows x 800 keys, 4 heads x 12 samples)
    (dict(M=30, N=800, K=256, batch=(12, 4), b_trans=1), ("glds", "64", 2, 1, "none", "generic", V)),
]


@pytest.mark.parametrize("i", range(len(TABLE)))
def test_plan_table(lib, i):
    kw, want = TABLE[i]
    got = plan(lib, desc(**kw))
    loop, tile, stages, splits, form, epi, vec = want
    if lib.bmhrl_deterministic_enabled() and splits > 1:
        # BMHRL_DETERMINISTIC=1 never splits K; the split rows are the 480 x 364 products (48 tiles: four stages unsplit)
        splits, form, stages = 1, "none", 4 if loop == "glds" else stages
    assert got[:7] == (LOOP[loop], TILE[tile], stages, splits, SPLIT[form], EPI[epi], vec), (kw, got)
    assert got[7] == 0


def test_plan_splits_match_bmhrl_gemm_splits(lib):
    """plan[splits] of a plain fp32 product with allow_split_k is bmhrl_gemm_splits, over shapes on both sides of every
    threshold of tile_plan"""
    n = 0
    for M in (1, 30, 128, 300, 480, 1024, 4096):
        for N in (8, 64, 300, 364, 1024):
            for K in (64, 300, 1024, 4096, 10176):
                for batch in (1, 2, 8):
                    d = desc(M, N, K, batch=(1, batch), split=True)
                    assert plan(lib, d)[3] == lib.bmhrl_gemm_splits(M, N, K, batch), (M, N, K, batch)
                    n += 1
    assert n == 7 * 5 * 5 * 3


def test_colsum_pass_follows_deterministic_mode(lib):
    p = plan(lib, desc(480, 300, 1024, colsum=True))
    assert p[7] == lib.bmhrl_deterministic_enabled()
    assert plan(lib, desc(480, 300, 1024))[7] == 0


@pytest.mark.parametrize("kw", [
    dict(M=0, N=8, K=8), dict(M=8, N=8, K=0), dict(M=64, N=64, K=64, batch=(0, 1)),
    dict(M=64, N=64, K=64, lda=60), dict(M=64, N=64, K=64, lda=68), dict(M=64, N=64, K=100, lda=96),
    dict(M=64, N=64, K=64, a_trans=1, lda=56), dict(M=64, N=64, K=64, b_trans=1, ldb=60),
    dict(M=64, N=64, K=64, dropout_p=1.0), dict(M=64, N=64, K=64, dropout_p=-0.1),
    dict(M=64, N=64, K=64, epilogue=4),
    # accumulate adds to the fp32 output only: not with a bf16 output or column sums (both modes)
    dict(M=64, N=64, K=64, accumulate=1, bf16=True), dict(M=64, N=64, K=64, accumulate=1, colsum=True),
    # accumulate with a K split needs the ordered form: a workspace too small for it is refused, not run on atomics
    dict(M=480, N=364, K=10176, b_trans=1, split=True, ws=8, accumulate=1),
])
def test_refused_descriptors(lib, kw):
    import ctypes as C
    from bmhrl_amd import _lib
    d = desc(**kw)
    assert lib.bmhrl_gemm_plan(C.byref(d), (_lib.i32 * 8)()) == -22
    assert lib.bmhrl_gemm_group_plan(C.byref(d), 1) == -22


def test_refused_pointers_and_missing_operands(lib):
    import ctypes as C
    from bmhrl_amd import _lib
    out = (_lib.i32 * 8)()
    d = desc(64, 64, 64)
    d.A = BASE + 8                                              # operands must be 16-byte aligned
    assert lib.bmhrl_gemm_plan(C.byref(d), out) == -22
    d = desc(64, 64, 64)
    d.C = None                                                  # no output at all
    assert lib.bmhrl_gemm_plan(C.byref(d), out) == -22
    for epi, field in ((1, "rowvec"), (1, "rowvec2"), (2, "rowvec"), (2, "aux"), (3, "aux")):
        d = desc(64, 64, 64, epilogue=epi)
        setattr(d, field, None)
        assert lib.bmhrl_gemm_plan(C.byref(d), out) == -22, (epi, field)
    assert lib.bmhrl_gemm_plan(None, out) == -22


def test_group_plan(lib):
    from bmhrl_amd import _lib

    def gp(*ds):
        return lib.bmhrl_gemm_group_plan((_lib.GemmDesc * len(ds))(*ds), len(ds))
    reg = lambda **kw: desc(64, 300, 300, a_trans=1, b_trans=1, split=True, **kw)  # noqa: E731 (caption-side dW, K = B L)
    assert gp(reg()) == 0                                       # one problem: a plain launch
    assert gp(reg(), reg()) == 1
    assert gp(reg(), reg(), reg(), reg()) == 1
    assert gp(reg(), reg(), reg(), reg(), reg()) == 1           # four in one launch + a plain one
    assert gp(*[reg() for _ in range(8)]) == 2
    assert gp(reg(), desc(64, 300, 256, a_trans=1, b_trans=1)) == 0        # direct-to-LDS problem: one by one
    assert gp(reg(), desc(64, 300, 300, a_trans=1, b_trans=0)) == 0        # another operand layout
    assert gp(reg(), desc(4100, 1030, 300, a_trans=1, b_trans=1)) == 0     # 128 x 128 tiles
    ordered = desc(480, 364, 10172, b_trans=1, split=True, ws=11 * 480 * 364)
    assert gp(desc(480, 364, 10172, b_trans=1, split=True), desc(480, 364, 10172, b_trans=1, split=True)) == 1
    assert gp(desc(480, 364, 10172, b_trans=1, split=True), ordered) == 0  # the ordered split is a second pass
    assert gp(reg(), desc(64, 64, 64, dropout_p=1.0)) == -22


# ---- self-check of the GPU tests' error bound (tests/gemm_reference.py), in float64 on the CPU
K_MAX = 10176                      # the largest reduction of test_gemm_paths_gpu (the vocabulary head's d cat[x, goal])


def _bf16(x):
    import torch
    return torch.from_numpy(x).to(torch.bfloat16).double().numpy()


def test_bound_flags_one_wrong_product_term():
    """At the largest K, one product term of typical size missing or doubled must violate TAU * S, while fp32
    accumulation of the same products (emulated: blocks of 16, rounded after every addition) must satisfy it."""
    rng = np.random.default_rng(5)
    worst_ok = 0.0
    for trial in range(6):
        a = _bf16(rng.standard_normal(K_MAX))
        b = _bf16(rng.standard_normal(K_MAX))
        prod = a * b
        exact = float(np.sum(prod))                            # float64: exact to far below TAU for these operands
        S = float(np.sum(np.abs(prod)))
        bound = gr.TAU * S
        fp32 = float(gr.emulate_fp32_dot(a, b))
        assert abs(fp32 - exact) <= bound
        worst_ok = max(worst_ok, abs(fp32 - exact) / S)
        typical = float(np.median(np.abs(prod)))
        k = int(np.argmin(np.abs(np.abs(prod) - typical)))    # a term of typical (median) size
        assert abs((exact - prod[k]) - exact) > bound          # missing
        assert abs((exact + prod[k]) - exact) > bound          # doubled
    # the emulated fp32 error sits orders of magnitude inside the bound (the margin tests/gemm_reference.py states)
    assert worst_ok < gr.TAU / 16


def test_dropout_mirror_matches_the_header():
    """keep fraction near 1 - p, ids of the documented default layout, and the threshold / scale of csrc/common.h"""
    assert gr.dropout_threshold(0.25) == 1 << 30
    assert gr.dropout_threshold(0.0) == 0
    assert gr.dropout_scale(0.25) == float(np.float32(1) / np.float32(0.75))
    ids = gr.drop_ids(3, 5, 2, 3, (0, 0, 0))
    assert int(ids[1, 2, 2, 4]) == ((1 * 3 + 2) * 3 + 2) * 5 + 4
    ids = gr.drop_ids(3, 5, 2, 3, (1000, 100, 7))
    assert int(ids[1, 2, 2, 4]) == 1000 + 200 + 14 + 4
    keep = gr.keep_mask(0.3, 1234, 64, 256, 2, 2, (0, 0, 0))
    assert abs(float(keep.mean()) - 0.7) < 0.01
    # 64-bit seeds and ids: the high words enter the hash
    x = gr.dropout_bits(1, np.array([5], dtype=np.uint64))
    assert x[0] != gr.dropout_bits(1 + (1 << 32), np.array([5], dtype=np.uint64))[0]
    assert x[0] != gr.dropout_bits(1, np.array([5 + (1 << 32)], dtype=np.uint64))[0]
