"""The specialised fp32-output epilogue of bmhrl_gemm (gemm_epilogue's fast_f32 path) against the generic loop it stands in for.

Every combination the fast path instantiates -- plain, bias, accumulate, (bias +) residual, dropout + residual, the last with
a bf16 twin -- plus the combinations that fall back (relu, column sums, residual + accumulate, unaligned ldc, a mask, PROB,
DSCORE) runs in four fresh child processes, {default tiles, BMHRL_GEMM_TILE=2 (128 x 128)} x {default, BMHRL_GEMM_FAST_F32=0},
all under BMHRL_DETERMINISTIC=1 (the switches are read once per process).  Each child checks its outputs against the float64
reference and bounds of tests/test_gemm_paths_gpu.py (operands with NaN padding, sentinel-filled outputs, the keep mask of the
dropout mirror in tests/gemm_reference.py, which is the generic loop's) and saves them; the parent compares the two settings
of the switch bit for bit and what bmhrl_gemm_f32_fast_path reported.

Shapes: 256 x 256 x 128 has interior tiles only on either plan (direct-to-LDS loop); 130 x 132 x 80 has a ragged M and N edge and a
K tail (register-staged loop; on 64 x 64 tiles four of its nine tiles are interior, on 128 x 128 tiles one of four); a group of
two transposed 130 x 132 x 80 problems runs through gemm_group_kernel."""
import os
import subprocess
import sys

import pytest
import torch

from tests import test_gemm_paths_gpu as gp

pytestmark = pytest.mark.gpu

ROOT = gp.ROOT
P, D = gp.P, gp.D
SHAPES = {"int": (256, 256, 128), "rag": (130, 132, 80)}
# name -> (case keywords, served by the fast path)
VARIANTS = {
    "plain": (dict(), True),
    "bias": (dict(bias=True, alpha=0.5), True),
    "acc": (dict(accumulate=True), True),
    "res": (dict(bias=True, residual=True), True),
    "drop_res": (dict(bias=True, residual=True, p=0.1), True),
    "drop_res_twin": (dict(bias=True, residual=True, p=0.1, bf16=True, ldcb_pad=4), True),
    # combinations without an instance: the generic loop
    "relu": (dict(bias=True, relu=True), False),
    "drop": (dict(bias=True, p=0.1), False),
    "res_acc": (dict(bias=True, residual=True, accumulate=True), False),
    "res_twin": (dict(bias=True, residual=True, bf16=True), False),
    "colsum": (dict(colsum=True), False),
}
CASES, FAST = [], {}
for sname, (M, N, K) in SHAPES.items():
    for vname, (kw, fast) in VARIANTS.items():
        c = gp.case(f"f32_{sname}_{vname}", M, N, K, **kw)
        CASES.append(c)
        FAST[c["name"]] = fast
for c, fast in [
    (gp.case("f32_batched", 130, 132, 128, bt=True, batch=(1, 2), bias=True, per_head=True, residual=True, p=0.1, bf16=True,
             drop_strides=(100003, 20011, 307)), True),
    (gp.case("f32_batched_acc", 64, 192, 64, at=True, batch=(1, 2), accumulate=True), True),
    (gp.case("f32_unaligned_ldc", 256, 256, 128, ldc_pad=1, bias=True, residual=True, p=0.1), False),
    (gp.case("f32_offset_c", 256, 256, 128, c_off=1, accumulate=True), False),
    (gp.case("f32_masked", 256, 256, 128, bias=True, residual=True, mask="mn", p=0.1), False),
    (gp.case("f32_keymask", 130, 132, 80, bias=True, mask="key"), False),
    (gp.case("f32_prob", 130, 132, 128, bt=True, epi=P, bf16=True, mask="key", alpha=0.0625), False),
    (gp.case("f32_dscore", 130, 132, 128, epi=D, bf16=True, mask="key", alpha=0.0625), False),
]:
    CASES.append(c)
    FAST[c["name"]] = fast
GROUP = [gp.case(f"f32_group_{i}", 130, 132, 80, at=True, bt=True, **kw)
         for i, kw in enumerate((dict(accumulate=True), dict(bias=True, residual=True, p=0.1)))]
NAMES = [c["name"] for c in CASES] + [c["name"] for c in GROUP]
for c in GROUP:
    FAST[c["name"]] = True
SETTINGS = {"t64_fast": {}, "t64_generic": dict(BMHRL_GEMM_FAST_F32="0"),
            "t128_fast": dict(BMHRL_GEMM_TILE="2"), "t128_generic": dict(BMHRL_GEMM_TILE="2", BMHRL_GEMM_FAST_F32="0")}


def child(setting, out_path):
    """run every case under the environment the parent started this process with; per case: the plan, the fast-path query,
    the reference check's verdict and the output buffers"""
    import ctypes as C
    from bmhrl_amd import _lib, ops
    for k, v in SETTINGS[setting].items():
        assert os.environ.get(k) == v, f"child {setting} started without {k}={v}"
    lib = _lib.load()
    assert lib.bmhrl_deterministic_enabled()
    dev = torch.device("cuda:0")
    out = {}

    def record(x, d):
        c = x["case"]
        r = dict(plan=ops.gemm_plan(d), fast=ops.gemm_f32_fast_path(d), error=None)
        try:
            gp.check(x, det=True)
        except AssertionError as e:
            r["error"] = str(e)
        r["bufs"] = {k: x[k].cpu() for k in ("Cbuf", "Cbbuf", "csbuf") if k in x}
        out[c["name"]] = r

    for c in CASES:
        x = gp.make(c, dev)
        d = gp.descriptor(x)
        _lib.check(lib.bmhrl_gemm(C.byref(d), ops.stream()), "bmhrl_gemm")
        torch.cuda.synchronize()
        record(x, d)
    xs = [gp.make(c, dev) for c in GROUP]
    ds = [gp.descriptor(x) for x in xs]
    # one gemm_group_kernel launch on the default plan (forced 128 x 128 tiles run one by one)
    assert ops.gemm_group_plan(ds) == (0 if "BMHRL_GEMM_TILE" in SETTINGS[setting] else 1)
    _lib.check(lib.bmhrl_gemm_group((_lib.GemmDesc * len(ds))(*ds), len(ds), ops.stream()), "bmhrl_gemm_group")
    torch.cuda.synchronize()
    for x, d in zip(xs, ds):
        record(x, d)
    torch.save(out, out_path)


_CHILD = "import sys; sys.path.insert(0, sys.argv[1]); from tests.test_gemm_f32_epilogue_gpu import child; child(sys.argv[2], sys.argv[3])"


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    tmp = tmp_path_factory.mktemp("f32_epilogue")
    base = {k: v for k, v in os.environ.items() if not (k.startswith("BMHRL_GEMM_") or k == "BMHRL_DETERMINISTIC")}
    base["BMHRL_DETERMINISTIC"] = "1"
    procs = {}
    for s, env_add in SETTINGS.items():                       # (four processes side by side: each is mostly start-up)
        procs[s] = subprocess.Popen([sys.executable, "-c", _CHILD, ROOT, s, str(tmp / f"{s}.pt")], env={**base, **env_add}, cwd=ROOT,
                                    stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    res = {}
    for s, pr in procs.items():
        text, _ = pr.communicate(timeout=300)
        assert pr.returncode == 0, f"child {s} exited {pr.returncode}:\n{text[-4000:]}"
        res[s] = torch.load(tmp / f"{s}.pt")
    return res


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("name", NAMES)
def test_against_float64_reference(results, setting, name):
    """(a) the bounds of tests/test_gemm_paths_gpu.py, on both plans, with the fast path and without"""
    r = results[setting][name]
    assert r["plan"]["tile"] == (1 if setting.startswith("t128") else 0), r["plan"]
    assert r["error"] is None, r["error"]


@pytest.mark.parametrize("tile", ["t64", "t128"])
@pytest.mark.parametrize("name", NAMES)
def test_fast_and_generic_paths_agree_bit_for_bit(results, tile, name):
    """(b) C, the bf16 twin and the column sums, whole buffers (padding and gaps included), under BMHRL_DETERMINISTIC=1"""
    a, b = results[f"{tile}_fast"][name], results[f"{tile}_generic"][name]
    assert sorted(a["bufs"]) == sorted(b["bufs"]) and "Cbuf" in a["bufs"]
    for k in a["bufs"]:
        ta, tb = a["bufs"][k], b["bufs"][k]
        assert torch.equal(ta, tb), f"{name} {k}: {int((ta != tb).sum())} of {ta.numel()} elements differ"
        bits = torch.int16 if ta.dtype == torch.bfloat16 else torch.int32
        assert torch.equal(ta.view(bits), tb.view(bits)), f"{name} {k}: equal values, different bits (signed zeros)"


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_fast_path_query(results, setting):
    """(c) bmhrl_gemm_f32_fast_path: the instantiated combinations with aligned operands, and only with the switch on;
    bmhrl_gemm_plan keeps naming the store path the edge tiles take"""
    on = setting.endswith("_fast")
    for name in NAMES:
        r = results[setting][name]
        assert r["fast"] == (on and FAST[name]), (setting, name, r)
        if FAST[name]:
            assert r["plan"]["epi_path"] == 2 and r["plan"]["vec_ok"] == 1 and r["plan"]["splits"] == 1, (name, r["plan"])
    assert results[setting]["f32_unaligned_ldc"]["plan"]["vec_ok"] == 0
    assert results[setting]["f32_prob"]["plan"]["epi_path"] == 2 and results[setting]["f32_dscore"]["plan"]["epi_path"] == 2
