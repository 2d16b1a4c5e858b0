"""The row kernels of csrc/elementwise.hip and csrc/conv_gn.hip, path by path, against the float64 formulas of
tests/row_reference.py (which tests/test_row_reference_cpu.py proves against torch): the scalar LayerNorm kernels (every
ln_bwd_kernel<NC>), the edges of the LayerNorm backward plan, null outputs, GroupNorm / unfold / fold at the real width and at
the widths that take another branch, and the ordered forms behind BMHRL_DETERMINISTIC=1 -- that switch is read once per
process, so those run in one child process.  Every case asserts the path it is meant to reach (D % 4, alignment, the block
count of the plan), so a retuning cannot silently empty it.  Figures are printed before they are asserted (pytest -s)."""
import functools
import math
import os
import subprocess
import sys

import pytest
import torch

from tests import row_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -512.0                  # sentinel (exact in bf16 too)
ATOMIC_MAX = 128               # bmhrl_layernorm_bwd_ws: up to this many blocks add with atomics, more go through the workspace


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bmhrl_amd import _lib, ops
    _lib.load()  # must exist: the product has no fallback
    assert not ops.deterministic(), "the default-mode paths are tested here; the ordered ones run in a child process"
    return torch.device("cuda:0")


def _refused(fn, *a, **k):
    from bmhrl_amd import _lib
    with pytest.raises(_lib.HipError, match="invalid argument -22"):
        fn(*a, **k)


# ------------------------------------------------------------------------------------------------ LayerNorm
@functools.lru_cache(maxsize=None)
def _ln_case(rows, D, G=1):
    """inputs as test_layernorm builds them (fp32, CPU; G groups stacked) and their float64 results, computed once"""
    g = torch.Generator().manual_seed(rows + D + 1000 * (G - 1))
    x = torch.randn(G * rows, D, generator=g) * 2 + 0.5
    gamma = 1 + 0.1 * torch.randn(G, D, generator=g)
    beta = 0.1 * torch.randn(G, D, generator=g)
    dy = torch.randn(G * rows, D, generator=g)
    add = torch.randn(G * rows, D, generator=g)
    ref = dict(y=[], mean=[], rstd=[], dx=[], dx0=[], dg=[], db=[])
    for i in range(G):
        sl = slice(i * rows, (i + 1) * rows)
        y, mean, rstd = R.layernorm_fwd(x[sl].double(), gamma[i].double(), beta[i].double())
        dx, dg, db = R.layernorm_bwd(dy[sl].double(), x[sl].double(), gamma[i].double(), add[sl].double())
        dx0, _, _ = R.layernorm_bwd(dy[sl].double(), x[sl].double(), gamma[i].double())
        for k, v in dict(y=y, mean=mean, rstd=rstd, dx=dx, dx0=dx0, dg=dg, db=db).items():
            ref[k].append(v)
    ref = {k: torch.stack(v) if k in ("dg", "db") else torch.cat(v) for k, v in ref.items()}
    return dict(rows=rows, D=D, G=G, x=x, gamma=gamma, beta=beta, dy=dy, add=add, **{"r_" + k: v for k, v in ref.items()})


def _put(dev, t, off=0):
    """t on the device, as a view that starts `off` floats into a larger buffer (off = 1: no 16-byte alignment)"""
    buf = torch.full((t.numel() + 4,), float("nan"), device=dev)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * off and v.is_contiguous()
    return v


def _ln_fwd(dev, c, off=0, want_yb=True, want_yf=True, ldy=None):
    """-> yb (rows, ldy) sentinel-filled buffer or None, yf or None, mean, rstd"""
    from bmhrl_amd import ops
    rows, D, G = c["rows"] * c["G"], c["D"], c["G"]
    ldy = ldy or ops.pad8(D)
    x, gamma, beta = _put(dev, c["x"], off), c["gamma"].to(dev), c["beta"].to(dev)
    yb = torch.full((rows, ldy), SENT, dtype=torch.bfloat16, device=dev) if want_yb else None
    yf = _put(dev, torch.full((rows, D), SENT), off) if want_yf else None
    mean, rstd = torch.full((rows,), SENT, device=dev), torch.full((rows,), SENT, device=dev)
    if G == 1:
        ops.layernorm_fwd(x, gamma, beta, yb, ldy, yf, mean, rstd, rows, D)
    else:
        ops.layernorm_fwd_groups(x, gamma, beta, yb, ldy, yf, mean, rstd, c["rows"], D, G)
    return yb, yf, mean, rstd


def _check_ln_fwd(what, c, yb, yf, mean, rstd):
    """test_layernorm's bounds: fp32 1e-5, bf16 twin 1e-2, mean / rstd 1e-5; the padding columns of yb keep the sentinel"""
    D = c["D"]
    e = dict(mean=R.rel_err(mean, c["r_mean"]), rstd=R.rel_err(rstd, c["r_rstd"]))
    if yf is not None:
        e["y_f32"] = R.rel_err(yf, c["r_y"])
    if yb is not None:
        e["y_bf16"] = R.rel_err(yb[:, :D].float(), c["r_y"])
    print(f"{what}: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    for k, v in e.items():
        assert v < (1e-2 if k == "y_bf16" else 1e-5), (what, k, v)
    if yb is not None and yb.shape[1] > D:
        assert bool((yb[:, D:] == SENT).all()), f"{what}: padding columns of y_bf16 written"
    return e


def _ln_bwd(dev, c, mean, rstd, off=0, want_dg=True, want_db=True, with_add=True, workspace=None):
    """-> dx, pg: dgamma | dbeta halves of ONE (2, G, D) buffer; a half that is not asked for is passed as null and keeps SENT"""
    from bmhrl_amd import ops
    rows, D, G = c["rows"] * c["G"], c["D"], c["G"]
    x, dy, gamma = _put(dev, c["x"], off), _put(dev, c["dy"], off), c["gamma"].to(dev)
    add = _put(dev, c["add"], off) if with_add else None
    dx = _put(dev, torch.full((rows, D), SENT), off)
    pg = torch.full((2, G, D), SENT, device=dev)
    if want_dg:
        pg[0].zero_()
    if want_db:
        pg[1].zero_()
    dg, db = (pg[0] if want_dg else None), (pg[1] if want_db else None)
    if G == 1:
        ops.layernorm_bwd(dy, x, gamma, mean, rstd, dx, add, dg, db, rows, D, workspace=workspace)
    else:
        ops.layernorm_bwd_groups(dy, x, gamma, mean, rstd, dx, add, dg, db, c["rows"], D, G)
    return dx, pg


def _check_ln_bwd(what, c, dx, pg, want_dg=True, want_db=True, with_add=True):
    """test_layernorm's bound, 2e-5, on dx / dgamma / dbeta; a gradient that was not asked for is not written"""
    e = dict(dx=R.rel_err(dx, c["r_dx"] if with_add else c["r_dx0"]))
    if want_dg:
        e["dgamma"] = R.rel_err(pg[0], c["r_dg"])
    if want_db:
        e["dbeta"] = R.rel_err(pg[1], c["r_db"])
    print(f"{what}: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    for k, v in e.items():
        assert v < 2e-5, (what, k, v)
    if not want_dg:
        assert bool((pg[0] == SENT).all()), f"{what}: dgamma's neighbour written"
    if not want_db:
        assert bool((pg[1] == SENT).all()), f"{what}: dbeta's neighbour written"
    return e


def _blocks(rows, D):
    """blocks of the workspace plan of bmhrl_layernorm_bwd_ws, from the size it asks for"""
    from bmhrl_amd import ops
    ws = ops.layernorm_bwd_workspace(rows, D)
    assert ws % (2 * D) == 0
    return ws // (2 * D)


def _rows_per_wave(rows, blocks):
    """the rows_per_wave behind a block count: blocks = ceil(ceil(rows / rv) / 4) (4 waves per block); None if ambiguous"""
    fits = [rv for rv in range(1, 33) if (-(-rows // rv) + 3) // 4 == blocks]
    return fits[0] if len(fits) == 1 else None


NC_OF = {37: 1, 70: 2, 301: 5, 322: 8, 514: 16, 1022: 16}      # D -> the ln_bwd_kernel<NC> instantiation it launches


def _nc(D):
    nc = -(-D // 64)
    return next(n for n in (1, 2, 5, 8, 16) if nc <= n)


@pytest.mark.parametrize("rows,D", [(37, 37), (37, 70), (37, 301), (37, 322), (37, 514), (37, 1022), (2100, 301)])
def test_layernorm_scalar_kernels(dev, rows, D):
    """D % 4 != 0: ln_fwd_kernel and ln_bwd_kernel<NC>, one case per NC; 1022 = the last column of NC 16; (2100, 301): two rows
    per wave and 263 blocks of atomics"""
    assert D % 4 != 0 and D <= 1024 and _nc(D) == NC_OF[D]
    if rows == 2100:        # ln_bwd_direct: rows_per_wave = ceil(rows / 2048), 4 waves per block
        rpw = -(-rows // 2048)
        assert rpw == 2 and (-(-rows // rpw) + 3) // 4 == 263
    c = _ln_case(rows, D)
    yb, yf, mean, rstd = _ln_fwd(dev, c)
    _check_ln_fwd(f"ln_fwd_kernel ({rows}, {D})", c, yb, yf, mean, rstd)
    dx, pg = _ln_bwd(dev, c, mean, rstd)
    _check_ln_bwd(f"ln_bwd_kernel<{_nc(D)}> ({rows}, {D})", c, dx, pg)


def test_layernorm_misaligned_base_takes_the_scalar_kernels(dev):
    """x, dy, dx, dx_add, y_f32 one float into a larger buffer: every pointer the vector kernels read or write 16 bytes at a time
    is in the host's alignment test (x | gamma | beta | y_f32 and y_bf16 forward; dy | x | gamma | dx | dx_add backward), so the
    call falls back to the scalar kernels.  Against float64, and against the aligned (vector) result of the same values: those two
    differ in summation order only"""
    c = _ln_case(37, 300)
    assert c["D"] % 4 == 0                                   # only the alignment keeps the vector kernels away
    yb, yf, mean, rstd = _ln_fwd(dev, c, off=1)
    assert yf.data_ptr() % 16 == 4
    _check_ln_fwd("misaligned fwd (37, 300)", c, yb, yf, mean, rstd)
    dx, pg = _ln_bwd(dev, c, mean, rstd, off=1)
    assert dx.data_ptr() % 16 == 4
    _check_ln_bwd("misaligned bwd (37, 300)", c, dx, pg)
    yb_a, yf_a, mean_a, rstd_a = _ln_fwd(dev, c)
    dx_a, pg_a = _ln_bwd(dev, c, mean_a, rstd_a)
    assert torch.equal(yb, yb_a) or R.rel_err(yb.float(), yb_a.float()) < 1e-2     # (bf16 twin: a last-bit flip of the fp32 value)
    e = dict(y_f32=R.rel_err(yf, yf_a), mean=R.rel_err(mean, mean_a), rstd=R.rel_err(rstd, rstd_a), dx=R.rel_err(dx, dx_a),
             dgamma=R.rel_err(pg[0], pg_a[0]), dbeta=R.rel_err(pg[1], pg_a[1]))
    print("misaligned vs aligned (37, 300): " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    for k, v in e.items():
        assert v < 2e-6, (k, v)


@pytest.mark.parametrize("D", [1028, 2052])
def test_layernorm_forward_wider_than_1024(dev, D):
    """the forward accepts D > 1024 (scalar kernel, D % 4 == 0 or not); the backward refuses it"""
    from bmhrl_amd import ops
    c = _ln_case(5, D)
    assert D > 1024
    yb, yf, mean, rstd = _ln_fwd(dev, c)
    _check_ln_fwd(f"ln_fwd_kernel (5, {D})", c, yb, yf, mean, rstd)
    if D == 1028:
        x, dy, dx = c["x"].to(dev), c["dy"].to(dev), torch.full((5, D), SENT, device=dev)
        dg, db = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
        _refused(ops.layernorm_bwd, dy, x, c["gamma"].to(dev), mean, rstd, dx, None, dg, db, 5, D)
        _refused(ops.layernorm_bwd, dy, x, c["gamma"].to(dev), mean, rstd, dx, None, dg, db, 5, D, workspace=torch.empty(0))
        torch.cuda.synchronize()
        assert bool((dx == SENT).all()) and float(dg.abs().max()) == 0.0 and float(db.abs().max()) == 0.0


# (rows, D, blocks, rows per wave, partial sums through the workspace?, what)
PLAN_EDGES = [(512, 1024, 128, 1, False, "ln_bwd_vec_kernel<4, false>: the last block count that adds with atomics"),
              (516, 1024, 129, 1, True, "ln_bwd_vec_kernel<4, true> + reduce: the first block count through the workspace"),
              (2050, 1024, 171, 3, True, "ln_bwd_vec_kernel<4, true>: 3 rows per wave (a pair, then a single), last wave 1 row"),
              (2100, 300, 525, 1, True, "ln_bwd_vec_kernel<2, true> + reduce")]


@pytest.mark.parametrize("rows,D,blocks,rv,part,what", PLAN_EDGES, ids=[f"{e[0]}x{e[1]}" for e in PLAN_EDGES])
def test_layernorm_bwd_plan_edges(dev, rows, D, blocks, rv, part, what):
    assert D % 4 == 0 and _blocks(rows, D) == blocks and _rows_per_wave(rows, blocks) == rv and (blocks > ATOMIC_MAX) == part
    if rv == 3:
        assert rows % rv == 1                                    # the last wave walks one row
    c = _ln_case(rows, D)
    _, _, mean, rstd = _ln_fwd(dev, c, want_yb=False)
    dx, pg = _ln_bwd(dev, c, mean, rstd)
    _check_ln_bwd(f"{what} ({rows}, {D})", c, dx, pg)


def test_layernorm_bwd_without_a_workspace_takes_the_direct_vector_path(dev):
    """workspace of 0 floats: ln_bwd_direct, ln_bwd_vec_kernel<4, false> at ceil(2050 / 1024) = 3 rows per wave (what
    bmhrl_layernorm_bwd_groups falls back to)"""
    rows, D = 2050, 1024
    assert D % 4 == 0 and -(-rows // 1024) == 3 and rows % 3 == 1
    c = _ln_case(rows, D)
    _, _, mean, rstd = _ln_fwd(dev, c, want_yb=False)
    empty = torch.empty(0)
    assert empty.numel() < _blocks(rows, D) * 2 * D
    dx, pg = _ln_bwd(dev, c, mean, rstd, workspace=empty)
    _check_ln_bwd(f"direct ln_bwd_vec_kernel<4, false> ({rows}, {D})", c, dx, pg)


@pytest.mark.parametrize("rows,D,path", [(37, 300, "atomic"), (516, 1024, "part"), (37, 301, "scalar")])
@pytest.mark.parametrize("want_dg,want_db,with_add", [(True, False, True), (False, True, True), (False, False, True), (True, True, False)])
def test_layernorm_bwd_optional_pointers(dev, rows, D, path, want_dg, want_db, with_add):
    """null dgamma / dbeta / dx_add: what is asked for is right, a sentinel-filled neighbour of it is unchanged"""
    if path == "scalar":
        assert D % 4 != 0
    else:
        assert D % 4 == 0 and (_blocks(rows, D) > ATOMIC_MAX) == (path == "part")
    c = _ln_case(rows, D)
    _, _, mean, rstd = _ln_fwd(dev, c, want_yb=False)
    dx, pg = _ln_bwd(dev, c, mean, rstd, want_dg=want_dg, want_db=want_db, with_add=with_add)
    _check_ln_bwd(f"{path} ({rows}, {D}) dgamma {want_dg} dbeta {want_db} dx_add {with_add}", c, dx, pg, want_dg, want_db, with_add)


@pytest.mark.parametrize("rows,D,kernel", [(37, 300, "ln_fwd_vec_kernel<2, 1>"), (37, 128, "ln_fwd_vec_kernel<1, 2>"), (37, 301, "ln_fwd_kernel")])
@pytest.mark.parametrize("want_yb,want_yf", [(True, False), (False, True), (True, True)])
def test_layernorm_fwd_outputs(dev, rows, D, kernel, want_yb, want_yf):
    """only y_bf16, only y_f32, both; y_bf16 rows of pad8(D) + 8 columns: the columns >= D keep their sentinel"""
    from bmhrl_amd import ops
    assert (D % 4 == 0) == ("vec" in kernel)
    c = _ln_case(rows, D)
    ldy = ops.pad8(D) + 8
    assert ldy % 4 == 0 and ldy - D >= 8
    yb, yf, mean, rstd = _ln_fwd(dev, c, want_yb=want_yb, want_yf=want_yf, ldy=ldy)
    _check_ln_fwd(f"{kernel} ({rows}, {D}) y_bf16 {want_yb} y_f32 {want_yf}", c, yb, yf, mean, rstd)


@pytest.mark.parametrize("rows,D", [(37, 128), (37, 301)])
def test_layernorm_groups_against_float64(dev, rows, D):
    """two groups in one call, each against ITS float64 result: (37, 128) loops over the groups in the forward (D <= 128) and
    takes the grouped vector launch in the backward; (37, 301) loops over the scalar kernels in both"""
    c = _ln_case(rows, D, G=2)
    if D % 4 == 0:
        assert _blocks(rows, D) <= ATOMIC_MAX                # the one-launch grouped backward
    yb, yf, mean, rstd = _ln_fwd(dev, c)
    _check_ln_fwd(f"groups fwd 2 x ({rows}, {D})", c, yb, yf, mean, rstd)
    dx, pg = _ln_bwd(dev, c, mean, rstd)
    _check_ln_bwd(f"groups bwd 2 x ({rows}, {D})", c, dx, pg)


# ------------------------------------------------------------------------------------------------ GroupNorm
GN_CASES = [(2, 5, 1024, 32, "fixed", "cpg 32: the real width, a group smaller than the block"),
            (2, 40, 1024, 32, "fixed", "cpg 32: the real width"),
            (3, 7, 96, 32, "atomic", "cpg 3"),
            (2, 3, 40, 8, "atomic", "cpg 5"),
            (1, 1, 64, 32, "fixed", "cpg 2: T = 1"),
            (2, 9, 512, 2, "fixed", "cpg 256: the limit, every thread reduces"),
            (2, 4, 1024, 2, "refused", "cpg 512: forward only, the backward is refused")]


def _gn_branch(C, G):
    """what groupnorm_bwd does with C / G channels per group: its dgamma / dbeta terms stay in registers (`fixed`: a thread
    always meets the same channel), go through atomics element by element, or the call is refused"""
    cpg = C // G
    return "refused" if cpg > 256 else ("fixed" if 256 % cpg == 0 else "atomic")


@functools.lru_cache(maxsize=None)
def _gn_case(B, T, C, G):
    """inputs (fp32), the float64 results, and E: the relative error of the SAME formulas evaluated in float32 on the CPU"""
    g = torch.Generator().manual_seed(B * 1000 + T * 100 + C + G)
    x = torch.randn(B, T, C, generator=g) * 1.5 + 0.3
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.1
    dy = torch.randn(B, T, C, generator=g)
    names = ("y", "mean", "rstd", "dx", "dgamma", "dbeta")
    r64 = dict(zip(names, R.groupnorm_fwd(x.double(), gamma.double(), beta.double(), G) + R.groupnorm_bwd(dy.double(), x.double(), gamma.double(), G)))
    r32 = dict(zip(names, R.groupnorm_fwd(x, gamma, beta, G) + R.groupnorm_bwd(dy, x, gamma, G)))
    assert all(v.dtype == torch.float32 for v in r32.values()) and all(v.dtype == torch.float64 for v in r64.values())
    E = {k: R.rel_err(r32[k], r64[k]) for k in ("mean", "rstd", "dx")}
    assert all(0.0 < e < 1e-5 for e in E.values()), f"yardstick E = {E}: the float32 evaluation disagrees with the float64 one"
    return dict(x=x, gamma=gamma, beta=beta, dy=dy, r=r64, E=E)


def _guarded(dev, shape):
    """a sentinel-filled tensor with 64 sentinel floats before and after it -> (tensor, whole buffer)"""
    n = math.prod(shape)
    buf = torch.full((n + 128,), SENT, device=dev)
    return buf[64:64 + n].view(shape), buf


def _guards_intact(buf):
    return bool((buf[:64] == SENT).all()) and bool((buf[-64:] == SENT).all())


@pytest.mark.parametrize("B,T,C,G,branch,what", GN_CASES, ids=["-".join(map(str, e[:5])) for e in GN_CASES])
def test_groupnorm_paths(dev, B, T, C, G, branch, what):
    """forward < 2e-5 and dgamma / dbeta < 1e-4 (the bounds of test_conv1d_same_and_groupnorm_gradients); mean, rstd and dx
    within 8 E of the float64 result, E the error of the same formulas in float32 (8 = the margin tests/test_critic_train_gpu.py
    gives a different summation order)"""
    from bmhrl_amd import ops
    assert _gn_branch(C, G) == branch
    c = _gn_case(B, T, C, G)
    r, E = c["r"], c["E"]
    x, gamma, beta, dy = (c[k].to(dev) for k in ("x", "gamma", "beta", "dy"))
    (y, ybuf), (mean, mbuf), (rstd, rbuf) = _guarded(dev, (B, T, C)), _guarded(dev, (B, G)), _guarded(dev, (B, G))
    ops.groupnorm_fwd(x, gamma, beta, y, mean, rstd, B, T, C, G, 1e-5)
    e = dict(y=R.rel_err(y, r["y"]), mean=R.rel_err(mean, r["mean"]), rstd=R.rel_err(rstd, r["rstd"]))
    (dx, dxbuf), (dg, dgbuf), (db, dbbuf) = _guarded(dev, (B, T, C)), _guarded(dev, (C,)), _guarded(dev, (C,))
    dg.zero_(); db.zero_()
    if branch == "refused":
        _refused(ops.groupnorm_bwd, dy, x, gamma, mean, rstd, dx, dg, db, B, T, C, G)
        torch.cuda.synchronize()
        assert bool((dx == SENT).all()) and float(dg.abs().max()) == 0.0 and float(db.abs().max()) == 0.0
    else:
        ops.groupnorm_bwd(dy, x, gamma, mean, rstd, dx, dg, db, B, T, C, G)
        e.update(dx=R.rel_err(dx, r["dx"]), dgamma=R.rel_err(dg, r["dgamma"]), dbeta=R.rel_err(db, r["dbeta"]))
    print(f"groupnorm ({B}, {T}, {C}, {G}) {branch}, {what}: " + ", ".join(
        f"{k} {v:.2e}" + (f" = {v / E[k]:.2f} E (E {E[k]:.2e})" if k in E else "") for k, v in e.items()))
    assert e["y"] < 2e-5
    for k in ("mean", "rstd", "dx"):
        if k in e:
            assert e[k] <= 8 * E[k], f"{k}: err {e[k]:.3e} > 8 E = {8 * E[k]:.3e}"
    for k in ("dgamma", "dbeta"):
        if k in e:
            assert e[k] < 1e-4, (k, e[k])
    assert all(_guards_intact(b) for b in (ybuf, mbuf, rbuf, dxbuf, dgbuf, dbbuf))


@pytest.mark.parametrize("B,T,C,G", [(2, 5, 1024, 32), (3, 7, 96, 32)])
def test_groupnorm_bwd_without_parameter_gradients(dev, B, T, C, G):
    """dgamma = dbeta = null, on the register-resident branch and on the atomic one: dx right, nothing else written"""
    from bmhrl_amd import ops
    assert _gn_branch(C, G) == ("fixed" if C == 1024 else "atomic")
    c = _gn_case(B, T, C, G)
    x, gamma, dy = (c[k].to(dev) for k in ("x", "gamma", "dy"))
    mean, rstd = c["r"]["mean"].float().to(dev), c["r"]["rstd"].float().to(dev)
    inputs = [t.clone() for t in (x, gamma, dy, mean, rstd)]
    dx, dxbuf = _guarded(dev, (B, T, C))
    ops.groupnorm_bwd(dy, x, gamma, mean, rstd, dx, None, None, B, T, C, G)
    err = R.rel_err(dx, c["r"]["dx"])
    print(f"groupnorm_bwd ({B}, {T}, {C}, {G}) without dgamma / dbeta: dx {err:.2e} = {err / c['E']['dx']:.2f} E")
    assert err <= 8 * c["E"]["dx"]
    assert _guards_intact(dxbuf) and all(torch.equal(a, b) for a, b in zip(inputs, (x, gamma, dy, mean, rstd)))


# ------------------------------------------------------------------------------------------------ unfold / fold
@pytest.mark.parametrize("k", [1, 3, 6, 9])
@pytest.mark.parametrize("T", [1, 4, 17])
def test_unfold1d_operand(dev, k, T):
    """the bf16 operand of Conv1d 'same' (left = (k - 1) // 2, kernels longer than the clip included), rows of k * C and of
    k * C + 8 columns: equal to the bf16 cast of the reference operand, padding columns untouched"""
    from bmhrl_amd import ops
    B = 2
    for C in (4, 64):
        x = torch.randn(B, T, C, generator=torch.Generator().manual_seed(100 * k + 10 * T + C))
        want = R.unfold1d(x.double(), k).to(torch.bfloat16)
        for ldo in (k * C, k * C + 8):
            out = torch.full((B * T, ldo), SENT, dtype=torch.bfloat16, device=dev)
            ops.unfold1d_bf16(x.to(dev), out, ldo, B, T, C, k, R.same_left(k))
            assert torch.equal(out[:, :k * C].cpu(), want), (k, T, C, ldo)
            assert bool((out[:, k * C:] == SENT).all()), (k, T, C, ldo)


@pytest.mark.parametrize("k", [1, 3, 6, 9])
@pytest.mark.parametrize("T", [1, 4, 17])
def test_fold1d_gradient(dev, k, T):
    """the fold adds the k terms of an element in fp32, in order: |err| <= k 2^-24 sum|terms| per element against float64 (each
    of the at most k roundings is half an ulp, 2^-24 relative, of a partial sum no larger than sum|terms|).  The padding columns of
    du hold NaN: reading one shows"""
    from bmhrl_amd import ops
    B = 2
    for C in (4, 64):
        du = torch.randn(B * T, k * C, generator=torch.Generator().manual_seed(100 * k + 10 * T + C + 1))
        terms = R.fold1d_terms(du.double(), B, T, C, k)
        want, bound = terms.sum(0), k * 2.0 ** -24 * terms.abs().sum(0)
        for ldu in (k * C, k * C + 8):
            buf = torch.full((B * T, ldu), float("nan"), device=dev)
            buf[:, :k * C] = du.to(dev)
            dx, dxbuf = _guarded(dev, (B, T, C))
            ops.fold1d(buf, ldu, dx, B, T, C, k, R.same_left(k))
            err = (dx.cpu().double() - want).abs()
            assert bool(torch.isfinite(dx).all()) and bool((err <= bound).all()), (k, T, C, ldu, float((err - bound).max()))
            assert _guards_intact(dxbuf)


# ------------------------------------------------------------------------------------------------ ordered forms (child process)
def _twice(run):
    """run() -> tuple of fresh output tensors; two runs must be bit-identical; -> the first"""
    a, b = run(), run()
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(a, b)), "two ordered runs differ"
    return a


def child():
    """BMHRL_DETERMINISTIC=1 (the parent started this process with it): every ordered form twice from fresh outputs, bit-identical,
    and the first run against float64 within the bound the default-mode test of the same entry point uses"""
    from bmhrl_amd import _lib, ops
    assert os.environ.get("BMHRL_DETERMINISTIC") == "1"
    assert _lib.load().bmhrl_deterministic_enabled() == 1 and ops.deterministic()
    dev = torch.device("cuda:0")

    # -- LayerNorm backward: PART + one-block-per-column reduce; the one-block scalar kernel; the same without a workspace
    for rows, D, G, ws, what in [(1001, 128, 1, None, "PART, ordered reduce"), (37, 301, 1, None, "one-block scalar"),
                                 (600, 300, 1, torch.empty(0), "no workspace: one block, 150 rows per wave"),
                                 (37, 128, 2, None, "groups: the per-group loop of ops.layernorm_bwd_groups")]:
        c = _ln_case(rows, D, G)
        if "PART" in what or G == 2:
            assert D % 4 == 0 and _blocks(rows, D) >= 1          # vector form; deterministic: always through the workspace
        if "scalar" in what:
            assert D % 4 != 0
        if ws is not None:
            assert ws.numel() == 0 and (rows + 3) // 4 == 150
        _, _, mean, rstd = _ln_fwd(dev, c, want_yb=False)
        dx, pg = _twice(lambda: _ln_bwd(dev, c, mean, rstd, workspace=ws))
        _check_ln_bwd(f"ordered layernorm_bwd {G} x ({rows}, {D}) {what}", c, dx, pg)

    # -- embedding gradient: tokens repeat (V 5 < B * S 33); with the tok2 mix and without
    B, S, V = 3, 11, 5
    for D in (20, 70):
        g = torch.Generator().manual_seed(D)
        tok, tok2 = torch.randint(0, V, (B, S), generator=g), torch.randint(0, V, (B, S), generator=g)
        assert tok.unique().numel() < B * S and not torch.equal(tok, tok2)
        dC, sc = torch.randn(B, S, D, generator=g), math.sqrt(D)
        for t2 in (tok2, None):
            def run():
                dt = torch.zeros(V, D, device=dev)
                ops.embed_bwd(tok.to(dev), None if t2 is None else t2.to(dev), 0.25, dC.to(dev), dt, B, S, D, sc)
                return (dt,)
            (dt,) = _twice(run)
            want = R.embed_bwd(tok.reshape(-1), None if t2 is None else t2.reshape(-1), 0.25, dC.reshape(-1, D).double(), V, sc)
            err = R.rel_err(dt, want)
            print(f"ordered embed_bwd D {D} tok2 {t2 is not None}: {err:.2e}")
            assert err < 1e-5

    # -- scatter-add along a row map: the map of test_expand_goals_backward_is_ordered into a ZEROED dx, and a general map
    B, L = 7, 30
    for D in (64, 70):
        g = torch.Generator().manual_seed(2)
        seg = (torch.rand(B, L, generator=g) < 0.25).to(torch.int32)
        seg[3] = 0
        src_eg = torch.empty(B * L, dtype=torch.int32, device=dev)
        ops.expand_goals_index(seg.to(dev), src_eg, B, L)
        dout = torch.randn(B * L, D, generator=g)
        for what, src in (("expand_goals map", src_eg.cpu()), ("general map", R.general_row_map(B * L, g))):
            assert int(src.min()) >= -1 and int(src.max()) < B * L
            if what == "general map":
                kept = src[src >= 0]
                assert int((src < 0).sum()) > 0 and kept.unique().numel() < kept.numel()
            def run():
                dx = torch.zeros(B * L, D, device=dev)
                ops.scatter_add_rows(dout.to(dev), src.to(dev), dx, B * L, D)
                return (dx,)
            (dx,) = _twice(run)
            err = float((dx.cpu().double() - R.scatter_add_rows(dout.double(), src, B * L)).abs().max())
            print(f"ordered scatter_add_rows D {D} {what}: {err:.2e}")
            assert err < 1e-5

    # -- gate backward in one block: inside the clamp, on its closed end, outside it
    for rows, D in ((96, 20), (300, 300)):
        g = torch.Generator().manual_seed(rows)
        cv, ca, dout = (torch.randn(rows, D, generator=g) for _ in range(3))
        for a0 in (0.3, 2.0, -2.5):
            def run():
                dcv, dca, da = torch.empty(rows, D, device=dev), torch.empty(rows, D, device=dev), torch.zeros(1, device=dev)
                ops.gate_bwd(dout.to(dev), cv.to(dev), ca.to(dev), torch.tensor([a0], device=dev), dcv, dca, da, rows, D)
                return dcv, dca, da
            dcv, dca, da = _twice(run)
            w_cv, w_ca, w_a = R.gate_bwd(dout.double(), cv.double(), ca.double(), a0)
            e_cv, e_ca, e_a = R.rel_err(dcv, w_cv), R.rel_err(dca, w_ca), abs(float(da) - float(w_a))
            print(f"ordered gate_bwd ({rows}, {D}) a_v {a0}: dcv {e_cv:.2e}, dca {e_ca:.2e}, da {float(da):.6f} vs {float(w_a):.6f}")
            assert e_cv < 1e-6 and e_ca < 1e-6 and e_a < 1e-4 * max(1.0, abs(float(w_a)))
            assert (float(w_a) != 0.0) == (abs(a0) <= 2.0) and (float(da) != 0.0) == (abs(a0) <= 2.0)

    # -- cast + column sums in one row block per column block; the grouped form
    for rows, cols, group_rows in ((480, 300, None), (37, 5, None), (80, 300, 40)):
        x = torch.randn(rows, cols, generator=torch.Generator().manual_seed(rows + cols))
        groups = 1 if group_rows is None else rows // group_rows
        def run():
            y = torch.zeros(rows, ops.pad8(cols), dtype=torch.bfloat16, device=dev)
            cs = torch.zeros(groups * cols, device=dev)
            ops.cast_colsum_bf16(x.to(dev), cols, y, y.shape[1], rows, cols, cs, scale=0.5, group_rows=group_rows,
                                 colsum_stride=cols if group_rows else 0)
            return y, cs
        y, cs = _twice(run)
        ref = (x * 0.5).to(torch.bfloat16)
        want = ref.double().view(groups, rows // groups, cols).sum(1).reshape(-1)
        err = float((cs.cpu().double() - want).abs().max())
        print(f"ordered cast_colsum_bf16 ({rows}, {cols}) groups {groups}: sums {err:.2e}")
        assert torch.equal(y[:, :cols].cpu(), ref) and float(y[:, cols:].float().abs().max() if y.shape[1] > cols else 0.0) == 0.0
        assert err < 1e-3 * max(1.0, float(want.abs().max()))

    # -- column sums of a bf16 matrix: rows_per_block = rows; the grouped form
    for rows, cols, groups in ((500, 300, 1), (40, 520, 2)):
        dY = torch.randn(groups * rows, cols, generator=torch.Generator().manual_seed(rows + cols)).to(torch.bfloat16)
        ld = ops.pad8(cols)
        buf = torch.zeros(groups * rows, ld, dtype=torch.bfloat16)
        buf[:, :cols] = dY
        def run():
            if groups == 1:
                db = torch.full((cols,), SENT, device=dev)          # (accumulate = False: overwritten)
                ops.colsum_bf16(buf.to(dev), ld, db, False, rows, cols)
            else:
                db = torch.zeros(groups * cols, device=dev)
                ops.colsum_bf16_groups(buf.to(dev), ld, db, rows, cols, groups, cols)
            return (db,)
        (db,) = _twice(run)
        err = R.rel_err(db, dY.double().view(groups, rows, cols).sum(1).reshape(-1))
        print(f"ordered colsum_bf16 ({rows}, {cols}) groups {groups}: {err:.2e}")
        assert err < 1e-5
    torch.cuda.synchronize()
    print("ordered forms: all cases passed")


_CHILD = "import sys; sys.path.insert(0, sys.argv[1]); from tests.test_row_paths_gpu import child; child()"


def test_ordered_forms_in_child(dev):
    env = {k: v for k, v in os.environ.items() if not k.startswith("BMHRL_LN_")}
    env["BMHRL_DETERMINISTIC"] = "1"
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0, f"child exited {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-4000:]}"
    assert "ordered forms: all cases passed" in r.stdout
