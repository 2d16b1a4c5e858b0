"""tests/row_reference.py against torch's own operators and autograd, in float64 on the CPU: what the GPU comparisons of
tests/test_row_paths_gpu.py rest on.  Agreement is to rounding (1e-12 relative)."""
import pytest
import torch
import torch.nn.functional as F

from tests import row_reference as R

TOL = 1e-12


def _rand(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


@pytest.mark.parametrize("rows,D", [(37, 37), (5, 1028), (9, 300), (1, 4)])
def test_layernorm_matches_torch(rows, D):
    g = torch.Generator().manual_seed(rows + D)
    x = (_rand(g, rows, D) * 2 + 0.5).requires_grad_(True)
    gamma = (1 + 0.1 * _rand(g, D)).requires_grad_(True)
    beta = (0.1 * _rand(g, D)).requires_grad_(True)
    dy, add = _rand(g, rows, D), _rand(g, rows, D)
    y = F.layer_norm(x, (D,), gamma, beta, 1e-5)
    y.backward(dy)
    yr, mean, rstd = R.layernorm_fwd(x.detach(), gamma.detach(), beta.detach())
    assert R.rel_err(yr, y.detach()) < TOL
    assert R.rel_err(mean, x.detach().mean(1)) < TOL
    assert R.rel_err(rstd, 1 / torch.sqrt(x.detach().var(1, unbiased=False) + 1e-5)) < TOL
    dx, dg, db = R.layernorm_bwd(dy, x.detach(), gamma.detach(), add)
    assert R.rel_err(dx - add, x.grad) < TOL and R.rel_err(dg, gamma.grad) < TOL and R.rel_err(db, beta.grad) < TOL
    dx0, _, _ = R.layernorm_bwd(dy, x.detach(), gamma.detach())
    assert R.rel_err(dx0, x.grad) < TOL


@pytest.mark.parametrize("B,T,C,G", [(2, 5, 64, 32), (3, 7, 96, 32), (2, 3, 40, 8), (1, 1, 64, 32), (2, 4, 1024, 2)])
def test_groupnorm_matches_torch_on_the_transposed_layout(B, T, C, G):
    g = torch.Generator().manual_seed(B + T + C + G)
    x = (_rand(g, B, T, C) * 1.5 + 0.3).requires_grad_(True)
    gamma = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = (0.1 * _rand(g, C)).requires_grad_(True)
    dy = _rand(g, B, T, C)
    y = F.group_norm(x.transpose(1, 2), G, gamma, beta, 1e-5).transpose(1, 2)
    y.backward(dy)
    yr, mean, rstd = R.groupnorm_fwd(x.detach(), gamma.detach(), beta.detach(), G)
    assert R.rel_err(yr, y.detach()) < TOL
    xg = x.detach().reshape(B, T, G, C // G).permute(0, 2, 1, 3).reshape(B, G, -1)
    assert R.rel_err(mean, xg.mean(2)) < TOL
    assert R.rel_err(rstd, 1 / torch.sqrt(xg.var(2, unbiased=False) + 1e-5)) < TOL
    dx, dg, db = R.groupnorm_bwd(dy, x.detach(), gamma.detach(), G)
    assert R.rel_err(dx, x.grad) < TOL and R.rel_err(dg, gamma.grad) < TOL and R.rel_err(db, beta.grad) < TOL


@pytest.mark.parametrize("k", [1, 3, 6, 9])
@pytest.mark.parametrize("T", [1, 4, 17])
def test_unfold_is_the_operand_of_conv1d_same(k, T):
    """unfold(x) @ W.reshape(...) = conv1d(padding='same'), T < k included; even k has its extra step on the right"""
    g = torch.Generator().manual_seed(10 * k + T)
    B, C, Co = 2, 4, 5
    x, w, b = _rand(g, B, T, C), _rand(g, Co, C, k), _rand(g, Co)
    want = F.conv1d(x.transpose(1, 2), w, b, padding="same").transpose(1, 2)
    u = R.unfold1d(x, k)
    assert u.shape == (B * T, k * C)
    got = (u @ w.permute(2, 1, 0).reshape(k * C, Co) + b).reshape(B, T, Co)      # operand column j * C + c <-> w[o][c][j]
    assert R.rel_err(got, want) < TOL
    assert R.same_left(k) == (k - 1) // 2 and R.same_left(6) == 2


@pytest.mark.parametrize("k", [1, 3, 6, 9])
@pytest.mark.parametrize("T", [1, 4, 17])
def test_fold_is_the_adjoint_of_unfold(k, T):
    """<unfold(x), U> = <x, fold(U)>, and the k terms of fold1d_terms add up to fold1d"""
    g = torch.Generator().manual_seed(100 * k + T)
    B, C = 2, 4
    x, U = _rand(g, B, T, C), _rand(g, B * T, k * C)
    lhs, rhs = float((R.unfold1d(x, k) * U).sum()), float((x * R.fold1d(U, B, T, C, k)).sum())
    assert abs(lhs - rhs) <= TOL * max(1.0, abs(lhs))
    xr = x.clone().requires_grad_(True)
    (R.unfold1d(xr, k) * U).sum().backward()            # autograd through the copy loop of unfold1d
    assert R.rel_err(R.fold1d(U, B, T, C, k), xr.grad) < TOL
    terms = R.fold1d_terms(U, B, T, C, k)
    assert terms.shape == (k, B, T, C) and torch.equal(terms.sum(0), R.fold1d(U, B, T, C, k))


def test_embed_bwd_matches_autograd_of_the_mixed_lookup():
    g = torch.Generator().manual_seed(3)
    rows, V, D, sc, mix = 33, 5, 7, 2.5, 0.25
    tok, tok2 = torch.randint(0, V, (rows,), generator=g), torch.randint(0, V, (rows,), generator=g)
    dC = _rand(g, rows, D)
    for t2 in (tok2, None):
        table = _rand(g, V, D).requires_grad_(True)
        e = table[tok] * sc if t2 is None else table[tok] * sc * (1 - mix) + table[t2] * sc * mix
        e.backward(dC)
        assert R.rel_err(R.embed_bwd(tok, t2, mix, dC, V, sc), table.grad) < TOL
    want = torch.zeros(V, D, dtype=torch.float64)
    want.index_add_(0, tok, dC * sc * (1 - mix))
    want.index_add_(0, tok2, dC * sc * mix)
    assert R.rel_err(R.embed_bwd(tok, tok2, mix, dC, V, sc), want) < TOL


def test_scatter_add_rows_matches_index_add():
    g = torch.Generator().manual_seed(4)
    rows, D = 50, 6
    src = R.general_row_map(rows, g)
    assert int((src < 0).sum()) == 10 and src[src >= 0].unique().numel() < 40          # -1 entries and repeats
    dout = _rand(g, rows, D)
    keep = src >= 0
    want = torch.zeros(rows, D, dtype=torch.float64)
    want.index_add_(0, src[keep].long(), dout[keep])
    assert R.rel_err(R.scatter_add_rows(dout, src, rows), want) < TOL


@pytest.mark.parametrize("a0", [0.3, 2.0, -2.0, -2.5, 2.5])
def test_gate_bwd_matches_autograd_with_a_closed_clamp(a0):
    g = torch.Generator().manual_seed(5)
    rows, D = 12, 5
    cv, ca, dout = (_rand(g, rows, D) for _ in range(3))
    a = torch.tensor([a0], dtype=torch.float64, requires_grad=True)
    cvr, car = cv.clone().requires_grad_(True), ca.clone().requires_grad_(True)
    gt = torch.sigmoid(torch.clamp(a, -2, 2))
    (gt * cvr + (1 - gt) * car).backward(dout)
    dcv, dca, da = R.gate_bwd(dout, cv, ca, a0)
    assert R.rel_err(dcv, cvr.grad) < TOL and R.rel_err(dca, car.grad) < TOL
    assert abs(float(da) - float(a.grad)) <= TOL * max(1.0, abs(float(a.grad)))
    assert (float(a.grad) != 0.0) == (abs(a0) <= 2.0)                 # torch's clamp: gradient on the closed interval
