"""Tuning aid: one CriticTrainer.step() (B=64, L=30, d_caps=300, H=600) on the HIP training kernels, beside the same step
through stock nn.LSTM / nn.GRU autograd on the same device (what a user could do without this package).  Eager, wall
clock over synchronised repeats; a per-phase split of the HIP step follows."""
import sys, os, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bmhrl_amd import synthetic as syn
from bmhrl_amd.critic_train import CriticTrainer
from bmhrl_amd.model.bm_hrl_agent import SegmentCritic
from tests import critic_reference as R

B, L, D, V, PAD, REPS = 64, 30, 300, 1000, 1, 10
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(0)
table = (torch.randn(V, D, generator=g) * 17.3).to(dev)
tokens = torch.randint(2, V, (B, L), generator=g)
tokens[torch.rand(B, L, generator=g) < 0.2] = PAD
tokens[:, 0] = 2
tokens = tokens.to(dev)
labels = (torch.rand(B, L, generator=g) < 0.3).float().to(dev)
embed = lambda tok: table[tok]


def timed(fn, reps=REPS):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


crit = SegmentCritic(syn.default_cfg()).to(dev)
tr = CriticTrainer(crit, embed, PAD, lr=1e-3, pos_weight=3.0)
hip = timed(lambda: tr.step(tokens, labels))
emb, mask = embed(tokens), tokens != PAD
fwd = timed(lambda: crit.masked_bce(emb, labels, mask, 3.0))


def fwd_bwd():
    tr.optimizer.zero_grad(set_to_none=True)
    crit.masked_bce(emb, labels, mask, 3.0)[0].backward()


fb = timed(fwd_bwd)
tr.close()

ref = R.CriticRef(D).to(dev)
opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
pw = torch.tensor(3.0, device=dev)


def stock_step():
    opt.zero_grad(set_to_none=True)
    with torch.no_grad():
        x = embed(tokens)
    l = torch.nn.functional.binary_cross_entropy_with_logits(ref(x).squeeze(-1), labels, pos_weight=pw, reduction="none")
    m = (tokens != PAD).float()
    ((l * m).sum() / m.sum()).backward()
    opt.step()


stock = timed(stock_step)
print(f"critic train step B={B} L={L} d_caps={D}: HIP {hip:.0f} us (forward {fwd:.0f} us, forward + backward {fb:.0f} us), "
      f"stock nn.LSTM/nn.GRU autograd {stock:.0f} us")
