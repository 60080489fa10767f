"""The sigmoid router kernels (moe_sigmoid.hip) on one MI355X against ``moe_route_reference`` in fp64, the
``MoEFeedForwardBlock`` with ``router="sigmoid"`` and a shared expert with native against reference routing ops, and
a DeepSeek-style ``moe_tiny`` under checkpointing.

Bounds are derived, not measured (u = 2^-24):
* idx is EQUAL, as a condition on the inputs: with ``expf`` and IEEE division s is good to 2^-22 absolute, c = s + bias
  adds one rounding of a value below 1.5, a group score adds two of them and rounds once more, so it stays below
  2^-19; ``_margins`` asserts on the fp64 reference that the k-th chosen c against the best unchosen eligible one, and
  the last kept group's score against the best dropped one, differ by 2^-18 at least or tie exactly (equal logits
  give equal s in both implementations; SEED is chosen so that this holds for every case);
* gate: k + 3 roundings of values in [0, 1], times scale: 2^-20 max(1, scale);  probs_sum: T 2^-22 per entry;
* dlogits: the gate term is scale n_j (1 - s_j) (dg_j - <n, dg>), at most 2 scale max|dg| with about 2 k + 30
  roundings (s, S, the k-term inner product) of relative size u: below 2^-18 scale max|dg|; the probs term is
  q_e (1 - s_e) (dp_e - <q, dp>), at most 2 max|dp| and free of scale, its inner product a shuffle tree over at
  most 256 terms (10 levels): below 2^-19 max|dp|.  Asserted: the rounding of the result plus 2^-16 (scale max|dg| +
  max|dp|), the softmax file's constant with scale where it acts.
"""
import dataclasses

import pytest
import torch

from test_gpu_kernels import _tol
from test_gpu_moe_kernels import DEV, DTYPES, _eps, _rows, k  # noqa: F401  (k: the extension fixture)

from mipipe import checkpoint, ops
from mipipe.models import CONFIGS, build_lm_blocks
from mipipe.models.transformer import MoEFeedForwardBlock
from mipipe.ops import moe as M

pytestmark = pytest.mark.gpu

SEED = 0
SCALE = 2.5
# T, Ne, k, n_group, topk_group
SHAPES = [(193, 6, 2, 1, 1), (193, 16, 2, 4, 2), (130, 64, 6, 8, 3), (67, 96, 4, 3, 2), (67, 128, 8, 4, 2),
          (67, 256, 8, 8, 4), (67, 256, 8, 1, 1)]


def _inputs(T, Ne, dtype, with_bias):
    """Logits with row 1 all equal (ties go to the lower group and expert) and -inf entries in row 2 (s = 0)."""
    g = torch.Generator().manual_seed(SEED)
    lg = torch.randn(T, Ne, generator=g) + torch.linspace(-1, 1, Ne)
    lg[1] = 0.25
    lg[2, ::3] = float("-inf")
    bias = torch.rand(Ne, generator=g) - 0.5
    return lg.to(dtype).to(DEV), (bias.to(DEV) if with_bias else None)


def _margins(lg, bias, kk, n_group, topk_group):
    """Every selection boundary of the fp64 reference is an exact tie or at least 2^-18 wide."""
    c = torch.sigmoid(lg.double()) + (0 if bias is None else bias.double())
    T, Ne = c.shape
    if n_group > 1:
        score = c.view(T, n_group, -1).topk(2, -1).values.sum(-1).sort(-1, descending=True).values
        if topk_group < n_group:
            gap = score[:, topk_group - 1] - score[:, topk_group]
            assert ((gap == 0) | (gap >= 2.0 ** -18)).all(), gap.min().item()
        keep = score[:, topk_group - 1].view(T, 1, 1)
        full = c.view(T, n_group, -1).topk(2, -1).values.sum(-1, keepdim=True)
        c = c.view(T, n_group, -1).masked_fill(full < keep, float("-inf")).view(T, Ne)   # ties: both stay, gap 0
    top = c.sort(-1, descending=True).values
    if kk < Ne:
        gap = top[:, kk - 1] - top[:, kk]
        assert ((gap == 0) | (gap >= 2.0 ** -18)).all(), gap.min().item()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("renorm", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_route_sigmoid(k, shape, renorm, with_bias, dtype):
    T, Ne, kk, n_group, topk_group = shape
    lg, bias = _inputs(T, Ne, dtype, with_bias)
    _margins(lg, bias, kk, n_group, topk_group)
    kw = dict(score="sigmoid", bias=bias, n_group=n_group, topk_group=topk_group, renormalize=renorm, scale=SCALE)
    lg.requires_grad_()
    idx, gate, probs = ops.moe_route(lg, kk, **kw)
    ld = lg.detach().double().requires_grad_()
    r_idx, r_gate, r_probs = M.moe_route_reference(ld, kk, **kw)
    assert idx.dtype == torch.int32 and gate.dtype == torch.float32 and probs.dtype == torch.float32
    assert torch.equal(idx, r_idx)
    assert idx[1].tolist() == list(range(kk)) or with_bias    # all-equal logits: the lower group, the lower expert
    assert ((gate.double() - r_gate).abs() <= 2.0 ** -20 * SCALE).all()
    assert ((probs.double() - r_probs).abs() <= T * 2.0 ** -22).all()

    g = torch.Generator(device=DEV).manual_seed(1)
    dgate = torch.randn(T, kk, device=DEV, generator=g)
    dprobs = torch.randn(Ne, device=DEV, generator=g)
    ((gate * dgate).sum() + (probs * dprobs).sum()).backward()
    ((r_gate * dgate.double()).sum() + (r_probs * dprobs.double()).sum()).backward()
    assert lg.grad.dtype == dtype
    err = (lg.grad.double() - ld.grad).abs()
    slack = 2.0 ** -16 * (SCALE * dgate.abs().max().item() + dprobs.abs().max().item())
    assert (err <= _eps(dtype) * ld.grad.abs() + slack).all(), err.max().item()
    assert (lg.grad != 0).any() and (lg.grad[2, ::3] == 0).all()

    grad = lg.grad.clone()      # the same bits on every run
    lg.grad = None
    again = ops.moe_route(lg, kk, **kw)
    ((again[1] * dgate).sum() + (again[2] * dprobs).sum()).backward()
    assert all(torch.equal(a, b) for a, b in zip(again, (idx, gate, probs))) and torch.equal(lg.grad, grad)


def test_softmax_score_is_the_existing_kernel(k):
    lg = _inputs(193, 64, torch.bfloat16, False)[0]
    for a, b in zip(ops.moe_route(lg, 6, score="softmax"), k.moe_route_fwd(lg, 6)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("tiles", [1, 42])
def test_bias_update(k, tiles):
    """Mean load 6: experts above it move by -rate, below by +rate, the ones at the mean not at all; exact."""
    load = torch.tensor([10, 2, 6, 6, 0, 12] * tiles + [6] * (4 if tiles > 1 else 0), dtype=torch.int32, device=DEV)
    bias = torch.rand(load.numel(), device=DEV) - 0.5
    want = bias + torch.tensor(1e-3, device=DEV) * torch.sign(6.0 - load.float())
    at_mean = load == 6
    assert torch.equal(want[at_mean], bias[at_mean]) and (want[~at_mean] != bias[~at_mean]).all()
    ops.moe_bias_update(bias, load, 1e-3)
    assert torch.equal(bias, want) and (load == 0).all()


# ------------------------------------------------------------------ the block and the model
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("expert_gemm", ["loop", "grouped"])
def test_sigmoid_block_native_against_reference_ops(k, expert_gemm, dtype, monkeypatch):
    torch.manual_seed(0)
    blk = MoEFeedForwardBlock(256, 512, 8, 2, capacity_factor=None, expert_gemm=expert_gemm, router="sigmoid",
                              n_group=4, topk_group=2, routed_scale=2.5, n_shared_experts=1).to(DEV, dtype).train()
    with torch.no_grad():
        blk.router_weight.normal_(std=0.3)
        blk.router_bias.uniform_(-0.2, 0.2)
    x = (_rows(384, 256, dtype, 8) + 1.0).view(2, 192, 256).requires_grad_()
    dy = _rows(384, 256, dtype, 9).view(2, 192, 256)
    params = dict(blk.named_parameters())
    assert "shared_w1" in params and blk.router_bias.dtype == torch.float32

    def run():
        y = blk(x)
        return [y.detach()] + list(torch.autograd.grad(y, [x] + list(params.values()), dy))

    got = run()
    for name in ("moe_route", "moe_assign", "moe_assign_sorted", "moe_dispatch", "moe_combine"):
        monkeypatch.setattr(ops, name, getattr(M, name + "_reference"))
    want = run()
    atol, rtol = _tol(dtype)
    assert torch.allclose(got[0].float(), want[0].float(), atol=atol, rtol=rtol)
    assert torch.allclose(got[1].float(), want[1].float(), atol=atol * 5, rtol=rtol * 5)
    for n, g, w in zip(params, got[2:], want[2:]):
        assert (g.float() - w.float()).abs().max().item() <= 2e-2 * (w.float().abs().max().item() + 1e-6), n
        assert (g != 0).any(), n
    assert int(blk.expert_load.sum()) == 2 * 384 * 2      # two counted forwards of T k choices


def test_deepseek_style_moe_tiny_trains_under_checkpoint(k):
    cfg = dataclasses.replace(CONFIGS["moe_tiny"], moe_router="sigmoid", moe_n_group=2, moe_topk_group=1,
                              moe_routed_scale=2.5, n_shared_experts=1, moe_bias_rate=1e-3)
    torch.manual_seed(0)
    blocks = [b.to(DEV) for b in build_lm_blocks(cfg, dtype=torch.bfloat16)]
    moe = [b for b in blocks if isinstance(b, MoEFeedForwardBlock)]
    tok = torch.randint(0, cfg.vocab, (2, cfg.seq_len + 1), generator=torch.Generator().manual_seed(7)).to(DEV)
    from mipipe.optim import FlatAdam
    opt = FlatAdam([p for b in blocks for p in b.parameters()], lr=1e-3)
    for step in range(2):
        opt.zero_grad()
        h = blocks[0](tok[:, :-1])
        for b in blocks[1:-1]:
            h = checkpoint(b, h)
        loss = ops.cross_entropy(blocks[-1](h).reshape(-1, cfg.vocab), tok[:, 1:].reshape(-1))
        loss.backward()
        opt.step(opt.grad_sumsq())
        assert torch.isfinite(loss).all()
        for b in moe:    # the recompute did not count: T k choices per forward
            assert int(b.expert_load.sum()) == 2 * cfg.seq_len * cfg.experts_per_token
            b.update_router_bias()
            assert (b.expert_load == 0).all() and b.router_bias.dtype == torch.float32
    assert any((b.router_bias != 0).any() for b in moe)
