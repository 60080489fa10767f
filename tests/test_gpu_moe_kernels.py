"""The mixture-of-experts kernels (moe.hip) on one MI355X against the eager references in fp64, at the smallest
shapes at which they can go wrong, the ``MoEFeedForwardBlock`` with native against reference routing ops, and the
``moe_tiny`` model end to end.  Every kernel comes from mipipe/_C.so: the tests fail if the extension lacks it.

Bounds are derived, not measured (u = 2^-24, fp32's unit roundoff):
* gate: k + 3 roundings of values in [0, 1] (the exponentials, their sum, the division): 2^-20 absolute;
* probs_sum: T fp32 additions of values in [0, 1]: T * 2^-22 per entry;
* a row sum of k weighted rows (+ a residual): one rounding of the result (2^-8 relative in bf16, 2^-23 in fp32)
  plus k * 2^-23 * sum |terms|;
* dgate, a dot product of E terms: E * 2^-24 * sum |dy ye|;
* dlogits: the rounding of the result plus 2^-16 (max |dgate| + max |dprobs|): at most 256 terms in the inner
  product with the softmax, gates good to 2^-20.
"""
import copy
import warnings

import pytest
import torch

from test_gpu_kernels import _tol
from test_gpu_llama_kernels import _assert_model_close

from mipipe import checkpoint, ops
from mipipe.models import CONFIGS, build_lm_blocks
from mipipe.models.transformer import MoEFeedForwardBlock
from mipipe.ops import moe as M
from mipipe.optim import FlatAdam

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float32]
# T, Ne, k, C: drop shares 0.24, 0.32, 0.41, 0.39 and 0.40 on the logits below
TABLE = [(384, 4, 2, 192), (384, 8, 2, 96), (193, 6, 2, 50), (3000, 8, 2, 640), (1000, 128, 8, 64)]


@pytest.fixture(scope="module")
def k():
    from mipipe._native_loader import kernels

    kern = kernels()
    for name in ("moe_route_fwd", "moe_route_bwd", "moe_assign", "moe_gather_slots", "moe_gather_tokens",
                 "moe_combine_bwd"):
        assert hasattr(kern, name), name
    return kern


def _logits(T, Ne, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(0)
    return (torch.randn(T, Ne, generator=g) + torch.linspace(-1, 1, Ne)).to(dtype).to(DEV)


def _eps(dtype):
    return 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -23


_TABLES = {}


def _tables(T, Ne, kk, C):
    """(idx, gate, slot, src, counts) from the REFERENCE ops, computed once per shape and never changed; asserts that
    the capacity binds: a drop share in [0.1, 0.6] and at least one expert under capacity."""
    key = (T, Ne, kk, C)
    if key not in _TABLES:
        idx, gate, _ = M.moe_route_reference(_logits(T, Ne), kk)
        slot, src, counts = M.moe_assign_reference(idx, Ne, C)
        drop = (slot < 0).float().mean().item()
        assert 0.1 <= drop <= 0.6, drop
        assert counts.min().item() < C < counts.max().item()
        _TABLES[key] = (idx, gate, slot, src, counts)
    return _TABLES[key]


# ------------------------------------------------------------------ route
def _check_route(logits, kk):
    T, Ne = logits.shape
    idx, gate, probs = ops.moe_route(logits, kk)
    r_idx, r_gate, r_probs = M.moe_route_reference(logits.double(), kk)
    assert idx.dtype == torch.int32 and gate.dtype == torch.float32 and probs.dtype == torch.float32
    assert torch.equal(idx, r_idx)
    assert ((gate.double() - r_gate).abs() <= 2.0 ** -20).all()
    assert ((probs.double() - r_probs).abs() <= T * 2.0 ** -22).all()
    return idx, gate, probs


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Ne,kk", [(2, 1), (2, 2), (4, 2), (6, 1), (6, 2), (8, 2), (8, 8), (64, 2), (64, 8), (128, 8),
                                   (256, 1), (256, 8)])
def test_route_fwd(k, Ne, kk, dtype):
    for T in (1, 63, 64, 193, 1000):
        _check_route(_logits(T, Ne, dtype), kk)


@pytest.mark.parametrize("Ne,kk", [(8, 2), (64, 8), (128, 8), (256, 8)])
def test_route_fwd_ties(k, Ne, kk):
    """Logits quantised to the 8 levels -2, -1.5 .. 1.5: most rows tie at the k-th place (0.84 - 1.0 of them from
    64 experts on, 0.30 with 8 experts), and the lower expert must win."""
    lg = ((_logits(193, Ne, torch.float32).clamp(-2, 2) * 2).floor().clamp(-4, 3) / 2).to(torch.bfloat16)
    assert lg.unique().numel() == 8
    vals = lg.float().sort(-1, descending=True).values
    assert (vals[:, kk - 1] == vals[:, kk]).float().mean() > (0.5 if Ne >= 64 else 0.25)
    _check_route(lg, kk)
    _check_route(lg.float(), kk)


@pytest.mark.parametrize("dtype", DTYPES)
def test_route_fwd_neg_inf(k, dtype):
    lg = _logits(193, 8, dtype)
    lg[::3, 1:] = float("-inf")      # a single finite value: the other choice is a -inf
    lg[1::3, ::2] = float("-inf")
    idx, gate, probs = _check_route(lg, 2)
    assert (gate[::3, 0] == 1).all() and (gate[::3, 1] == 0).all() and (idx[::3, 1] == 1).all()
    assert torch.isfinite(probs).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_dprobs", [False, True])
@pytest.mark.parametrize("T,Ne,kk", [(193, 6, 2), (64, 8, 8), (65, 64, 2), (193, 128, 8), (63, 256, 8)])
def test_route_bwd(k, T, Ne, kk, with_dprobs, dtype):
    lg = _logits(T, Ne, dtype).requires_grad_()
    g = torch.Generator(device=DEV).manual_seed(1)
    dgate = torch.randn(T, kk, device=DEV, generator=g)
    dprobs = torch.randn(Ne, device=DEV, generator=g) if with_dprobs else None
    idx, gate, probs = ops.moe_route(lg, kk)
    out = (gate * dgate).sum() + ((probs * dprobs).sum() if with_dprobs else 0.0)
    out.backward()
    ld = lg.detach().double().requires_grad_()
    r_idx, r_gate, r_probs = M.moe_route_reference(ld, kk)
    ((r_gate * dgate.double()).sum() + ((r_probs * dprobs.double()).sum() if with_dprobs else 0.0)).backward()
    assert lg.grad.dtype == dtype
    scale = dgate.abs().max().item() + (dprobs.abs().max().item() if with_dprobs else 0.0)
    err = (lg.grad.double() - ld.grad).abs()
    assert (err <= _eps(dtype) * ld.grad.abs() + 2.0 ** -16 * scale).all(), err.max().item()
    if not with_dprobs:   # the unselected experts get exactly 0
        sel = torch.zeros(T, Ne, dtype=torch.bool, device=DEV).scatter_(1, idx.long(), True)
        assert (lg.grad[~sel] == 0).all() and (lg.grad[sel] != 0).any()


# ------------------------------------------------------------------ assign
def _check_assign(idx, Ne, C):
    got = ops.moe_assign(idx, Ne, C)
    want = M.moe_assign_reference(idx, Ne, C)
    for g, w, name in zip(got, want, ("slot", "src", "counts")):
        assert g.dtype == torch.int32 and torch.equal(g, w), name
    again = ops.moe_assign(idx, Ne, C)
    assert all(torch.equal(a, b) for a, b in zip(got, again))   # the same bits on every run
    return got


@pytest.mark.parametrize("T,Ne,kk,C", TABLE)
def test_assign(k, T, Ne, kk, C):
    idx = _tables(T, Ne, kk, C)[0]
    slot, src, counts = _check_assign(idx, Ne, C)
    assert int(counts.sum()) == T * kk and int((src >= 0).sum()) == int((slot >= 0).sum())
    native_idx = ops.moe_route(_logits(T, Ne), kk)[0]   # and from the native route, the same tables
    assert torch.equal(native_idx, idx)


def test_assign_one_expert_gets_every_token_and_one_gets_none(k):
    T, Ne, C = 1500, 6, 320
    idx = torch.empty(T, 2, dtype=torch.int32, device=DEV)
    idx[:, 0] = 3                                        # every first choice
    idx[:, 1] = torch.arange(T, device=DEV) % 2 * 4      # experts 0 and 4; 1, 2 and 5 get nothing
    slot, src, counts = _check_assign(idx, Ne, C)
    assert counts.tolist() == [750, 0, 0, 1500, 750, 0]
    assert (slot[:C, 0] == 3 * C + torch.arange(C, device=DEV)).all() and (slot[C:, 0] == -1).all()
    assert (src[C:3 * C] == -1).all() and (src[5 * C:] == -1).all()
    _check_assign(idx[:1], Ne, 1)
    _check_assign(idx[:, :1].contiguous(), Ne, C)


def test_assign_refusals(k):
    idx = torch.zeros(4, 2, dtype=torch.int32, device=DEV)
    for bad in ((idx.long(), 4, 4), (idx, 1, 4), (idx, 257, 4), (idx, 4, 0), (idx, 256, 2 ** 23), (idx.cpu(), 4, 4),
                (idx[:, :0], 4, 4)):
        with pytest.raises(RuntimeError):
            k.moe_assign(*bad)
    with pytest.raises(RuntimeError):
        k.moe_route_fwd(torch.zeros(4, 257, device=DEV), 2)
    with pytest.raises(RuntimeError):
        k.moe_route_fwd(torch.zeros(4, 4, device=DEV), 5)
    with pytest.raises(RuntimeError):
        k.moe_gather_slots(torch.zeros(4, 12, device=DEV, dtype=torch.bfloat16), idx.view(-1), 2)   # 24-byte rows
    # an index out of range addresses nothing: the slot is dropped, the row zero-filled
    wild = torch.tensor([[7, -3], [1, 2]], dtype=torch.int32, device=DEV)
    slot, src, counts = k.moe_assign(wild, 4, 2)
    assert slot.tolist() == [[-1, -1], [2, 4]] and counts.tolist() == [0, 1, 1, 0]
    x = torch.ones(2, 8, device=DEV)
    xe = k.moe_gather_slots(x, torch.tensor([0, 99, -1, 3], dtype=torch.int32, device=DEV), 2)
    assert xe.sum(1).tolist() == [8.0, 0.0, 0.0, 8.0]
    y = k.moe_gather_tokens(xe, torch.tensor([[0, 9], [-1, 3]], dtype=torch.int32, device=DEV))
    assert y.sum(1).tolist() == [8.0, 8.0]
    torch.cuda.synchronize()


# ------------------------------------------------------------------ dispatch
def _rows(n, E, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, E, generator=g).to(dtype).to(DEV)


def _sum_bound(ref, mag, dtype, kk):
    return _eps(dtype) * ref.abs() + kk * 2.0 ** -23 * mag


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("E", [64, 256, 520])
def test_dispatch(k, E, dtype):
    T, Ne, kk, C = TABLE[2]
    _, _, slot, src, _ = _tables(T, Ne, kk, C)
    x = _rows(T, E, dtype, 2).requires_grad_()
    xe = ops.moe_dispatch(x, slot, src)
    want = torch.where((src >= 0)[:, None], x.detach().index_select(0, (src.clamp(min=0) // kk).long()),
                       torch.zeros((), device=DEV, dtype=dtype))
    assert xe.shape == (Ne * C, E) and torch.equal(xe, want)
    dxe = _rows(Ne * C, E, dtype, 3)
    xe.backward(dxe)
    rows = dxe.double()[slot.clamp(min=0).long()] * (slot >= 0)[..., None]      # [T, k, E]
    ref, mag = rows.sum(1), rows.abs().sum(1)
    assert ((x.grad.double() - ref).abs() <= _sum_bound(ref, mag, dtype, kk)).all()
    assert (x.grad[(slot < 0).all(1)] == 0).all()


# ------------------------------------------------------------------ combine
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("shape,E", [(TABLE[2], 520), (TABLE[0], 256), (TABLE[4], 64)])
def test_combine_and_backward(k, shape, E, residual, dtype):
    T, Ne, kk, C = shape
    _, gate, slot, src, _ = _tables(T, Ne, kk, C)
    ye = _rows(Ne * C, E, dtype, 4).requires_grad_()
    gt = gate.clone().requires_grad_()
    res = _rows(T, E, dtype, 5).requires_grad_() if residual else None
    y = ops.moe_combine(ye, gt, slot, src, residual=res)
    keep = (slot >= 0)[..., None]
    rows = ye.detach().double()[slot.clamp(min=0).long()] * keep
    terms = rows * gate.double()[..., None]
    ref, mag = terms.sum(1), terms.abs().sum(1)
    plain = rows.sum(1)
    if residual:
        ref, mag, plain = ref + res.detach().double(), mag + res.detach().double().abs(), plain + res.detach().double()
    bound = _sum_bound(ref, mag, dtype, kk)
    assert ((ref - plain).abs() > bound).float().mean() >= 0.25   # the gate matters
    assert ((y.double() - ref).abs() <= bound).all()
    dy = _rows(T, E, dtype, 6)
    y.backward(dy)
    again = ops.moe_combine(ye.detach(), gate, slot, src, residual=None if res is None else res.detach())
    assert torch.equal(again, y.detach())
    # dye[s] = gate[a] dy[a // k]; dgate[a] = <dy, ye[s]>
    full = src >= 0
    a = src.clamp(min=0).long()
    r_dye = torch.where(full[:, None], gate.double().view(-1)[a][:, None] * dy.double()[a // kk], torch.zeros((), device=DEV, dtype=torch.float64))
    assert ((ye.grad.double() - r_dye).abs() <= _eps(dtype) * r_dye.abs()).all()
    assert (ye.grad[~full] == 0).all()
    prod = dy.double()[:, None, :] * rows
    r_dg = prod.sum(-1)
    assert ((gt.grad.double() - r_dg).abs() <= E * 2.0 ** -24 * prod.abs().sum(-1) + 1e-30).all()
    assert (gt.grad[slot < 0] == 0).all() and (gt.grad[slot >= 0] != 0).any()
    if residual:
        assert torch.equal(res.grad, dy)
    dye2, dg2 = k.moe_combine_bwd(dy, ye.detach(), gate, src)
    assert torch.equal(dye2, ye.grad) and torch.equal(dg2, gt.grad)   # the same bits on every run


def test_unsupported_width_runs_the_reference_and_warns_once(k):
    T, Ne, kk, C = TABLE[2]
    _, gate, slot, src, _ = _tables(T, Ne, kk, C)
    x = _rows(T, 12, torch.bfloat16, 7)     # 24-byte rows
    M._noted.discard(("moe_dispatch", (T, 12), torch.bfloat16))
    with pytest.warns(UserWarning, match="16-byte"):
        xe = ops.moe_dispatch(x, slot, src)
    assert torch.equal(xe, M.moe_dispatch_reference(x, slot, src))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ops.moe_dispatch(x, slot, src)


# ------------------------------------------------------------------ the block
D_MODEL, FF, NE, TOPK = 256, 512, 4, 2


def _reference_forward(blk, logits, x2, xr2):
    """MoEFeedForwardBlock.forward after the router GEMM with the REFERENCE routing ops (the experts' GEMMs and the
    gate kernel are the block's own)."""
    tokens = x2.shape[0]
    idx, gate, probs_sum = M.moe_route_reference(logits, TOPK)
    cap = ops.moe_capacity(tokens, NE, TOPK, blk.capacity_factor)
    slot, src, counts = M.moe_assign_reference(idx, NE, cap)
    dprobs = counts.float() * (blk.aux_coef * blk.aux_scale * NE / (float(tokens) * tokens * TOPK))
    gate = ops.moe_attach_aux(gate, probs_sum, dprobs)
    ye = blk.experts(M.moe_dispatch_reference(x2, slot, src), cap)
    return M.moe_combine_reference(ye, gate, slot, src, xr2), (slot < 0).float().mean()


def _skewed_block(capacity_factor):
    """The block with a router that loads its experts unevenly on ``_skewed_input``: inputs with a common mean
    direction, router rows of different sums.  At ``capacity_factor=1.0`` about a quarter of the choices drop."""
    torch.manual_seed(0)
    blk = MoEFeedForwardBlock(D_MODEL, FF, NE, TOPK, capacity_factor=capacity_factor).to(DEV, torch.bfloat16).train()
    with torch.no_grad():
        blk.router_weight.normal_(std=0.3)
        blk.router_weight += (torch.linspace(-1, 1, NE)[:, None] * 0.02).to(DEV, torch.bfloat16)
    return blk


def _skewed_input(seed):
    return (_rows(384, D_MODEL, torch.bfloat16, seed) + 1.0).view(2, 192, D_MODEL)


@pytest.mark.parametrize("capacity_factor", [1.0, None])
def test_block_native_against_reference_ops(k, capacity_factor):
    blk = _skewed_block(capacity_factor)
    opt = FlatAdam(blk.parameters(), lr=1e-3)
    x = _skewed_input(8).requires_grad_()
    dy = _rows(384, D_MODEL, torch.bfloat16, 9)
    xn = ops.add_dropout_rms_norm(x, None, blk.norm_weight, blk.eps, 0.0, True).reshape(-1, D_MODEL)
    logits = ops.linear(xn, blk.router_weight)        # ONE router GEMM: both paths route the same logits
    xr2 = x.reshape(-1, D_MODEL)

    gate, slot, src, cap = blk.route(logits, 384)
    y = ops.moe_combine(blk.experts(ops.moe_dispatch(xn, slot, src), cap), gate, slot, src, residual=xr2)
    y_ref, drop = _reference_forward(blk, logits, xn, xr2)
    assert cap == (192 if capacity_factor == 1.0 else 384)
    assert float(blk.last_drop_fraction) == float(drop)
    if capacity_factor == 1.0:   # the capacity binds: a drop share in [0.1, 0.6], an expert under capacity
        assert 0.1 <= float(drop) <= 0.6 and int((src < 0).sum()) > 0
    else:
        assert float(drop) == 0.0

    def grads(out):
        opt.zero_grad()
        x.grad = None
        out.backward(dy, retain_graph=True)
        opt.fold_grads()
        torch.cuda.synchronize()
        return x.grad.clone(), {n: p.main_grad.clone() for n, p in blk.named_parameters()}

    gx, gp = grads(y)
    rx, rp = grads(y_ref)
    atol, rtol = _tol(torch.bfloat16)
    assert torch.allclose(y.float(), y_ref.float(), atol=atol, rtol=rtol)
    assert torch.allclose(gx.float(), rx.float(), atol=atol * 5, rtol=rtol * 5)
    assert gp.keys() == rp.keys() and len(gp) == 2 + 2 * NE
    for n, g in gp.items():
        assert (g - rp[n]).abs().max().item() <= 2e-2 * (rp[n].abs().max().item() + 1e-6), n
        assert (g != 0).any(), n
    # and the whole forward is those pieces
    assert torch.equal(blk(x.detach()).view(-1, D_MODEL), y.detach())


def test_block_checkpoint_and_deferred_wgrad_bit_exact(k):
    blk = _skewed_block(1.0)
    opt = FlatAdam(blk.parameters(), lr=1e-3)
    base = _skewed_input(10)
    dy = _rows(384, D_MODEL, torch.bfloat16, 11).view(2, 192, D_MODEL)

    def run(ckpt=False, deferred=False):
        opt.zero_grad()
        x = base.clone().requires_grad_()
        if deferred:
            with ops.deferred_wgrad():
                y = blk(x)
                y.backward(dy)
            ops.flush_wgrad()
        else:
            y = checkpoint(blk, x) if ckpt else blk(x)
            y.backward(dy)
        opt.fold_grads()
        torch.cuda.synchronize()
        return [y.detach(), x.grad] + [p.main_grad.clone() for p in blk.parameters()]

    plain = run()
    assert all((t != 0).any() for t in plain) and 0.1 <= float(blk.last_drop_fraction) <= 0.6
    for other in (run(ckpt=True), run(deferred=True), run()):
        assert all(torch.equal(a, b) for a, b in zip(plain, other))


# ------------------------------------------------------------------ the model
def _cfg():
    return CONFIGS["moe_tiny"]


def _data(cfg, n, seed=7):
    tok = torch.randint(0, cfg.vocab, (n, cfg.seq_len + 1), generator=torch.Generator().manual_seed(seed))
    return tok[:, :-1].to(DEV), tok[:, 1:].contiguous().to(DEV)


def _loss(cfg, model, x, t):
    return ops.cross_entropy(model(x).reshape(-1, cfg.vocab), t.reshape(-1))


def test_moe_tiny_step_against_the_eager_model(k, monkeypatch):
    """One forward-backward of moe_tiny in bf16 through the kernels against the same weights in fp32 on the eager
    references (CPU), by test_gpu_llama_kernels' rule, with the routing pinned: the fp32 model takes the expert
    indices the bf16 model chose (its gates, its ``probs_sum`` and everything else are its own).  Unpinned, the two
    precisions order a few near-ties differently, 3 and 8 of the 384 tokens in the two layers between the EAGER
    bf16 and fp32 models on the CPU alone, and that, not the kernels, then moves the embedding's gradient by
    0.0016 - 0.0020 where the rule allows 0.0007 of a maximum of 0.035 (the losses agree to 2e-5 either way).  The
    share of tokens whose own fp32 choice differs is asserted to stay below 5 %; the router itself is compared
    exactly in the tests above.  Only this first step is compared: after an update the routing may differ."""
    cfg = _cfg()
    torch.manual_seed(0)
    blocks = build_lm_blocks(cfg, dtype=torch.bfloat16)
    model = torch.nn.Sequential(*copy.deepcopy(blocks)).to(DEV).train()
    assert sum(isinstance(b, MoEFeedForwardBlock) for b in model) == 2
    x, t = _data(cfg, 2)
    route, chosen, flips = ops.moe_route, [], []

    def record(logits, kk):
        out = route(logits, kk)
        chosen.append(out[0].cpu())
        return out

    def replay(logits, kk):
        idx = chosen.pop(0)
        flips.append((M.moe_route_reference(logits, kk)[0] != idx).any(1).float().mean().item())
        gate = torch.softmax(logits.gather(1, idx.long()), -1)
        return idx, gate, torch.softmax(logits, -1).sum(0)

    monkeypatch.setattr(ops, "moe_route", record)
    opt = FlatAdam(model.parameters(), lr=1e-3)
    opt.zero_grad()
    loss = _loss(cfg, model, x, t)
    loss.backward()
    opt.fold_grads()
    torch.cuda.synchronize()
    grads = {n: p.main_grad.clone() for n, p in model.named_parameters()}
    assert len(chosen) == 2
    monkeypatch.setattr(ops, "moe_route", replay)
    ref = torch.nn.Sequential(*copy.deepcopy(blocks)).float().train()
    ref_loss = _loss(cfg, ref, x.cpu(), t.cpu())
    ref_loss.backward()
    assert len(flips) == 2 and not chosen and max(flips) < 0.05, flips
    ref_grads = {n: p.grad for n, p in ref.named_parameters()}
    _assert_model_close(float(loss.detach()), grads, float(ref_loss.detach()), ref_grads)


def test_moe_tiny_training_is_deterministic(k):
    cfg = _cfg()
    x, t = _data(cfg, 2)

    def run():
        torch.manual_seed(0)
        model = torch.nn.Sequential(*build_lm_blocks(cfg, dtype=torch.bfloat16)).to(DEV).train()
        opt = FlatAdam(model.parameters(), lr=1e-3)
        losses = []
        for _ in range(3):
            opt.zero_grad()
            loss = _loss(cfg, model, x, t)
            loss.backward()
            opt.step(opt.grad_sumsq())
            losses.append(loss.detach().clone())
        torch.cuda.synchronize()
        aux = [float(b.last_aux) for b in model if isinstance(b, MoEFeedForwardBlock)]
        return torch.stack(losses), aux

    a, aux_a = run()
    b, aux_b = run()
    assert torch.isfinite(a).all() and torch.equal(a, b) and aux_a == aux_b
    assert a[2] < a[0] and all(v >= 0.99 for v in aux_a)
