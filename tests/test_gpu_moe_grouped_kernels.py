"""The dropless mixture-of-experts path on one MI355X: ``moe_assign_sorted`` (moe.hip) bit for bit against its eager
reference, the three grouped GEMM kernels (gemm_grouped.hip) against themselves expert by expert and against fp32
references, the ``MoEFeedForwardBlock`` with ``expert_gemm="grouped"``, and ``moe_tiny`` with that option end to end.
Every kernel comes from mipipe/_C.so: the tests fail if the extension lacks it.

Bounds (set by the operand formats, not measured):
* bf16 outputs: ``|y - ref| <= 2^-8 |ref| + 1e-3 max|ref|``: the one bf16 rounding of the result (at most ``2^-9``
  relative) with a factor 2 of margin, plus the fp32 accumulation of at most 384 products;
* the fp32 weight gradient: ``1e-3 max|ref|``, test_wgrad_split_k's bound.
"""
import copy
import dataclasses
import importlib
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

GL = importlib.import_module("mipipe.ops.grouped_linear")   # the module: ops.grouped_linear is the function

DEV = "cuda"
BF = torch.bfloat16


@pytest.fixture(scope="module")
def k():
    from mipipe._native_loader import kernels

    kern = kernels()
    for name in ("moe_assign_sorted", "grouped_gemm_rows", "grouped_gemm_wgrad"):
        assert hasattr(kern, name), name
    return kern


# ------------------------------------------------------------------ sorted assignment
def _logits(T, Ne):
    g = torch.Generator().manual_seed(0)
    return (torch.randn(T, Ne, generator=g) + torch.linspace(-1, 1, Ne)).to(BF).to(DEV)


def _check_sorted(idx, Ne):
    got = ops.moe_assign_sorted(idx, Ne)
    want = M.moe_assign_sorted_reference(idx, Ne)
    for g, w, name in zip(got, want, ("slot", "src", "counts", "offsets", "tile_expert")):
        assert g.dtype == torch.int32 and g.shape == w.shape and torch.equal(g, w), name
    again = ops.moe_assign_sorted(idx, Ne)
    assert all(torch.equal(a, b) for a, b in zip(got, again))   # the same bits on every run
    T, kk = idx.shape
    assert got[1].shape == (ops.moe_sorted_rows(T, Ne, kk),)
    return got


@pytest.mark.parametrize("T,Ne,kk", [(193, 6, 2), (384, 4, 2), (65, 64, 2), (193, 128, 8), (63, 256, 8), (4100, 8, 2)])
def test_assign_sorted(k, T, Ne, kk):
    idx = ops.moe_route(_logits(T, Ne), kk)[0]
    slot, src, counts, offsets, tile_expert = _check_sorted(idx, Ne)
    assert int(counts.sum()) == T * kk and int((src >= 0).sum()) == T * kk and int((slot < 0).sum()) == 0
    a = torch.arange(T * kk, device=DEV, dtype=torch.int32).view(T, kk)
    assert torch.equal(src[slot.long()], a)
    # the same places as the capacity layout's, and its dispatch / combine take the tables as they are
    cap = T * kk
    slot_c = ops.moe_assign(idx, Ne, cap)[0]
    assert torch.equal(slot - offsets[idx.long()], slot_c - idx * cap)


def test_assign_sorted_one_expert_gets_every_token_and_one_gets_none(k):
    T, Ne = 1500, 6
    idx = torch.empty(T, 2, dtype=torch.int32, device=DEV)
    idx[:, 0] = 3
    idx[:, 1] = torch.arange(T, device=DEV) % 2 * 4      # experts 0 and 4; 1, 2 and 5 get nothing
    slot, src, counts, offsets, tile_expert = _check_sorted(idx, Ne)
    assert counts.tolist() == [750, 0, 0, 1500, 750, 0]
    assert offsets.tolist() == [0, 768, 768, 768, 2304, 3072, 3072]
    assert tile_expert.tolist()[:24] == [0] * 6 + [3] * 12 + [4] * 6 and (tile_expert[24:] == -1).all()
    assert (slot[:, 0] == 768 + torch.arange(T, device=DEV)).all()
    _check_sorted(idx[:1], Ne)
    _check_sorted(idx[:, :1].contiguous(), Ne)


def test_assign_sorted_counts_of_128_and_129_and_a_wild_index(k):
    idx = torch.cat([torch.full((128,), 1), torch.full((129,), 2), torch.full((3,), 0)]).to(torch.int32)
    idx = idx[torch.randperm(260, generator=torch.Generator().manual_seed(1))].view(260, 1).to(DEV)
    slot, src, counts, offsets, tile_expert = _check_sorted(idx, 4)
    assert counts.tolist() == [3, 128, 129, 0] and offsets.tolist() == [0, 128, 256, 512, 512]
    assert tile_expert.tolist()[:4] == [0, 1, 2, 2] and (tile_expert[4:] == -1).all()
    wild = idx.clone()
    wild[5, 0], wild[77, 0] = 9, -2
    slot, src, counts, offsets, tile_expert = _check_sorted(wild, 4)
    assert int((slot < 0).sum()) == 2 and slot[5, 0] == -1 and slot[77, 0] == -1 and int(counts.sum()) == 258


# ------------------------------------------------------------------ grouped GEMMs
COUNTS = {
    "five": [0, 1, 128, 129, 300],
    "two": [384, 0],
    "sparse256": [130 if e == 3 else 1 if e == 77 else 256 if e == 200 else 5 if e == 255 else 0 for e in range(256)],
}


def _layout(counts, dead=1):
    """(offsets, tile_expert, R, live row mask) of the sorted layout for these counts, with ``dead`` tiles past the
    end."""
    offs = [0]
    for c in counts:
        offs.append(offs[-1] + (c + 127) // 128 * 128)
    te = []
    for e in range(len(counts)):
        te += [e] * ((offs[e + 1] - offs[e]) // 128)
    te += [-1] * dead
    R = offs[-1] + 128 * dead
    live = torch.zeros(R, dtype=torch.bool)
    for e, c in enumerate(counts):
        live[offs[e]:offs[e] + c] = True
    return (torch.tensor(offs, dtype=torch.int32, device=DEV), torch.tensor(te, dtype=torch.int32, device=DEV), R,
            live.to(DEV))


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(BF).to(DEV)


def _ptrs(ts):
    return torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64).to(DEV)


def _assert_bf16_close(y, ref):
    err = (y.double() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 1e-3 * ref.abs().max()
    print("bf16 max err", err.max().item(), "max |ref|", ref.abs().max().item())
    assert (err <= bound).all(), (err - bound).max().item()


@pytest.mark.parametrize("N", [128, 384])
@pytest.mark.parametrize("Kred", [128, 192, 384])
@pytest.mark.parametrize("case", sorted(COUNTS))
def test_grouped_forward_and_dgrad(k, case, Kred, N):
    counts = COUNTS[case]
    Ne = len(counts)
    offsets, tile_expert, R, live = _layout(counts)
    offs = offsets.tolist()
    a = _rand((R, Kred), 1)
    for w_kc in (True, False):                    # forward: W_e [N, Kred]; dgrad: W_e [Kred, N]
        wall = _rand((Ne, N, Kred) if w_kc else (Ne, Kred, N), 2, Kred ** -0.5)
        ws = list(wall.unbind(0))
        y = k.grouped_gemm_rows(a, _ptrs(ws), tile_expert, N, w_kc)
        assert y.shape == (R, N) and y.dtype == BF
        assert (y[offs[-1]:] == 0).all()          # the dead tile is exactly zero
        zero = torch.zeros(1, dtype=torch.int32, device=DEV)
        for e in range(Ne):
            lo, hi = offs[e], offs[e + 1]
            if hi == lo:
                continue
            # the same kernel on this expert's rows alone: the same bits
            alone = k.grouped_gemm_rows(a[lo:hi], _ptrs(ws[e:e + 1]), zero.expand((hi - lo) // 128).contiguous(), N,
                                        w_kc)
            assert torch.equal(alone, y[lo:hi]), (e, w_kc)
            w = ws[e].double()
            _assert_bf16_close(y[lo:hi], a[lo:hi].double() @ (w.t() if w_kc else w))
        assert torch.equal(k.grouped_gemm_rows(a, _ptrs(ws), tile_expert, N, w_kc), y)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("N,K", [(128, 128), (384, 128), (128, 384)])
@pytest.mark.parametrize("case", sorted(COUNTS))
def test_grouped_wgrad(k, case, N, K, accumulate):
    counts = COUNTS[case]
    Ne = len(counts)
    offsets, tile_expert, R, live = _layout(counts)
    offs = offsets.tolist()
    x = _rand((R, K), 3) * live[:, None]          # the padding rows of x are zeros, those of dy are not
    dy = _rand((R, N), 4)
    start = torch.randn(Ne, N, K, generator=torch.Generator().manual_seed(5)).to(DEV)
    out = start.clone()
    outs = list(out.unbind(0))
    assert k.grouped_gemm_wgrad(dy, x, offsets, _ptrs(outs), accumulate) is None
    two = torch.zeros(2, dtype=torch.int32, device=DEV)
    for e in range(Ne):
        lo, hi = offs[e], offs[e + 1]
        if hi == lo:    # no rows: zeros after a store, untouched after an accumulation
            assert torch.equal(out[e], start[e] if accumulate else torch.zeros_like(start[e])), e
            continue
        alone = start[e].clone()
        two[1] = hi - lo
        k.grouped_gemm_wgrad(dy[lo:hi], x[lo:hi], two, _ptrs([alone]), accumulate)
        assert torch.equal(alone, out[e]), e       # the same kernel on this expert alone: the same bits
        ref = dy[lo:hi].double().t() @ x[lo:hi].double()
        got = out[e].double() - (start[e].double() if accumulate else 0.0)
        scale = ref.abs().max().item()
        err = (got - ref).abs().max().item()
        print("wgrad max err", err, "scale", scale)
        assert err <= 1e-3 * scale, (e, err, scale)
    if not accumulate:   # the table-free form writes the same bits into a fresh [Ne, N, K]
        assert torch.equal(k.grouped_gemm_wgrad(dy, x, offsets, None, False), out)


def test_grouped_refusals(k):
    offsets, tile_expert, R, _ = _layout([128, 1])
    a, w = _rand((R, 128), 1), _rand((2, 128, 128), 2)
    tab = _ptrs(list(w.unbind(0)))
    for bad in ((a[:100], tab, tile_expert, 128, True), (a, tab, tile_expert[:1], 128, True),
                (a, tab, tile_expert, 136, True), (a.float(), tab, tile_expert, 128, True),
                (a, tab.int(), tile_expert, 128, True), (a, tab.cpu(), tile_expert, 128, True),
                (_rand((R, 136), 1), tab, tile_expert, 128, True)):
        with pytest.raises(RuntimeError):
            k.grouped_gemm_rows(*bad)
    for bad in ((a, a[:128], offsets, None, False), (a, a, offsets, None, True), (a, a, offsets.long(), None, False),
                (a, a, offsets, tab[:1], False)):
        with pytest.raises(RuntimeError):
            k.grouped_gemm_wgrad(*bad)


def test_unsupported_width_runs_the_reference_and_warns_once(k):
    offsets, tile_expert, R, _ = _layout([100, 28])
    x = _rand((R, 136), 1)
    ws = [_rand((128, 136), 2 + e) for e in range(2)]
    GL._noted.clear()
    with pytest.warns(UserWarning, match="eager reference"):
        y = ops.grouped_linear(x, ws, tile_expert, offsets)
    assert torch.equal(y, ops.grouped_linear_reference(x, ws, tile_expert, offsets))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ops.grouped_linear(x, ws, tile_expert, offsets)


def test_grouped_linear_autograd_without_main_grad(k):
    """The op end to end on plain tensors: gradients returned in the weight dtype, against the eager reference."""
    offsets, tile_expert, R, live = _layout([130, 0, 7])
    x = (_rand((R, 256), 1) * live[:, None]).requires_grad_()
    ws = [_rand((128, 256), 2 + e, 1 / 16).requires_grad_() for e in range(3)]
    dy = _rand((R, 128), 9)
    ops.grouped_linear(x, ws, tile_expert, offsets).backward(dy)
    xr = x.detach().float().requires_grad_()
    wr = [w.detach().float().requires_grad_() for w in ws]
    ops.grouped_linear_reference(xr, wr, tile_expert, offsets).backward(dy.float())
    _assert_bf16_close(x.grad[live], xr.grad[live].double())
    for w, r in zip(ws, wr):
        assert w.grad.dtype == BF
        assert (w.grad.double() - r.grad.double()).abs().max() <= (2.0 ** -8 + 1e-3) * r.grad.abs().max() + 1e-30
    assert (ws[1].grad == 0).all()


# ------------------------------------------------------------------ the block
D_MODEL, FF, NE, TOPK = 256, 512, 4, 2


def _rows(n, E, seed):
    return _rand((n, E), seed)


def _skewed_block():
    torch.manual_seed(0)
    blk = MoEFeedForwardBlock(D_MODEL, FF, NE, TOPK, capacity_factor=None, expert_gemm="grouped")
    blk = blk.to(DEV, BF).train()
    with torch.no_grad():
        blk.router_weight.normal_(std=0.3)
        blk.router_weight += (torch.linspace(-1, 1, NE)[:, None] * 0.02).to(DEV, BF)
    return blk


def _skewed_input(seed):
    return (_rows(384, D_MODEL, seed) + 1.0).view(2, 192, D_MODEL)


def _reference_forward(blk, logits, x2, xr2):
    """The grouped forward after the router GEMM on the REFERENCE ops (the gate kernel is the block's own)."""
    tokens = x2.shape[0]
    idx, gate, probs_sum = M.moe_route_reference(logits, TOPK)
    slot, src, counts, offsets, tile_expert = M.moe_assign_sorted_reference(idx, NE)
    dprobs = counts.float() * (blk.aux_coef * blk.aux_scale * NE / (float(tokens) * tokens * TOPK))
    gate = ops.moe_attach_aux(gate, probs_sum, dprobs)
    xe = M.moe_dispatch_reference(x2, slot, src)
    h = ops.swiglu(ops.grouped_linear_reference(xe, list(blk.experts_w1), tile_expert, offsets))
    ye = ops.grouped_linear_reference(h, list(blk.experts_w2), tile_expert, offsets)
    return M.moe_combine_reference(ye, gate, slot, src, xr2), counts


def test_block_grouped_against_reference_ops(k):
    blk = _skewed_block()
    opt = FlatAdam(blk.parameters(), lr=1e-3)
    x = _skewed_input(8).requires_grad_()
    dy = _rows(384, D_MODEL, 9)
    xn = ops.add_dropout_rms_norm(x, None, blk.norm_weight, blk.eps, 0.0, True).reshape(-1, D_MODEL)
    logits = ops.linear(xn, blk.router_weight)        # ONE router GEMM: both paths route the same logits
    xr2 = x.reshape(-1, D_MODEL)

    gate, slot, src, (offsets, tile_expert) = blk.route(logits, 384)
    y = ops.moe_combine(blk.experts_grouped(ops.moe_dispatch(xn, slot, src), offsets, tile_expert), gate, slot, src,
                        residual=xr2)
    y_ref, counts = _reference_forward(blk, logits, xn, xr2)
    assert float(blk.last_drop_fraction) == 0.0 and int((slot < 0).sum()) == 0
    assert counts.max().item() > 1.5 * counts.min().item()     # the router is skewed

    def grads(out):
        opt.zero_grad()
        x.grad = None
        out.backward(dy, retain_graph=True)
        opt.fold_grads()
        torch.cuda.synchronize()
        return x.grad.clone(), {n: p.main_grad.clone() for n, p in blk.named_parameters()}

    gx, gp = grads(y)
    rx, rp = grads(y_ref)
    atol, rtol = _tol(BF)
    assert torch.allclose(y.float(), y_ref.float(), atol=atol, rtol=rtol)
    assert torch.allclose(gx.float(), rx.float(), atol=atol * 5, rtol=rtol * 5)
    assert gp.keys() == rp.keys() and len(gp) == 2 + 2 * NE
    for n, g in gp.items():
        assert (g - rp[n]).abs().max().item() <= 2e-2 * (rp[n].abs().max().item() + 1e-6), n
        assert (g != 0).any(), n
    # and the whole forward is those pieces
    assert torch.equal(blk(x.detach()).view(-1, D_MODEL), y.detach())


def test_block_grouped_checkpoint_and_deferred_wgrad_bit_exact(k):
    blk = _skewed_block()
    opt = FlatAdam(blk.parameters(), lr=1e-3)
    base = _skewed_input(10)
    dy = _rows(384, D_MODEL, 11).view(2, 192, D_MODEL)

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
    assert all((t != 0).any() for t in plain) and float(blk.last_drop_fraction) == 0.0
    for other in (run(ckpt=True), run(deferred=True), run()):
        assert all(torch.equal(a, b) for a, b in zip(plain, other))


def test_block_grouped_accumulates_over_micro_batches(k):
    """Two backwards between two zero_grads: the second accumulates into every expert's main_grad."""
    blk = _skewed_block()
    opt = FlatAdam(blk.parameters(), lr=1e-3)
    xs = [_skewed_input(12), _skewed_input(13)]
    dy = _rows(384, D_MODEL, 14).view(2, 192, D_MODEL)

    def run(inputs):
        opt.zero_grad()
        for x in inputs:
            blk(x).backward(dy)
        opt.fold_grads()
        torch.cuda.synchronize()
        return [p.main_grad.clone() for n, p in blk.named_parameters() if n.startswith("experts_")]

    one, two, both = run(xs[:1]), run(xs[1:]), run(xs)
    assert len(both) == 2 * NE
    for a, b, c in zip(one, two, both):   # one fp32 rounding of the sum apart
        assert (c - (a + b)).abs().max().item() <= 2.0 ** -22 * c.abs().max().item()


# ------------------------------------------------------------------ the model
def _cfg():
    return dataclasses.replace(CONFIGS["moe_tiny"], expert_gemm="grouped", capacity_factor=None)


def _data(cfg, n, seed=7):
    tok = torch.randint(0, cfg.vocab, (n, cfg.seq_len + 1), generator=torch.Generator().manual_seed(seed))
    return tok[:, :-1].to(DEV), tok[:, 1:].contiguous().to(DEV)


def _loss(cfg, model, x, t):
    return ops.cross_entropy(model(x).reshape(-1, cfg.vocab), t.reshape(-1))


def test_moe_tiny_grouped_step_against_the_eager_model(k, monkeypatch):
    """test_moe_tiny_step_against_the_eager_model with the grouped experts: one forward-backward in bf16 through the
    kernels against the same weights in fp32 on the eager references (CPU), the routing pinned to the bf16 model's
    choices."""
    cfg = _cfg()
    torch.manual_seed(0)
    blocks = build_lm_blocks(cfg, dtype=BF)
    model = torch.nn.Sequential(*copy.deepcopy(blocks)).to(DEV).train()
    moes = [b for b in model if isinstance(b, MoEFeedForwardBlock)]
    assert len(moes) == 2 and all(b.expert_gemm == "grouped" for b in moes)
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
    assert len(chosen) == 2 and all(float(b.last_drop_fraction) == 0.0 for b in moes)
    monkeypatch.setattr(ops, "moe_route", replay)
    ref = torch.nn.Sequential(*copy.deepcopy(blocks)).float().train()
    ref_loss = _loss(cfg, ref, x.cpu(), t.cpu())
    ref_loss.backward()
    assert len(flips) == 2 and not chosen and max(flips) < 0.05, flips
    ref_grads = {n: p.grad for n, p in ref.named_parameters()}
    _assert_model_close(float(loss.detach()), grads, float(ref_loss.detach()), ref_grads)


def test_moe_tiny_grouped_training_is_deterministic(k):
    cfg = _cfg()
    x, t = _data(cfg, 2)

    def run():
        torch.manual_seed(0)
        model = torch.nn.Sequential(*build_lm_blocks(cfg, dtype=BF)).to(DEV).train()
        opt = FlatAdam(model.parameters(), lr=1e-3)
        losses = []
        for _ in range(3):
            opt.zero_grad()
            loss = _loss(cfg, model, x, t)
            loss.backward()
            opt.step(opt.grad_sumsq())
            losses.append(loss.detach().clone())
        torch.cuda.synchronize()
        return torch.stack(losses)

    a, b = run(), run()
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert a[2] < a[0]
