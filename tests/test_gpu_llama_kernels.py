"""The LLaMA-style block's HIP kernels on one MI355X: RMSNorm (rmsnorm.hip),
SwiGLU and RoPE (llama.hip) against fp64 references at their dispatch edges,
with exact Philox dropout masks, and the ``llama_tiny`` model end to end.

Tolerances are those of tests/helpers/rowwise_cases.py; every kernel comes
from mipipe/_C.so: the tests fail if the extension is missing."""
import copy
import dataclasses

import pytest
import torch

from helpers.rowwise_cases import (BF16_REL, assert_close, assert_close_slack, assert_reduction, ln_inputs)
from test_gpu_pipeline import _assert_same_grad, _note_embeddings
from test_gpu_rowwise_edges import LN_SHAPES, keep8

from mipipe import Pipe, ops
from mipipe.models import CONFIGS, build_lm_blocks
from mipipe.optim import FlatAdam

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
EPS = 1e-5


@pytest.fixture(scope="module")
def k():
    from mipipe._native_loader import kernels

    return kernels()


def _all_zero(t):
    return bool((t == 0).all().item())


# ------------------------------------------------------------------ 1. RMSNorm
def rms_reference(x, res, w, eps, dy, keep=None, p=0.0):
    """fp64 RMSNorm(res + x * keep / (1 - p)) of the tensors as given (already
    rounded to the kernel's dtype), and its gradients for the output gradient dy."""
    xd = x.detach().double().requires_grad_()
    rd = res.detach().double().requires_grad_() if res is not None else None
    wd = w.detach().double().requires_grad_()
    h = xd
    if keep is not None:
        h = h * keep.to(h.device).double() / (1.0 - p)
    z = h + rd if rd is not None else h
    rstd = (z.pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    y = z * rstd * wd
    y.backward(dy.detach().double())
    return {"y": y.detach(), "z": z.detach(), "rstd": rstd.detach().squeeze(-1), "dx": xd.grad,
            "dres": rd.grad if rd is not None else None, "dw": wd.grad}


def rms_saved_z_slack(z, w, dy, eps):
    """Extra error allowed in the bf16 backward WITH a residual or dropout, as (dz, dgamma).

    The forward normalises the fp32 sum z = res + x but saves it for the
    backward rounded to bf16, so the backward sees xhat = z rstd (rstd is the
    forward's, from the unrounded z) off by up to |dxh| = 2**-8 |z| rstd (half a
    bf16 ulp of z is at most 2**-8 |z|).  Propagated to first order through
        dz = rstd (gy - xhat mean(gy xhat)),  dgamma = sum_rows dy xhat
    with gy = dy gamma, in fp64 from the inputs (never from a kernel's output):
        |d dz|     <= rstd (|dxh| |mean(gy xhat)| + |xhat| mean(|gy| |dxh|))
        |d dgamma| <= sum_rows |dy| |dxh|
    This is ln_saved_z_slack without the mean: RMSNorm has no centring term."""
    z, gy, dy = z.double(), dy.double() * w.double(), dy.double()
    rstd = (z.pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    xh = z * rstd
    dxh = BF16_REL * z.abs() * rstd
    dz = rstd * (dxh * (gy * xh).mean(-1, keepdim=True).abs() + xh.abs() * (gy.abs() * dxh).mean(-1, keepdim=True))
    dg = (dy.abs() * dxh).sum(0)
    return dz, dg


def check_rmsnorm(cols, rows, dtype, residual, offset=0.0):
    """add_dropout_rms_norm (p = 0) forward and backward against fp64."""
    x, res, w, _, dy = ln_inputs(rows, cols, dtype, residual, offset)
    ref = rms_reference(x, res, w, EPS, dy)
    xs = x.clone().requires_grad_()
    rs = res.clone().requires_grad_() if residual else None
    ws = w.clone().requires_grad_()
    y = ops.add_dropout_rms_norm(xs, rs, ws, EPS, 0.0, True)
    tag = f"rmsnorm {rows}x{cols} {dtype} residual={residual}"
    assert_close(y, ref["y"], dtype, tag + " y")
    y.backward(dy)
    if dtype == torch.float32:
        assert_close(xs.grad, ref["dx"], dtype, tag + " dx")
        if residual:
            assert_close(rs.grad, ref["dres"], dtype, tag + " dresidual")
        assert_reduction(ws.grad, ref["dw"], tag + " dgamma")
    elif not residual:  # the backward reads x itself: no rounded copy in between
        assert_close(xs.grad, ref["dx"], dtype, tag + " dx")
        assert_close(ws.grad, ref["dw"], dtype, tag + " dgamma")
    else:
        s_dz, s_dg = rms_saved_z_slack(ref["z"], w, dy, EPS)
        assert_close_slack(xs.grad, ref["dx"], s_dz, tag + " dx")
        assert_close_slack(rs.grad, ref["dres"], s_dz, tag + " dresidual")
        assert_close_slack(ws.grad, ref["dw"], s_dg, tag + " dgamma")


# The dispatch is LayerNorm's (cols <= 2048: wave per row; <= 4096: 2 vectors per
# thread, two-row blocks; <= 8192: 4; <= 16384: 8), so LN_SHAPES meets every kernel
# and both sides of 2048 | 2056 and 8192 | 8200; 4096 is the near side of 4096 | 4104.
RMS_SHAPES = LN_SHAPES + [(4096, 67)]


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cols,rows", RMS_SHAPES)
def test_rmsnorm_dispatch_edges(k, cols, rows, dtype, residual):
    check_rmsnorm(cols, rows, dtype, residual)


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("cols", [1024, 4096, 8192])
def test_rmsnorm_offset_inputs(k, cols, residual):
    """x = 100 + randn in fp32.  RMSNorm has no mean to cancel against: this
    checks the sum of z^2 (about 1e4 per element, 8e7 per row) for overflow and
    for precision -- every term is positive, so the fp32 sum stays within a few
    ulp relative and the fp32 tolerance holds."""
    check_rmsnorm(cols, 33, torch.float32, residual, offset=100.0)


@pytest.mark.parametrize("cols", [12, 2052, 16392])
def test_rmsnorm_rejects_width(k, cols):
    """Widths that are no multiple of 8, and 16392 (> 8 vectors per thread)."""
    x = torch.randn(3, cols, device=DEV)
    w = torch.ones(cols, device=DEV)
    with pytest.raises(RuntimeError):
        k.rmsnorm_fwd(x, None, w, EPS, 0.0, False)
    with pytest.raises(RuntimeError):
        k.rmsnorm_bwd(x, x, torch.ones(3, device=DEV), w, 0.0, 0, 0)
    with pytest.raises(RuntimeError):
        ops.add_dropout_rms_norm(x, None, w)


@pytest.mark.parametrize("dtype", DTYPES)
def test_rmsnorm_zero_rows(k, dtype):
    x = torch.empty(0, 64, device=DEV, dtype=dtype)
    w = torch.ones(64, device=DEV, dtype=dtype)
    y, z, rstd, _, _ = k.rmsnorm_fwd(x, x, w, EPS, 0.0, True)
    assert y.shape == (0, 64) and z.shape == (0, 64) and rstd.shape == (0,)
    dz, dx, dg = k.rmsnorm_bwd(x, x, rstd, w, 0.0, 0, 0)
    assert dz.shape == (0, 64) and dx is None and _all_zero(dg) and dg.shape == (64,)
    xs, ws = x.clone().requires_grad_(), w.clone().requires_grad_()
    out = ops.add_dropout_rms_norm(xs, None, ws)
    out.sum().backward()
    assert out.shape == (0, 64) and xs.grad.shape == (0, 64) and _all_zero(ws.grad)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cols,p", [(1600, 0.25), (4096, 0.1)])
def test_rmsnorm_dropout_exact_mask(k, cols, p, dtype):
    """Forward and backward regenerate the same documented keep8 mask: the zeros
    of z - res and of dx sit exactly where keep8 drops, and y, z, rstd, dz, dx,
    dgamma match the fp64 reference of res + x * keep / (1 - p).  |x| >= 1 here,
    so a kept x / (1 - p) is never lost in the rounding of res + x / (1 - p) (a
    bf16 sum below 16 has half an ulp of at most 2**-5) and never 0 itself."""
    rows = 37
    x, res, w, _, dy = ln_inputs(rows, cols, dtype, True)
    x = torch.where(x >= 0, x.float() + 1, x.float() - 1).to(dtype)
    y, z, rstd, seed, offset = k.rmsnorm_fwd(x, res, w, EPS, p, True)
    keep = keep8(rows * cols, p, seed, offset).view(rows, cols).to(DEV)
    assert abs(keep.float().mean().item() - (1 - p)) < 0.01
    assert torch.equal((z.float() - res.float()) == 0, ~keep)
    ref = rms_reference(x, res, w, EPS, dy, keep, p)
    assert_close(z, ref["z"], dtype, "z")
    assert_close(y, ref["y"], dtype, "y")
    assert_close(rstd, ref["rstd"], torch.float32, "rstd")
    dz, dx, dg = k.rmsnorm_bwd(dy, z, rstd, w, p, seed, offset)
    assert torch.equal(dx == 0, ~keep)
    if dtype == torch.float32:
        assert_close(dz, ref["dres"], dtype, "dz")
        assert_close(dx, ref["dx"], dtype, "dx")
        assert_reduction(dg, ref["dw"], "dgamma")
    else:
        s_dz, s_dg = rms_saved_z_slack(ref["z"], w, dy, EPS)
        assert_close_slack(dz, ref["dres"], s_dz, "dz")
        assert_close_slack(dx, ref["dx"], s_dz / (1 - p), "dx")
        assert_close_slack(dg, ref["dw"], s_dg, "dgamma")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cols,rows", [(1600, 300), (4096, 300)])
def test_rmsnorm_main_grad_accumulation(k, cols, rows, dtype):
    """weight.main_grad (fp32): the first backward after _mg_fresh = True
    overwrites the stale 7.0s, the second accumulates; weight.grad stays None."""
    x, _, w, _, dy = ln_inputs(rows, cols, dtype, False)
    dy2 = torch.randn(rows, cols, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5)).to(dtype)
    ref1 = rms_reference(x, None, w, EPS, dy)["dw"]
    ref2 = rms_reference(x, None, w, EPS, dy2)["dw"]
    ws = w.clone().requires_grad_()
    ws.main_grad = torch.full((cols,), 7.0, device=DEV)
    ws._mg_fresh = True
    ops.add_dropout_rms_norm(x.clone().requires_grad_(), None, ws, EPS).backward(dy)
    assert_reduction(ws.main_grad, ref1, "main_grad after the first backward")
    ops.add_dropout_rms_norm(x.clone().requires_grad_(), None, ws, EPS).backward(dy2)
    assert_reduction(ws.main_grad, ref1 + ref2, "main_grad after the second backward")
    assert ws.grad is None
    # the binding itself: prefill + column sums, nothing returned for dgamma
    _, _, rstd, _, _ = k.rmsnorm_fwd(x, None, w, EPS, 0.0, False)
    pre = 1 + 3 * torch.randn(cols, device=DEV)
    acc = pre.clone()
    dz, dx, dg = k.rmsnorm_bwd(dy, x, rstd, w, 0.0, 0, 0, acc)
    assert dg is None and dx is None
    assert_reduction(acc, pre.double() + ref1, "acc_gamma")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cols", [1600, 4096])
def test_rmsnorm_fanout(k, cols, dtype):
    """rms_norm_fanout adds the other consumer's gradient inside the backward
    kernel.  Asserted: the fused dx is within the dtype's bound of the fp64
    dx + dfan (fp32 too: the kernel's rstd * (..) + addend contracts to an fma, so
    it is not bit-equal to the two-kernel sum), and within that bound plus the
    roundings of the non-fused path (its separately stored dx and its own sum, bf16);
    dgamma is the same bits on both paths (the addend does not enter it)."""
    rows = 67
    x, _, w, _, dy = ln_inputs(rows, cols, dtype, False)
    dfan = torch.randn(rows, cols, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)).to(dtype)
    ref = rms_reference(x, None, w, EPS, dy)
    xs, ws = x.clone().requires_grad_(), w.clone().requires_grad_()
    y, xr = ops.rms_norm_fanout(xs, ws, EPS)
    assert xr.data_ptr() == xs.data_ptr()
    torch.autograd.backward([y, xr], [dy, dfan])
    assert_close(xs.grad, ref["dx"] + dfan.double(), dtype, "fused dx + dfan")
    x2, w2 = x.clone().requires_grad_(), w.clone().requires_grad_()
    y2 = ops.add_dropout_rms_norm(x2, None, w2, EPS)
    assert torch.equal(y2, y)
    torch.autograd.backward([y2, x2 * 1], [dy, dfan])
    if dtype == torch.float32:
        assert_close(xs.grad, x2.grad.double(), dtype, "fused against non-fused")
    else:
        # three roundings separate the two bf16 results, each at most half an ulp <= 2**-8 |value|: the
        # fused sum's and the non-fused sum's (one is in assert_close_slack's own bound) and the stored dx's
        total = ref["dx"] + dfan.double()
        assert_close_slack(xs.grad, x2.grad.double(), BF16_REL * (ref["dx"].abs() + total.abs()),
                           "fused against non-fused")
    assert torch.equal(ws.grad, w2.grad)
    # only the fan-out branch carries a gradient
    xs2 = x.clone().requires_grad_()
    _, xr2 = ops.rms_norm_fanout(xs2, w.clone().requires_grad_(), EPS)
    xr2.backward(dfan)
    assert torch.equal(xs2.grad, dfan)


# ------------------------------------------------------------------ 2. SwiGLU
# (4100, 2056): 1,053,700 16-byte items, more than the 2048 x 256 x 2 one trip of the grid covers
SWIGLU_SHAPES = [(1, 8), (7, 8), (67, 2056), (1100, 1504), (3, 16384), (4100, 2056)]


def _swiglu_ref(gu, dh):
    gd = gu.detach().double().requires_grad_()
    h = ops.swiglu_reference(gd)
    h.backward(dh.detach().double())
    return h.detach(), gd.grad


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,F", SWIGLU_SHAPES)
def test_swiglu_against_fp64(k, rows, F, dtype):
    """Gates over [-30, 30] (the sigmoid saturates on both sides), exact zeros in
    gate, up and dh, and one -inf gate: h = 0 there and dgu is what the fp64
    reference gives (0 for both halves)."""
    g = torch.Generator(device=DEV).manual_seed(rows * 31 + F)
    gate = torch.rand(rows, F, device=DEV, generator=g) * 60 - 30
    gate[0, :8] = torch.tensor([-30.0, 30.0, 0.0, -0.0, 1e-3, -20.0, 20.0, 0.5], device=DEV)
    up = torch.randn(rows, F, device=DEV, generator=g)
    dh = torch.randn(rows, F, device=DEV, generator=g)
    up[0, 1], dh[0, 4] = 0.0, 0.0
    gate[-1, -1] = float("-inf")
    gu = torch.cat((gate, up), dim=1).to(dtype)
    dh = dh.to(dtype)
    ref_h, ref_dgu = _swiglu_ref(gu, dh)
    assert torch.isfinite(ref_h).all() and torch.isfinite(ref_dgu).all()
    gs = gu.clone().requires_grad_()
    h = ops.swiglu(gs)
    tag = f"swiglu {rows}x{F} {dtype}"
    assert h.shape == (rows, F)
    assert_close(h, ref_h, dtype, tag + " h")
    h.backward(dh)
    assert gs.grad.shape == (rows, 2 * F)
    assert_close(gs.grad, ref_dgu, dtype, tag + " dgu")
    assert h[-1, -1].item() == 0.0 and gs.grad[-1, F - 1].item() == 0.0 and gs.grad[-1, -1].item() == 0.0
    assert h[0, 1].item() == 0.0 and gs.grad[0, 4].item() == 0.0 and gs.grad[0, F + 4].item() == 0.0


def test_swiglu_rejects_and_empty(k):
    with pytest.raises(RuntimeError):
        k.swiglu_fwd(torch.randn(3, 24, device=DEV))  # F = 12
    with pytest.raises(RuntimeError):
        k.swiglu_bwd(torch.randn(3, 8, device=DEV), torch.randn(3, 32, device=DEV))  # dh is not [rows, F]
    h = k.swiglu_fwd(torch.empty(0, 32, device=DEV))
    assert h.shape == (0, 16)
    assert k.swiglu_bwd(h, torch.empty(0, 32, device=DEV)).shape == (0, 32)


# ------------------------------------------------------------------ 3. RoPE
ROPE_CASES = [(1, 1, 1, 16, 0), (2, 64, 4, 64, 0), (1, 130, 3, 128, 7), (2, 8, 2, 256, 0)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,S,H,D,pos0", ROPE_CASES)
def test_rope_against_fp64(k, B, S, H, D, pos0, dtype):
    """Forward against the fp64 rotation by the same fp32 tables, V bit-identical;
    the backward is the inverse rotation of the gradient (V's passes through);
    the in-place variant gives the same bits as the out-of-place one."""
    g = torch.Generator(device=DEV).manual_seed(S * 7 + D)
    qkv = torch.randn(B, S, 3, H, D, device=DEV, generator=g).to(dtype)
    grad = torch.randn(B, S, 3, H, D, device=DEV, generator=g).to(dtype)
    cos, sin = ops.rope_tables(pos0 + S + 3, D, device=DEV)
    ref = ops.rope_reference(qkv.double(), cos, sin, pos0)
    qs = qkv.clone().requires_grad_()
    out = ops.rope_packed(qs, cos, sin, pos0)
    tag = f"rope {B}x{S}x{H}x{D} pos0={pos0} {dtype}"
    assert out.data_ptr() != qs.data_ptr() and torch.equal(qs.detach(), qkv)
    assert_close(out, ref, dtype, tag)
    assert torch.equal(out[:, :, 2], qkv[:, :, 2])
    out.backward(grad)
    assert_close(qs.grad, ops.rope_reference(grad.double(), cos, sin, pos0, inverse=True), dtype, tag + " backward")
    assert torch.equal(qs.grad[:, :, 2], grad[:, :, 2])
    # in place: the same bits, in the argument's own storage
    buf = qkv.clone()
    same = ops.rope_packed(buf, cos, sin, pos0, inplace=True)
    assert same.data_ptr() == buf.data_ptr() and torch.equal(same, out)
    # in place below an autograd node (the models' use: the projection's output)
    leaf = qkv.clone().requires_grad_()
    out2 = ops.rope_packed(leaf * 1, cos, sin, pos0, inplace=True)
    out2.backward(grad)
    assert torch.equal(out2, out) and torch.equal(leaf.grad, qs.grad)


def test_rope_rejects(k):
    cos, sin = ops.rope_tables(8, 24, device=DEV)
    with pytest.raises(RuntimeError):  # D = 24
        k.rope_packed(torch.randn(1, 4, 3, 2, 24, device=DEV), cos, sin)
    cos, sin = ops.rope_tables(8, 32, device=DEV)
    qkv = torch.randn(1, 8, 3, 2, 32, device=DEV)
    with pytest.raises(RuntimeError):  # tables end at position 8
        k.rope_packed(qkv, cos, sin, None, 1)
    with pytest.raises(RuntimeError):  # bf16 tables
        k.rope_packed(qkv, cos.bfloat16(), sin.bfloat16())
    with pytest.raises(RuntimeError):  # not [B, S, 3, H, D]
        k.rope_packed(qkv[:, :, :2].contiguous(), cos, sin)
    assert k.rope_packed(qkv[:, :0].contiguous(), cos, sin).shape == (1, 0, 3, 2, 32)


# ------------------------------------------------------------------ 4. the model
def _cfg(**kw):
    return dataclasses.replace(CONFIGS["llama_tiny"], **kw)


def _data(cfg, n, seed=7):
    tok = torch.randint(0, cfg.vocab, (n, cfg.seq_len + 1), generator=torch.Generator().manual_seed(seed))
    return tok[:, :-1], tok[:, 1:].contiguous()


def _loss_fn(cfg):
    return lambda y, t: ops.cross_entropy(y.reshape(-1, cfg.vocab), t.reshape(-1))


def _assert_model_close(loss, grads, ref_loss, ref_grads):
    """run_engine_case's GPU rule: loss 2e-3 relative, each gradient 2e-2 of its max."""
    assert abs(loss - ref_loss) < 2e-3 * abs(ref_loss), (loss, ref_loss)
    assert grads.keys() == ref_grads.keys()
    for n, g in grads.items():
        r = ref_grads[n].float().cpu()
        assert (g.float().cpu() - r).abs().max().item() <= 2e-2 * (r.abs().max().item() + 1e-6), n


def _gpu_step(model, cfg, x, t):
    opt = FlatAdam(model.parameters(), lr=1e-3)
    opt.zero_grad()
    loss = _loss_fn(cfg)(model(x.to(DEV)), t.to(DEV))
    loss.backward()
    opt.fold_grads()
    torch.cuda.synchronize()
    return float(loss.detach()), {n: p.main_grad.clone() for n, p in model.named_parameters()}


@pytest.fixture(scope="module")
def llama_unpipelined():
    """llama_tiny in bf16 on the GPU, one unpipelined step: (blocks as built, loss, gradients)."""
    cfg = _cfg()
    torch.manual_seed(0)
    blocks = build_lm_blocks(cfg, dtype=torch.bfloat16)
    model = torch.nn.Sequential(*copy.deepcopy(blocks)).to(DEV).train()
    x, t = _data(cfg, 8)
    loss, grads = _gpu_step(model, cfg, x, t)
    return blocks, loss, grads


def test_llama_tiny_bf16_matches_cpu_fp32(k, llama_unpipelined):
    """The HIP-kernel model against the same (bf16-rounded) weights on the CPU
    eager path in fp32."""
    cfg = _cfg()
    blocks, loss, grads = llama_unpipelined
    ref = torch.nn.Sequential(*copy.deepcopy(blocks)).float().train()
    x, t = _data(cfg, 8)
    ref_loss = _loss_fn(cfg)(ref(x), t)
    ref_loss.backward()
    _assert_model_close(loss, grads, float(ref_loss.detach()), {n: p.grad for n, p in ref.named_parameters()})


@pytest.mark.parametrize("checkpoint", ["never", "except_last", "always"])
def test_llama_tiny_pipe_two_partitions(k, llama_unpipelined, checkpoint):
    cfg = _cfg()
    blocks, ref_loss, ref_grads = llama_unpipelined
    blocks = copy.deepcopy(blocks)
    model = torch.nn.Sequential(*blocks).to(DEV).train()
    opt = FlatAdam(model.parameters(), lr=1e-3)
    pipe = Pipe(model, chunks=4, checkpoint=checkpoint, balance=[3, len(blocks) - 3], copy_same_device=True)
    x, t = _data(cfg, 8)
    try:
        assert len(pipe.partitions) == 2
        opt.zero_grad()
        loss = _loss_fn(cfg)(pipe(x.to(DEV)).local_value(), t.to(DEV))
        loss.backward()
        opt.fold_grads()
        torch.cuda.synchronize()
    finally:
        pipe.close()
    _assert_model_close(float(loss.detach()), {n: p.main_grad for n, p in model.named_parameters()}, ref_loss,
                        ref_grads)


def _pipe_grads(checkpoint, cfg, seed=99):
    torch.manual_seed(0)
    blocks = build_lm_blocks(cfg, dtype=torch.bfloat16)
    model = torch.nn.Sequential(*blocks).to(DEV).train()
    opt = FlatAdam(model.parameters(), lr=1e-3)
    pipe = Pipe(model, chunks=4, checkpoint=checkpoint, balance=[3, len(blocks) - 3], copy_same_device=True)
    x, t = _data(cfg, 8)
    try:
        opt.zero_grad()
        torch.manual_seed(seed)
        loss = _loss_fn(cfg)(pipe(x.to(DEV)).local_value(), t.to(DEV))
        loss.backward()
        opt.fold_grads()
        torch.cuda.synchronize()
    finally:
        pipe.close()
    _note_embeddings(model)
    return float(loss.detach()), {n: p.main_grad.clone() for n, p in model.named_parameters()}


def test_llama_rms_post_norm_recompute_bit_identical_with_dropout(k):
    """Post-norm with norm="rms" and dropout 0.1 (embedding, attention, and the
    RMSNorm kernels' own residual dropout): 'always' and 'except_last' regenerate
    the same Philox masks, so their gradients equal 'never' bit for bit."""
    cfg = _cfg(dropout=0.1, norm_first=False)
    loss0, g0 = _pipe_grads("never", cfg)
    _, g_other = _pipe_grads("never", cfg, seed=100)
    assert any(not torch.equal(g0[n], g_other[n]) for n in g0)
    for mode in ("except_last", "always"):
        loss, g = _pipe_grads(mode, cfg)
        assert loss == loss0, mode
        for n in g0:
            _assert_same_grad(g[n], g0[n], n, mode)
