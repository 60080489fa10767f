"""The Gemma-2 block's HIP kernels on the GPU: GeGLU (csrc/kernels/llama.hip) and the sandwich norm
``residual + RMSNorm(x) * weight`` (the POST variants of rmsnorm.hip's forward kernels, and the
existing backward kernels behind it) against fp64 at their dispatch edges, the bindings' refusals,
and the ``gemma2_block_tiny`` model: against the CPU, through ``Pipe`` with the cut between a
decoupled attention core and its output, and through the engine.  The kernels come from
mipipe/_C.so: the tests fail if the extension is missing.

The references are fp64 math on the tensors as given (already rounded to the kernel's dtype); the
bounds are the project's own (helpers/rowwise_cases.py).  Both kernels compute in fp32 and round
once at the store, and the norm's backward reads x itself (the GEMM output, saved as it is), so no
extra term is needed: bf16 dx and dgamma are held to the plain bf16 bound."""
import copy

import pytest
import torch

from helpers.rowwise_cases import assert_close, assert_reduction, ln_inputs
from test_gpu_llama_kernels import _assert_model_close, _data, _gpu_step, _loss_fn
from test_gpu_pipeline import _assert_same_grad, _note_embeddings
from test_gpu_rowwise_edges import LN_SHAPES

from mipipe import Pipe, ops
from mipipe.models import CONFIGS, build_lm_blocks
from mipipe.models.transformer import PackedAttentionCore, PackedAttentionOutput, pipeline_units
from mipipe.optim import FlatAdam
from mipipe.parallel import PipelineEngine

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


# ------------------------------------------------------------------ 1. GeGLU
# (4100, 2056): 1,053,700 16-byte items, more than the 2048 x 256 x 2 one trip of the grid covers
GEGLU_SHAPES = [(1, 8), (7, 8), (67, 2056), (3, 16384), (4100, 2056)]


def _geglu_ref(gu, dh):
    gd = gu.detach().double().requires_grad_()
    h = ops.geglu_reference(gd)  # tied to the written-out formula in test_gemma2_ops.py
    h.backward(dh.detach().double())
    return h.detach(), gd.grad


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,F", GEGLU_SHAPES)
def test_geglu_against_fp64(k, rows, F, dtype):
    """Gates over [-30, 30] (s = 0.5 (1 + tanh) saturates on both sides, and exp(-2a) overflows below about
    -10), exact zeros in gate, up and dh, and one -inf gate: h = 0 there and dgu is what the fp64 reference
    gives (0 for both halves)."""
    g = torch.Generator(device=DEV).manual_seed(rows * 31 + F)
    gate = torch.rand(rows, F, device=DEV, generator=g) * 60 - 30
    gate[0, :8] = torch.tensor([-30.0, 30.0, 0.0, -0.0, 1e-3, -20.0, 20.0, 0.5], device=DEV)
    up = torch.randn(rows, F, device=DEV, generator=g)
    dh = torch.randn(rows, F, device=DEV, generator=g)
    up[0, 1], dh[0, 4] = 0.0, 0.0
    gate[-1, -1] = float("-inf")
    gu = torch.cat((gate, up), dim=1).to(dtype)
    dh = dh.to(dtype)
    ref_h, ref_dgu = _geglu_ref(gu, dh)
    assert torch.isfinite(ref_h).all() and torch.isfinite(ref_dgu).all()
    gs = gu.clone().requires_grad_()
    h = ops.geglu(gs)
    tag = f"geglu {rows}x{F} {dtype}"
    assert h.shape == (rows, F)
    assert_close(h, ref_h, dtype, tag + " h")
    h.backward(dh)
    assert gs.grad.shape == (rows, 2 * F)
    assert_close(gs.grad, ref_dgu, dtype, tag + " dgu")
    assert h[-1, -1].item() == 0.0 and gs.grad[-1, F - 1].item() == 0.0 and gs.grad[-1, -1].item() == 0.0
    assert h[0, 1].item() == 0.0 and gs.grad[0, 4].item() == 0.0 and gs.grad[0, F + 4].item() == 0.0
    # exp overflowed at the gate of -30: s = 0, h = 0 and dg = 0 exactly (du = dh gelu(g) = 0 as well)
    assert h[0, 0].item() == 0.0 and gs.grad[0, 0].item() == 0.0 and gs.grad[0, F].item() == 0.0


def test_geglu_is_not_swiglu_and_not_the_erf_gelu(k):
    gu = torch.randn(16, 64, device=DEV)
    h = ops.geglu(gu)
    assert not torch.allclose(h, ops.swiglu(gu), atol=1e-3)
    tanh = torch.nn.functional.gelu(gu[:, :32].double(), approximate="tanh") * gu[:, 32:].double()
    erf = torch.nn.functional.gelu(gu[:, :32].double()) * gu[:, 32:].double()
    assert (h.double() - tanh).abs().max().item() < 0.1 * (tanh - erf).abs().max().item()


def test_geglu_rejects_and_empty(k):
    with pytest.raises(RuntimeError):
        k.geglu_fwd(torch.randn(3, 24, device=DEV))  # F = 12
    with pytest.raises(RuntimeError):
        k.geglu_bwd(torch.randn(3, 8, device=DEV), torch.randn(3, 32, device=DEV))  # dh is not [rows, F]
    with pytest.raises(RuntimeError):
        k.geglu_bwd(torch.randn(3, 16, device=DEV).bfloat16(), torch.randn(3, 32, device=DEV))  # dtypes differ
    h = k.geglu_fwd(torch.empty(0, 32, device=DEV))
    assert h.shape == (0, 16)
    assert k.geglu_bwd(h, torch.empty(0, 32, device=DEV)).shape == (0, 32)


# ------------------------------------------------------------------ 2. the sandwich norm
def post_reference(x, res, w, eps, dy):
    """fp64 ``res + x * rsqrt(mean(x^2) + eps) * w`` of the tensors as given, and its gradients for dy."""
    xd, wd = x.detach().double().requires_grad_(), w.detach().double().requires_grad_()
    rstd = (xd.pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    y = res.detach().double() + xd * rstd * wd
    y.backward(dy.detach().double())
    return {"y": y.detach(), "rstd": rstd.detach().squeeze(-1), "dx": xd.grad, "dw": wd.grad}


def check_post_norm(cols, rows, dtype, offset=0.0):
    x, res, w, _, dy = ln_inputs(rows, cols, dtype, True, offset)
    ref = post_reference(x, res, w, EPS, dy)
    xs, rs, ws = (t.clone().requires_grad_() for t in (x, res, w))
    y = ops.rms_norm_residual(xs, rs, ws, EPS)
    tag = f"rms_norm_residual {rows}x{cols} {dtype}"
    assert y.shape == x.shape and y.dtype == dtype
    assert_close(y, ref["y"], dtype, tag + " y")
    y.backward(dy)
    assert torch.equal(rs.grad, dy), tag + " dresidual is dy"
    assert_close(xs.grad, ref["dx"], dtype, tag + " dx")
    if dtype == torch.float32:
        assert_reduction(ws.grad, ref["dw"], tag + " dgamma")
    else:  # the backward reads x itself: no rounded copy in between
        assert_close(ws.grad, ref["dw"], dtype, tag + " dgamma")


# LayerNorm's dispatch (cols <= 2048: wave per row; <= 4096: 2 vectors per thread; <= 8192: 4; <= 16384: 8): both
# sides of 2048 | 2056, 4096 | 4104 and 8192 | 8200, so every forward variant and every backward kernel
POST_SHAPES = LN_SHAPES + [(4096, 67)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cols,rows", POST_SHAPES)
def test_post_norm_dispatch_edges(k, cols, rows, dtype):
    check_post_norm(cols, rows, dtype)


@pytest.mark.parametrize("cols", [1024, 4096, 8192])
def test_post_norm_offset_inputs(k, cols):
    """x = 100 + randn in fp32.  RMSNorm has no mean to cancel against: this checks the sum of x^2 (about 1e4
    per element, 8e7 per row) for overflow and precision -- every term is positive, so the fp32 sum stays
    within a few ulp relative and the fp32 tolerance holds."""
    check_post_norm(cols, 33, torch.float32, offset=100.0)


@pytest.mark.parametrize("cols", [12, 2052, 16392])
def test_post_norm_rejects_width(k, cols):
    """Widths that are no multiple of 8, and 16392 (> 8 vectors per thread)."""
    x = torch.randn(3, cols, device=DEV)
    w = torch.ones(cols, device=DEV)
    with pytest.raises(RuntimeError):
        k.rmsnorm_residual_fwd(x, x, w, EPS, True)
    with pytest.raises(RuntimeError):
        ops.rms_norm_residual(x, x, w)


def test_post_norm_rejects_mismatches(k):
    x = torch.randn(3, 64, device=DEV)
    w = torch.ones(64, device=DEV)
    with pytest.raises(RuntimeError):
        k.rmsnorm_residual_fwd(x, x[:2].contiguous(), w, EPS, True)   # residual shape
    with pytest.raises(RuntimeError):
        k.rmsnorm_residual_fwd(x, x.bfloat16(), w, EPS, True)         # residual dtype
    with pytest.raises(RuntimeError):
        k.rmsnorm_residual_fwd(x, x, w[:32].contiguous(), EPS, True)  # gamma size
    with pytest.raises(RuntimeError):
        k.rmsnorm_residual_fwd(x, x.cpu(), w, EPS, True)              # residual on the CPU


@pytest.mark.parametrize("dtype", DTYPES)
def test_post_norm_zero_rows(k, dtype):
    x = torch.empty(0, 64, device=DEV, dtype=dtype)
    w = torch.ones(64, device=DEV, dtype=dtype)
    y, rstd = k.rmsnorm_residual_fwd(x, x, w, EPS, True)
    assert y.shape == (0, 64) and rstd.shape == (0,)
    xs, rs, ws = x.clone().requires_grad_(), x.clone().requires_grad_(), w.clone().requires_grad_()
    out = ops.rms_norm_residual(xs, rs, ws)
    out.sum().backward()
    assert out.shape == (0, 64) and xs.grad.shape == (0, 64) and rs.grad.shape == (0, 64) and _all_zero(ws.grad)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cols,rows", [(1600, 300), (4096, 300)])
def test_post_norm_main_grad_accumulation(k, cols, rows, dtype):
    """weight.main_grad (fp32): the first backward after _mg_fresh = True overwrites the stale 7.0s, the
    second accumulates; weight.grad stays None."""
    x, res, w, _, dy = ln_inputs(rows, cols, dtype, True)
    dy2 = torch.randn(rows, cols, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5)).to(dtype)
    ref1 = post_reference(x, res, w, EPS, dy)["dw"]
    ref2 = post_reference(x, res, w, EPS, dy2)["dw"]
    ws = w.clone().requires_grad_()
    ws.main_grad = torch.full((cols,), 7.0, device=DEV)
    ws._mg_fresh = True
    ops.rms_norm_residual(x.clone().requires_grad_(), res, ws, EPS).backward(dy)
    assert_reduction(ws.main_grad, ref1, "main_grad after the first backward")
    ops.rms_norm_residual(x.clone().requires_grad_(), res, ws, EPS).backward(dy2)
    assert_reduction(ws.main_grad, ref1 + ref2, "main_grad after the second backward")
    assert ws.grad is None


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cols", [1600, 4096, 16384])
def test_post_norm_no_grad_forward_saves_nothing(k, cols, dtype):
    """Under no_grad (a checkpointed stage's first forward) no rstd is allocated and y has the bits of the
    recording forward; the recording forward's rstd is the fp64 one."""
    x, res, w, _, dy = ln_inputs(37, cols, dtype, True)
    y1, rstd = k.rmsnorm_residual_fwd(x, res, w, EPS, True)
    y0, none = k.rmsnorm_residual_fwd(x, res, w, EPS, False)
    assert none is None and torch.equal(y0, y1)
    assert rstd.dtype == torch.float32 and rstd.shape == (37,)
    assert_close(rstd, post_reference(x, res, w, EPS, dy)["rstd"], torch.float32, "rstd")
    xs = x.clone().requires_grad_()
    with torch.no_grad():
        y2 = ops.rms_norm_residual(xs, res, w, EPS)
    assert not y2.requires_grad and torch.equal(y2, y1)
    assert torch.equal(ops.rms_norm_residual(xs, res, w, EPS), y1)


# ------------------------------------------------------------------ 3. the model
CFG = CONFIGS["gemma2_block_tiny"]


@pytest.fixture(scope="module")
def gemma2_reference():
    """gemma2_block_tiny's blocks (bf16-rounded weights, the post-norm weights moved off 1) and, on the CPU eager
    path in fp32, the loss and gradients of one step."""
    torch.manual_seed(0)
    blocks = build_lm_blocks(CFG, dtype=torch.bfloat16)
    posts = [p for b in blocks for n, p in b.named_parameters() if n.endswith("post_norm_weight")]
    assert len(posts) == 2 * CFG.num_layers
    with torch.no_grad():
        for p in posts:
            p.add_(0.2 * torch.randn(CFG.d_model))
    ref = torch.nn.Sequential(*copy.deepcopy(blocks)).float().train()
    x, t = _data(CFG, 8)
    loss = _loss_fn(CFG)(ref(x), t)
    loss.backward()
    return blocks, float(loss.detach()), {n: p.grad for n, p in ref.named_parameters()}


def test_gemma2_block_tiny_bf16_matches_cpu_fp32(k, gemma2_reference):
    """test_llama_tiny_bf16_matches_cpu_fp32's comparison and bound (loss 2e-3 relative, each gradient 2e-2 of
    its max) on the Gemma-2 block."""
    blocks, ref_loss, ref_grads = gemma2_reference
    model = torch.nn.Sequential(*copy.deepcopy(blocks)).to(DEV).train()
    x, t = _data(CFG, 8)
    loss, grads = _gpu_step(model, CFG, x, t)
    assert sum(n.endswith("post_norm_weight") for n in grads) == 2 * CFG.num_layers
    _assert_model_close(loss, grads, ref_loss, ref_grads)


def _pipe_step(blocks, ckpt):
    """One step through Pipe over the pipeline units, cut after layer 1's (global, decoupled) attention core:
    (loss, gradients by the block model's parameter names)."""
    model = torch.nn.Sequential(*copy.deepcopy(blocks)).to(DEV).train()
    names = {id(p): n for n, p in model.named_parameters()}
    _note_embeddings(model)
    units = pipeline_units(list(model.children()))
    assert isinstance(units[5], PackedAttentionCore) and isinstance(units[6], PackedAttentionOutput)
    assert units[5].core.window is None and units[5].core.attn_dim != CFG.d_model
    opt = FlatAdam(model.parameters(), lr=1e-3)
    pipe = Pipe(torch.nn.Sequential(*units), chunks=4, checkpoint=ckpt, balance=[6, len(units) - 6],
                copy_same_device=True)
    x, t = _data(CFG, 8)
    try:
        assert len(pipe.partitions) == 2
        opt.zero_grad()
        loss = _loss_fn(CFG)(pipe(x.to(DEV)).local_value(), t.to(DEV))
        loss.backward()
        opt.fold_grads()
        torch.cuda.synchronize()
    finally:
        pipe.close()
    return float(loss.detach()), {names[id(p)]: p.main_grad.clone() for p in model.parameters()}


@pytest.fixture(scope="module")
def pipe_never(gemma2_reference):
    return _pipe_step(gemma2_reference[0], "never")


def test_gemma2_block_tiny_pipe_cut_after_a_decoupled_core(k, gemma2_reference, pipe_never):
    _, ref_loss, ref_grads = gemma2_reference
    loss, grads = pipe_never
    _assert_model_close(loss, grads, ref_loss, ref_grads)


def test_gemma2_block_tiny_pipe_recompute_bit_identical(k, gemma2_reference, pipe_never):
    """checkpoint='always' recomputes every micro-batch's forward (the no_grad forwards save nothing): the loss
    and every gradient equal 'never' bit for bit (the token embedding's up to its atomics' order)."""
    _, ref_loss, ref_grads = gemma2_reference
    loss0, g0 = pipe_never
    loss, g = _pipe_step(gemma2_reference[0], "always")
    _assert_model_close(loss, g, ref_loss, ref_grads)
    assert loss == loss0
    for n in g0:
        _assert_same_grad(g[n], g0[n], n, "always")


def test_gemma2_block_tiny_engine_step_flat_adam(k, gemma2_reference):
    blocks, ref_loss, ref_grads = gemma2_reference
    model = torch.nn.Sequential(*copy.deepcopy(blocks)).to(DEV).train()
    opt = FlatAdam(model.parameters(), lr=1e-3)
    m, mb = 4, 2
    eng = PipelineEngine(model, chunks=m, checkpoint="except_last", act_shape=(mb, CFG.seq_len),
                         act_dtype=torch.bfloat16, loss_fn=_loss_fn(CFG), device=torch.device(DEV, 0))
    x, t = _data(CFG, m * mb)
    before = [p.detach().clone() for p in model.parameters()]
    opt.zero_grad()
    st = eng.step([c.to(DEV) for c in x.split(mb)], [c.to(DEV) for c in t.split(mb)])
    opt.fold_grads()
    torch.cuda.synchronize()
    _assert_model_close(float(st.loss), {n: p.main_grad.clone() for n, p in model.named_parameters()}, ref_loss,
                        ref_grads)
    opt.step()
    torch.cuda.synchronize()
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
    assert all(torch.isfinite(p.detach().float()).all() for p in model.parameters())
