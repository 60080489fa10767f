"""Sliding-window attention on the GPU: the generic attention kernels with the
band mask (``window=W``: query i sees the keys i - W < j <= i), their tile
skipping on both sides of the band, the dispatch that keeps a windowed call off
the S = 128, wide and long-sequence kernels, dropout, checkpoint recompute, the
padded shapes, the fp32 fallback and the ``mistral_tiny`` model.  Everything
here but the fp32 fallback runs native code from mipipe/_C.so: the tests fail
if the extension is missing.

Shapes are the smallest that reach each path: S = 192 has three 64-key tiles,
so a query tile can skip a tile below the band and one above the diagonal; W =
1, 17 leave rows whose first visited tile is wholly masked; W = 64, 65 sit on
both sides of the tile edge; S = 128 and S = 256 / 320 at D = 64 are the shapes
a call without a window sends to other kernels."""
import copy
import math
import sys
import warnings

import pytest
import torch

from helpers.gqa_cases import gqa_inputs
from test_gpu_kernels import _attn_keep_mask, _tol
from test_gpu_llama_kernels import _assert_model_close, _data, _gpu_step, _loss_fn

from mipipe import Pipe, checkpoint, ops
from mipipe.models import CONFIGS, build_lm_blocks
from mipipe.models.transformer import AttentionCore
from mipipe.optim import FlatAdam
from mipipe.parallel import PipelineEngine

pytestmark = pytest.mark.gpu

DEV = "cuda"
B = 2


@pytest.fixture(scope="module")
def k():
    from mipipe._native_loader import kernels

    return kernels()


def _band(S, W, device):
    """keep[i, j]: j <= i and j > i - W, from arange (not the op's own mask code)."""
    i = torch.arange(S, device=device)[:, None]
    j = torch.arange(S, device=device)[None, :]
    return (j <= i) & (j > i - W)


def _band_reference(qkv, do, H, Hkv, W, dtype=torch.float64, keep=None, p=0.0):
    """Band attention on ``qkv [B, S, H + 2 Hkv, D]`` with repeated K/V heads, every step in ``dtype``:
    (o [B, S, H, D], dqkv); autograd sums each group.  ``keep [B, H, S, S]``: a dropout mask."""
    x = qkv.to(dtype).requires_grad_()
    q, kk, v = (t.transpose(1, 2) for t in (x[:, :, :H], x[:, :, H:H + Hkv], x[:, :, H + Hkv:]))
    g = H // Hkv
    kk, v = kk.repeat_interleave(g, 1), v.repeat_interleave(g, 1)
    S = q.shape[-2]
    s = torch.matmul(q, kk.transpose(-1, -2)) / math.sqrt(q.shape[-1])
    s = s.masked_fill(~_band(S, W, s.device), float("-inf"))
    pr = torch.softmax(s, dim=-1)
    if keep is not None:
        pr = pr * keep.to(pr.device).to(dtype) / (1 - p)
    o = torch.matmul(pr, v)
    o.backward(do.to(dtype).transpose(1, 2))
    return o.detach().transpose(1, 2), x.grad


def _run_op(qkv, do, H, Hkv, W, p=0.0, seed=11):
    """(o, dqkv) of the windowed op on ``qkv [B, S, H + 2 Hkv, D]``: attention_packed for Hkv == H (the same
    bytes viewed [B, S, 3, H, D]), attention_gqa_packed otherwise."""
    x = qkv.clone().requires_grad_()
    torch.manual_seed(seed)
    if Hkv == H:
        Bn, S, _, D = qkv.shape
        o = ops.attention_packed(x.view(Bn, S, 3, H, D), causal=True, dropout_p=p, training=True, window=W)
    else:
        o = ops.attention_gqa_packed(x, Hkv, causal=True, dropout_p=p, training=True, window=W)
    o.backward(do)
    torch.cuda.synchronize()
    return o.detach(), x.grad


def _assert_parts_close(o, dqkv, ref_o, ref_d, H, Hkv, dtype, tag):
    atol, rtol = _tol(dtype)
    for name, out, r in (("o", o, ref_o), ("dq", dqkv[:, :, :H], ref_d[:, :, :H]),
                         ("dk", dqkv[:, :, H:H + Hkv], ref_d[:, :, H:H + Hkv]),
                         ("dv", dqkv[:, :, H + Hkv:], ref_d[:, :, H + Hkv:])):
        err = (out.double() - r.double()).abs()
        print(f"{tag} {name}: max|err| {err.max().item():.3e}, "
              f"max excess {(err - atol - rtol * r.double().abs()).max().item():.3e}")
        assert torch.isfinite(out.float()).all(), f"{tag}: {name} not finite"
        assert torch.allclose(out.double(), r.double(), atol=atol, rtol=rtol), f"{tag}: {name}"


# ------------------------------------------------------------------ 1. against fp64
SDW = [(192, 64, 1), (192, 64, 17), (192, 64, 64), (192, 64, 65), (192, 64, 100),
       (192, 128, 80), (192, 128, 48),
       (64, 256, 33), (192, 256, 64),
       (128, 64, 33), (128, 128, 70),      # not the S = 128 one-pass kernels
       (256, 64, 64), (320, 64, 130)]      # not the long-sequence kernels


@pytest.mark.parametrize("H,Hkv", [(4, 4), (6, 2), (4, 1)])
@pytest.mark.parametrize("S,D,W", SDW)
def test_window_against_fp64(k, S, D, W, H, Hkv):
    assert k.attention_supported(S, D)
    qkv, do = gqa_inputs(B, S, H, Hkv, D, seed=2)
    o, dqkv = _run_op(qkv, do, H, Hkv, W)
    ref_o, ref_d = _band_reference(qkv, do, H, Hkv, W)
    _assert_parts_close(o, dqkv, ref_o, ref_d, H, Hkv, torch.bfloat16, f"S{S} D{D} W{W} H{H}/{Hkv}")
    if W == 1:  # a query sees itself only: p = 1 exactly and o is v, bit for bit
        g = H // Hkv
        assert torch.equal(o, qkv[:, :, H + Hkv:].repeat_interleave(g, 2))


@pytest.mark.parametrize("H,Hkv", [(4, 4), (6, 2), (4, 1)])
def test_window_of_one_gives_zero_dq_dk_exactly(k, H, Hkv):
    """W = 1: dS = P (dP - delta) is 0 in exact arithmetic, and dq == dk == 0 bit for bit on the kernels: the
    windowed backward takes delta_i = dO_i . O_i from the same MFMA arithmetic that gives dP_ii = dO_i . V_i
    (attn_delta_mfma_kernel), and O_i is V_i bit for bit here.  (With delta from attn_delta_kernel, which adds
    the same 64 products in another order, max|dq| was 1.3e-06 and max|dk| 1.1e-06 at these shapes.)"""
    S, D = 192, 64
    qkv, do = gqa_inputs(B, S, H, Hkv, D, seed=2)
    o, dqkv = _run_op(qkv, do, H, Hkv, 1)
    assert torch.equal(o, qkv[:, :, H + Hkv:].repeat_interleave(H // Hkv, 2))
    print(f"W=1 H{H}/{Hkv}: max|dq| {dqkv[:, :, :H].abs().max().item():.3e}, "
          f"max|dk| {dqkv[:, :, H:H + Hkv].abs().max().item():.3e}")
    assert torch.equal(dqkv[:, :, :H + Hkv], torch.zeros_like(dqkv[:, :, :H + Hkv]))


def test_window_separate_tensors(k):
    """``ops.attention`` on separate ``[B, H, S, D]`` tensors (permuted to the kernels' layout, not copied when
    they share strides)."""
    S, D, W, H = 192, 64, 65, 4
    qkv, do = gqa_inputs(B, S, H, H, D, seed=3)
    leaves = [t.transpose(1, 2).contiguous().requires_grad_() for t in qkv.view(B, S, 3, H, D).unbind(2)]
    o = ops.attention(*leaves, causal=True, window=W)
    o.backward(do.transpose(1, 2))
    ref_o, ref_d = _band_reference(qkv, do, H, H, W)
    dqkv = torch.cat([t.grad.transpose(1, 2) for t in leaves], dim=2)
    _assert_parts_close(o.detach().transpose(1, 2), dqkv, ref_o, ref_d, H, H, torch.bfloat16, "ops.attention")


# ------------------------------------------------------------------ 2. locality, bit for bit
@pytest.mark.parametrize("D", [64, 128])
def test_window_locality_bit_exact(k, D):
    """Keys outside a query's band and queries outside a key's band do not reach it at all: both loop bounds
    and both masks, to the row.  The overwritten rows keep randn scale (this tests skipping, not overflow)."""
    S, W, H, Hkv = 320, 70, 4, 2
    qkv, do = gqa_inputs(B, S, H, Hkv, D, seed=4)
    other, other_do = gqa_inputs(B, S, H, Hkv, D, seed=5)
    o0, d0 = _run_op(qkv, do, H, Hkv, W)

    kv = qkv.clone()
    kv[:, :128, H:] = other[:, :128, H:]          # K and V rows [0, 128)
    o1, d1 = _run_op(kv, do, H, Hkv, W)
    first = 128 + W - 1                            # the first query that sees none of them
    assert torch.equal(o1[:, first:], o0[:, first:])
    assert torch.equal(d1[:, first:, :H], d0[:, first:, :H])
    assert not torch.equal(o1[:, first - 1], o0[:, first - 1])  # the row before does see key 127

    qd = qkv.clone()
    qd[:, 256:, :H] = other[:, 256:, :H]          # Q and dO rows [256, 320)
    do2 = do.clone()
    do2[:, 256:] = other_do[:, 256:]
    o2, d2 = _run_op(qd, do2, H, Hkv, W)
    last = 256 - W                                 # keys j with j + W <= 256 are seen by none of them
    assert torch.equal(d2[:, :last + 1, H:], d0[:, :last + 1, H:])
    assert not torch.equal(d2[:, last + 1, H:], d0[:, last + 1, H:])  # key 187 is seen by query 256


# ------------------------------------------------------------------ 3. a window that covers the sequence
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("S,D", [(128, 64), (256, 64), (192, 128)])
def test_covering_window_is_todays_causal_path(k, S, D, p):
    H, Hkv = 4, 2
    qkv, do = gqa_inputs(B, S, H, Hkv, D, seed=6)
    x = qkv.clone().requires_grad_()
    torch.manual_seed(11)
    o0 = ops.attention_gqa_packed(x, Hkv, causal=True, dropout_p=p, training=True)
    o0.backward(do)
    for W in (S, S + 37):
        o, d = _run_op(qkv, do, H, Hkv, W, p=p)
        assert torch.equal(o, o0.detach()) and torch.equal(d, x.grad), (W, p)
    # the binding normalises it too: the same kernels (the long-sequence ones return keep bits, whose words
    # above the diagonal are never written, so only their shape is compared)
    q, kk, v = qkv[:, :, :H], qkv[:, :, H:H + Hkv], qkv[:, :, H + Hkv:]
    scale = 1.0 / math.sqrt(D)
    torch.manual_seed(11)
    a = k.attention_fwd(q, kk, v, True, p, scale)
    torch.manual_seed(11)
    b = k.attention_fwd(q, kk, v, True, p, scale, window=S)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2:4] == b[2:4] and a[4].shape == b[4].shape


def test_binding_refuses_bad_windows(k):
    qkv, _ = gqa_inputs(B, 64, 4, 4, 64)
    q, kk, v = qkv.view(B, 64, 3, 4, 64).unbind(2)
    with pytest.raises(RuntimeError, match="window"):
        k.attention_fwd(q, kk, v, True, 0.0, 0.125, window=-1)
    with pytest.raises(RuntimeError, match="causal"):
        k.attention_fwd(q, kk, v, False, 0.0, 0.125, window=8)
    with pytest.raises(RuntimeError, match="bf16"):
        k.attention_fwd(q.float(), kk.float(), v.float(), True, 0.0, 0.125, window=8)


# ------------------------------------------------------------------ 4. dropout
@pytest.mark.parametrize("S,D,W", [(192, 64, 64), (320, 64, 130)])
def test_window_dropout_exact_mask(k, S, D, W):
    """p = 0.25: the mask is the generic kernels' Philox keying (bh, q / 4, key) at every S -- also where a
    call without a window uses the long-sequence kernels' stored bits -- restricted to the band."""
    H, p = 2, 0.25
    qkv, do = gqa_inputs(B, S, H, H, D, seed=7)
    q, kk, v = qkv.view(B, S, 3, H, D).unbind(2)
    scale = 1.0 / math.sqrt(D)
    torch.manual_seed(11)
    _, _, seed, offset, bits = k.attention_fwd(q, kk, v, True, p, scale, window=W)
    assert bits.numel() == 0
    keep = _attn_keep_mask(B, H, S, p, seed, offset)
    assert abs(keep.float().mean().item() - (1 - p)) < 0.02
    o, dqkv = _run_op(qkv, do, H, H, W, p=p, seed=11)  # the same draw
    ref_o, ref_d = _band_reference(qkv, do, H, H, W, dtype=torch.float32, keep=keep, p=p)
    err = (o.float() - ref_o).abs().max().item()
    gerr = (dqkv.float() - ref_d).abs().max().item()
    gscale = ref_d.abs().max().item()
    print(f"S{S} W{W} p={p}: o err {err:.3e}, grad err {gerr:.3e} (scale {gscale:.3e})")
    assert err < 3e-2, err
    assert gerr < 3e-2 * max(1.0, gscale), (gerr, gscale)
    o2, _ = _run_op(qkv, do, H, H, W, p=p, seed=12)
    assert not torch.equal(o, o2)


# ------------------------------------------------------------------ 5. checkpoint recompute
def test_window_checkpoint_recompute_bit_exact(k):
    """S = 256, D = 64 is a long-sequence shape: without a window the first forward would leave keep words
    for the recompute.  A windowed call has none and regenerates the same mask from the restored draw."""
    A = sys.modules["mipipe.ops.attention"]
    S, E = 256, 256
    torch.manual_seed(0)
    core = AttentionCore(E, 4, 0.1, norm_first=True, causal=True, layer_norm_eps=1e-5, n_kv_heads=2,
                         window=100).to(DEV, torch.bfloat16).train()
    assert core.head_dim == 64 and k.attention_long_supported(S, core.head_dim)
    g = torch.Generator(device=DEV).manual_seed(8)
    base = torch.randn(B, S, E, device=DEV, generator=g).to(torch.bfloat16)
    do = torch.randn(B, S, E, device=DEV, generator=g).to(torch.bfloat16)

    def run(ckpt):
        core.zero_grad()
        x = base.clone().requires_grad_()
        torch.manual_seed(7)
        o = checkpoint(core, x) if ckpt else core(x)
        o.backward(do)
        torch.cuda.synchronize()
        return o.detach(), x.grad, core.in_proj_weight.grad.clone()

    A.clear_keep_words()
    before = dict(A.keep_stats)
    o1, g1, w1 = run(True)
    assert A.keep_stats == before and not A._keep_words
    o0, g0, w0 = run(False)
    assert torch.equal(o1, o0) and torch.equal(g1, g0) and torch.equal(w1, w0)
    core.eval()
    with torch.no_grad():
        assert not torch.equal(core(base), o0)  # the dropout was really there


# ------------------------------------------------------------------ 6. padded shapes
@pytest.mark.parametrize("S,D", [(100, 64), (192, 96)])
def test_window_padded_shapes_run_native(k, S, D):
    """A causal length padded at the end and a head dim padded with zero features keep the band exact: padded
    keys lie after every real query, padded features add 0 to every score."""
    A = sys.modules["mipipe.ops.attention"]
    W, H = 40, 4
    assert not k.attention_supported(S, D)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for Hkv in (4, 2):
            qkv, do = gqa_inputs(B, S, H, Hkv, D, seed=9)
            o, dqkv = _run_op(qkv, do, H, Hkv, W)
            ref_o, ref_d = _band_reference(qkv, do, H, Hkv, W)
            _assert_parts_close(o, dqkv, ref_o, ref_d, H, Hkv, torch.bfloat16, f"padded S{S} D{D} H{H}/{Hkv}")
        qkv, do = gqa_inputs(B, S, H, H, D, seed=10)
        leaves = [t.transpose(1, 2).contiguous().requires_grad_() for t in qkv.view(B, S, 3, H, D).unbind(2)]
        o = ops.attention(*leaves, causal=True, window=W)
        o.backward(do.transpose(1, 2))
    ref_o, ref_d = _band_reference(qkv, do, H, H, W)
    dqkv = torch.cat([t.grad.transpose(1, 2) for t in leaves], dim=2)
    _assert_parts_close(o.detach().transpose(1, 2), dqkv, ref_o, ref_d, H, H, torch.bfloat16, f"padded attention S{S}")
    assert not [key for key in A._noted if key[:2] == (S, D)]  # no eager path was noted for this shape


# ------------------------------------------------------------------ 7. fp32 is not native
def test_window_fp32_uses_eager_band_reference_and_warns_once(k):
    A = sys.modules["mipipe.ops.attention"]
    S, D, W, H, Hkv = 64, 64, 20, 4, 2
    qkv, do = gqa_inputs(B, S, H, Hkv, D, seed=11)
    qkv, do = qkv.float(), do.float()
    A._noted.discard((S, D, torch.float32, "window"))
    with pytest.warns(UserWarning, match="fp32 sliding-window attention is not native"):
        o, dqkv = _run_op(qkv, do, H, Hkv, W)
    ref_o, ref_d = _band_reference(qkv, do, H, Hkv, W)
    _assert_parts_close(o, dqkv, ref_o, ref_d, H, Hkv, torch.float32, "fp32")
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # once per shape
        o2, _ = _run_op(qkv, do, H, Hkv, W)
    assert torch.equal(o2, o)


# ------------------------------------------------------------------ 8. the model
@pytest.fixture(scope="module")
def mistral_reference():
    """mistral_tiny's blocks (bf16-rounded weights) and, on the CPU in fp32 -- where the attention is the eager
    fp32 band reference --, the loss and gradients of one step."""
    cfg = CONFIGS["mistral_tiny"]
    torch.manual_seed(0)
    blocks = build_lm_blocks(cfg, dtype=torch.bfloat16)
    assert all(b.core.window == 48 for b in blocks if hasattr(b, "core"))
    ref = torch.nn.Sequential(*copy.deepcopy(blocks)).float().train()
    x, t = _data(cfg, 8)
    loss = _loss_fn(cfg)(ref(x), t)
    loss.backward()
    return blocks, float(loss.detach()), {n: p.grad for n, p in ref.named_parameters()}


def test_mistral_tiny_pipe_step(k, mistral_reference):
    cfg = CONFIGS["mistral_tiny"]
    blocks, ref_loss, ref_grads = mistral_reference
    # unpipelined first: the windowed kernels inside the model
    model = torch.nn.Sequential(*copy.deepcopy(blocks)).to(DEV).train()
    x, t = _data(cfg, 8)
    loss, grads = _gpu_step(model, cfg, x, t)
    _assert_model_close(loss, grads, ref_loss, ref_grads)
    model = torch.nn.Sequential(*copy.deepcopy(blocks)).to(DEV).train()
    opt = FlatAdam(model.parameters(), lr=1e-3)
    pipe = Pipe(model, chunks=4, checkpoint="except_last", balance=[3, len(blocks) - 3], copy_same_device=True)
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


def test_mistral_tiny_engine_step_flat_adam(k, mistral_reference):
    cfg = CONFIGS["mistral_tiny"]
    blocks, ref_loss, ref_grads = mistral_reference
    model = torch.nn.Sequential(*copy.deepcopy(blocks)).to(DEV).train()
    opt = FlatAdam(model.parameters(), lr=1e-3)
    m, mb = 4, 2
    eng = PipelineEngine(model, chunks=m, checkpoint="except_last", act_shape=(mb, cfg.seq_len),
                         act_dtype=torch.bfloat16, loss_fn=_loss_fn(cfg), device=torch.device(DEV, 0))
    x, t = _data(cfg, m * mb)
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
