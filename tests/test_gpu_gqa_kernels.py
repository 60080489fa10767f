"""Grouped-query attention on the GPU: the attention kernels reading shared K/V
heads in place, the dK/dV group-sum kernel, the generalised RoPE launcher and
the ``llama_gqa_tiny`` model.  Everything here runs native code from
mipipe/_C.so: the tests fail if the extension is missing.

Shapes are the smallest that reach each kernel: S=64 and 192 with D in {64,
128, 256} the generic forward / delta / dK-dV / dQ kernels (at D=64 both the
64-row and, where S allows, the wide forward and dQ), S=128 the fused one-pass
forward and backward, S=256 and 320 (a partly filled 256-row block) the
long-sequence 32x32x16 kernels."""
import copy
import dataclasses
import math
import os
import subprocess
import sys

import pytest
import torch

from helpers.gqa_cases import HEADS, check_native_against_expanded, expand, gqa_inputs, run_native
from helpers.rowwise_cases import assert_close
from test_gpu_kernels import _tol
from test_gpu_llama_kernels import _assert_model_close, _data, _gpu_step, _loss_fn, _pipe_grads
from test_gpu_pipeline import _assert_same_grad

from mipipe import Pipe, ops
from mipipe.models import CONFIGS, build_lm_blocks
from mipipe.optim import FlatAdam

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
B = 2
GENERIC = [(64, 64), (192, 64), (192, 128), (64, 256)]   # (S, D)
S128 = [(128, 64), (128, 128)]
LONG = [(256, 64), (320, 64)]
SHAPES = GENERIC + S128 + LONG


@pytest.fixture(scope="module")
def k():
    from mipipe._native_loader import kernels

    return kernels()


# ------------------------------------------------------------------ 1. native against the existing kernels
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("H,Hkv", HEADS)
@pytest.mark.parametrize("S,D", SHAPES)
def test_native_equals_repeated_heads(k, S, D, H, Hkv, causal):
    assert k.attention_supported(S, D)
    assert k.attention_long_supported(S, D) == ((S, D) in LONG)
    check_native_against_expanded(B, S, H, Hkv, D, causal)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("S,D", SHAPES)
def test_native_equals_repeated_heads_with_dropout(k, S, D, causal):
    """Groups of 3, p = 0.1: both runs draw the same Philox (seed, offset), and the counters are
    indexed by the QUERY head, so the masks are the same and the same equalities hold."""
    check_native_against_expanded(B, S, 6, 2, D, causal, p=0.1)
    # the mask is really there: another draw changes the output
    qkv, do = gqa_inputs(B, S, 6, 2, D)
    o1, _ = run_native(qkv, do, 2, causal, 0.1, seed=11)
    o2, _ = run_native(qkv, do, 2, causal, 0.1, seed=12)
    assert not torch.equal(o1, o2)


# ------------------------------------------------------------------ 2. absolute correctness
def _attention_fp64(q, k, v, causal):
    """Softmax attention on ``[B, H, S, D]`` fp64 tensors, every step in fp64 (an oracle of its own: the
    package's ``attention_reference`` computes in fp32 and is the expansion route's eager path)."""
    s = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(q.shape[-1])
    if causal:
        n = s.shape[-1]
        s = s.masked_fill(torch.ones(n, n, dtype=torch.bool, device=s.device).triu(1), float("-inf"))
    return torch.matmul(torch.softmax(s, dim=-1), v)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("S,D", [(192, 64), (192, 128), (64, 256), (128, 64), (128, 128), (320, 64)])
def test_native_against_reference_on_repeated_heads(k, S, D, causal):
    """(6, 2), p = 0, one shape per kernel family: forward and gradients against fp64 attention on repeated
    heads (autograd sums each group), at test_gpu_kernels._tol(bf16); ``ops.attention_reference`` on the same
    fp64 tensors agrees with the oracle to its own fp32 rounding."""
    H, Hkv = 6, 2
    qkv, do = gqa_inputs(B, S, H, Hkv, D, seed=1)
    o, dqkv = run_native(qkv, do, Hkv, causal, 0.0)
    x = qkv.double().requires_grad_()
    q, kk, v = (t.transpose(1, 2) for t in (x[:, :, :H], x[:, :, H:H + Hkv], x[:, :, H + Hkv:]))
    g = H // Hkv
    kr, vr = kk.repeat_interleave(g, 1), v.repeat_interleave(g, 1)
    ref = _attention_fp64(q, kr, vr, causal)
    assert ref.dtype == torch.float64
    with torch.no_grad():
        eager = ops.attention_reference(q, kr, vr, causal, 0.0)
    assert (eager - ref).abs().max().item() < 1e-4
    ref.backward(do.double().transpose(1, 2))
    atol, rtol = _tol(torch.bfloat16)
    for name, out, r in (("o", o, ref.detach().transpose(1, 2)), ("dq", dqkv[:, :, :H], x.grad[:, :, :H]),
                         ("dk", dqkv[:, :, H:H + Hkv], x.grad[:, :, H:H + Hkv]),
                         ("dv", dqkv[:, :, H + Hkv:], x.grad[:, :, H + Hkv:])):
        err = (out.double() - r).abs()
        print(f"S{S} D{D} causal={causal} {name}: max|err| {err.max().item():.3e}, "
              f"max excess {(err - atol - rtol * r.abs()).max().item():.3e}")
        assert torch.allclose(out.double(), r, atol=atol, rtol=rtol), name


# ------------------------------------------------------------------ 3. keep words across a checkpoint
@pytest.mark.parametrize("causal", [False, True])
def test_gqa_keep_words_reused_bit_exact(k, causal):
    """The GQA case of test_gpu_kernels.test_attention_keep_words_reused_bit_exact: the recompute reads the
    first forward's keep words (their key is the Philox draw; their index the query head)."""
    from mipipe import checkpoint

    A = sys.modules["mipipe.ops.attention"]
    S, H, Hkv, D, p = 256, 4, 2, 64, 0.1
    assert k.attention_long_supported(S, D)
    base, g = gqa_inputs(B, S, H, Hkv, D, seed=5)

    def run(ckpt: bool, reuse: bool):
        A._KEEP_REUSE = reuse
        A.clear_keep_words()
        x = base.clone().requires_grad_()
        torch.manual_seed(7)
        f = lambda t: ops.attention_gqa_packed(t, Hkv, causal, p, True)  # noqa: E731
        o = checkpoint(f, x) if ckpt else f(x)
        o.backward(g)
        torch.cuda.synchronize()
        return o.detach(), x.grad

    old = A._KEEP_REUSE
    try:
        before = dict(A.keep_stats)
        o1, g1 = run(True, True)
        assert A.keep_stats["stored"] == before["stored"] + 1 and A.keep_stats["reused"] == before["reused"] + 1
        assert not A._keep_words  # taken by the recompute
        o0, g0 = run(True, False)
        o2, g2 = run(False, True)
    finally:
        A._KEEP_REUSE = old
        A.clear_keep_words()
    assert torch.equal(o1, o0) and torch.equal(g1, g0)
    assert torch.equal(o1, o2) and torch.equal(g1, g2)


# ------------------------------------------------------------------ 4. kernels behind a switch
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("H,Hkv", [(4, 2), (6, 2)])
@pytest.mark.parametrize("S,D", S128)
def test_unfused_s128_backward(k, S, D, H, Hkv, causal):
    """attention_set_fused_bwd(0): S = 128 on the generic forward and the delta + dK/dV + dQ kernels."""
    k.attention_set_fused_bwd(0)
    try:
        check_native_against_expanded(B, S, H, Hkv, D, causal)
        check_native_against_expanded(B, S, H, Hkv, D, causal, p=0.1)
    finally:
        k.attention_set_fused_bwd(1)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("S", [256, 320])
def test_long_mask_kernel_rng(k, S, causal):
    """attention_long_set_fused_rng(False): keep words made by their own kernel, read by the forward."""
    k.attention_long_set_fused_rng(False)
    try:
        check_native_against_expanded(B, S, 6, 2, 64, causal, p=0.1)
    finally:
        k.attention_long_set_fused_rng(True)


@pytest.mark.parametrize("switch", ["MIPIPE_ATTN_LONG", "MIPIPE_ATTN_DKDV8"])
def test_env_switched_kernels(switch):
    """Read once per process: one fresh child each (S=256 D=64, 4 query heads over 2 K/V heads) on the
    generic kernels at a long-sequence shape and on the 4-wave long-sequence dK/dV kernel."""
    env = dict(os.environ)
    env[switch] = "0"
    worker = os.path.join(ROOT, "tests", "helpers", "gqa_worker.py")
    r = subprocess.run([sys.executable, worker], env=env, timeout=240, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True)
    assert r.returncode == 0, r.stdout[-4000:]


def test_native_refuses_what_it_cannot_run(k):
    """fp32 has no native grouped kernels (the op repeats the heads instead); the binding says so."""
    qkv = torch.randn(1, 64, 8, 64, device=DEV)
    q, kk, v = qkv[:, :, :4], qkv[:, :, 4:6], qkv[:, :, 6:]
    with pytest.raises(RuntimeError, match="bf16"):
        k.attention_fwd(q, kk, v, False, 0.0, 0.125)
    qb = qkv.bfloat16()
    with pytest.raises(RuntimeError):  # 4 query heads over 3 K/V heads
        k.attention_fwd(qb[:, :, :4], qb[:, :, 4:7], qb[:, :, 4:7], False, 0.0, 0.125)
    o, lse, _, _, _ = k.attention_fwd(qb[:, :, :4], qb[:, :, 4:6], qb[:, :, 6:], False, 0.0, 0.125)
    other = torch.empty_like(qb)
    d = torch.empty_like(qb)
    with pytest.raises(RuntimeError, match="packed"):  # gradients not the slices of one packed buffer
        k.attention_bwd(o, qb[:, :, :4], qb[:, :, 4:6], qb[:, :, 6:], o, lse, False, 0.0, 0.125, 0, 0,
                        d[:, :, :4], other[:, :, 4:6], d[:, :, 6:], None, 0)
    # the op takes the expansion route for fp32 and agrees with repeated heads
    x = qkv.clone().requires_grad_()
    o = ops.attention_gqa_packed(x, 2)
    o5 = ops.attention_packed(expand(qkv, 4, 2))
    assert torch.equal(o, o5)
    o.sum().backward()
    assert x.grad.shape == qkv.shape and torch.isfinite(x.grad).all()
    # separate q, k, v with fewer K/V heads: repeated, on the kernels
    qh, kh, vh = (t.transpose(1, 2).contiguous() for t in (qb[:, :, :4], qb[:, :, 4:6], qb[:, :, 6:]))
    oa = ops.attention(qh, kh, vh, causal=True)
    ob = ops.attention(qh, kh.repeat_interleave(2, 1), vh.repeat_interleave(2, 1), causal=True)
    assert torch.equal(oa, ob)


# ------------------------------------------------------------------ 5. the reduce kernel alone
REDUCE_SHAPES = [(1, 1, 2, 1, 64), (3, 67, 6, 2, 64), (2, 130, 8, 1, 128), (1, 5, 16, 2, 256)]  # B, S, H, Hkv, D


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("Bn,S,H,Hkv,D", REDUCE_SHAPES)
def test_gqa_reduce_dkv(k, Bn, S, H, Hkv, D, dtype):
    g = torch.Generator(device=DEV).manual_seed(S * 13 + H)
    dkv = torch.randn(Bn, S, 2, H, D, device=DEV, generator=g).to(dtype)
    sentinel = torch.full((Bn, S, H + 2 * Hkv, D), -7.0, device=DEV, dtype=dtype)
    dqkv = sentinel.clone()
    k.gqa_reduce_dkv(dkv, dqkv, H, Hkv)
    ref = dkv.double().view(Bn, S, 2, Hkv, H // Hkv, D).sum(4)
    assert torch.equal(dqkv[:, :, :H], sentinel[:, :, :H])  # the Q slots are not touched
    assert_close(dqkv[:, :, H:H + Hkv], ref[:, :, 0], dtype, "dk")
    assert_close(dqkv[:, :, H + Hkv:], ref[:, :, 1], dtype, "dv")


def test_gqa_reduce_dkv_rejects(k):
    ok = torch.zeros(1, 4, 2, 4, 64, device=DEV)
    dst = torch.zeros(1, 4, 8, 64, device=DEV)
    k.gqa_reduce_dkv(ok, dst, 4, 2)
    with pytest.raises(RuntimeError):  # 4 query heads over 3 K/V heads
        k.gqa_reduce_dkv(ok, torch.zeros(1, 4, 10, 64, device=DEV), 4, 3)
    with pytest.raises(RuntimeError):  # D % 8 != 0
        k.gqa_reduce_dkv(torch.zeros(1, 4, 2, 4, 12, device=DEV), torch.zeros(1, 4, 8, 12, device=DEV), 4, 2)
    with pytest.raises(RuntimeError):  # destination of the wrong width (3 H heads)
        k.gqa_reduce_dkv(ok, torch.zeros(1, 4, 12, 64, device=DEV), 4, 2)
    with pytest.raises(RuntimeError):  # dtypes differ
        k.gqa_reduce_dkv(ok, dst.bfloat16(), 4, 2)
    with pytest.raises(RuntimeError):  # not contiguous
        k.gqa_reduce_dkv(ok, torch.zeros(1, 4, 16, 64, device=DEV)[:, :, ::2], 4, 2)


# ------------------------------------------------------------------ 6. generalised RoPE
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("pos0", [0, 3])
@pytest.mark.parametrize("H,Hkv,D", [(4, 2, 16), (6, 2, 64), (4, 1, 128)])
def test_rope_heads_against_fp64(k, H, Hkv, D, pos0, dtype):
    """Q and K parts against ``rope_reference`` applied per part in fp64, V bit-identical, in-place bits
    equal to out-of-place bits, the backward the inverse rotation."""
    Bn, S = 2, 67
    g = torch.Generator(device=DEV).manual_seed(S * 7 + D + H)
    x = torch.randn(Bn, S, H + 2 * Hkv, D, device=DEV, generator=g).to(dtype)
    grad = torch.randn(Bn, S, H + 2 * Hkv, D, device=DEV, generator=g).to(dtype)
    cos, sin = ops.rope_tables(pos0 + S + 3, D, device=DEV)
    n_rot = H + Hkv

    def per_part(t, inverse=False):  # each part as the Q of a [B, S, 3, n, D] tensor through rope_reference
        parts = []
        for lo, hi in ((0, H), (H, n_rot)):
            five = torch.stack((t[:, :, lo:hi].double(),) * 3, dim=2)
            parts.append(ops.rope_reference(five, cos, sin, pos0, inverse=inverse)[:, :, 0])
        return torch.cat(parts, dim=2)

    xs = x.clone().requires_grad_()
    out = ops.rope_heads(xs, cos, sin, n_rot, pos0)
    tag = f"rope_heads {H}/{Hkv} D{D} pos0={pos0} {dtype}"
    assert out.data_ptr() != xs.data_ptr() and torch.equal(xs.detach(), x)
    assert_close(out[:, :, :n_rot], per_part(x), dtype, tag)
    assert torch.equal(out[:, :, n_rot:], x[:, :, n_rot:])
    out.backward(grad)
    assert_close(xs.grad[:, :, :n_rot], per_part(grad, inverse=True), dtype, tag + " backward")
    assert torch.equal(xs.grad[:, :, n_rot:], grad[:, :, n_rot:])
    buf = x.clone()
    same = ops.rope_heads(buf, cos, sin, n_rot, pos0, inplace=True)
    assert same.data_ptr() == buf.data_ptr() and torch.equal(same, out)
    # the models' entry point: the projection output [B, S, (H + 2 Hkv) D], in place without a graph
    proj = x.clone().view(Bn, S, -1)
    with torch.no_grad():
        via = ops.rope_projection(proj, cos, sin, H, pos0, n_kv_heads=Hkv)
    assert via.shape == x.shape and via.data_ptr() == proj.data_ptr() and torch.equal(via, out)
    leaf = x.clone().view(Bn, S, -1).requires_grad_()
    via2 = ops.rope_projection(leaf * 1, cos, sin, H, pos0, n_kv_heads=Hkv)
    via2.backward(grad)
    assert torch.equal(via2, out) and torch.equal(leaf.grad.view_as(x), xs.grad)


def test_rope_heads_rejects(k):
    cos, sin = ops.rope_tables(8, 32, device=DEV)
    x = torch.randn(1, 8, 6, 32, device=DEV)
    with pytest.raises(RuntimeError):  # more heads to rotate than there are
        k.rope_heads(x, cos, sin, None, 7)
    with pytest.raises(RuntimeError):  # tables end at position 8
        k.rope_heads(x, cos, sin, None, 4, 1)
    with pytest.raises(RuntimeError):  # D = 24
        k.rope_heads(torch.randn(1, 8, 6, 24, device=DEV), *ops.rope_tables(8, 24, device=DEV), None, 4)
    assert torch.equal(k.rope_heads(x, cos, sin, None, 0), x)  # nothing rotated: a copy


# ------------------------------------------------------------------ 7. the model
def _cfg(**kw):
    return dataclasses.replace(CONFIGS["llama_gqa_tiny"], **kw)


@pytest.fixture(scope="module")
def gqa_unpipelined():
    """llama_gqa_tiny in bf16 on the GPU, one unpipelined step: (blocks as built, loss, gradients)."""
    cfg = _cfg()
    torch.manual_seed(0)
    blocks = build_lm_blocks(cfg, dtype=torch.bfloat16)
    model = torch.nn.Sequential(*copy.deepcopy(blocks)).to(DEV).train()
    x, t = _data(cfg, 8)
    loss, grads = _gpu_step(model, cfg, x, t)
    return blocks, loss, grads


def test_llama_gqa_tiny_bf16_matches_cpu_fp32(k, gqa_unpipelined):
    cfg = _cfg()
    blocks, loss, grads = gqa_unpipelined
    assert blocks[1].core.in_proj_weight.shape == (512, 256)
    ref = torch.nn.Sequential(*copy.deepcopy(blocks)).float().train()
    x, t = _data(cfg, 8)
    ref_loss = _loss_fn(cfg)(ref(x), t)
    ref_loss.backward()
    _assert_model_close(loss, grads, float(ref_loss.detach()), {n: p.grad for n, p in ref.named_parameters()})


@pytest.mark.parametrize("checkpoint", ["never", "except_last", "always"])
def test_llama_gqa_tiny_pipe_two_partitions(k, gqa_unpipelined, checkpoint):
    cfg = _cfg()
    blocks, ref_loss, ref_grads = gqa_unpipelined
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


def test_llama_gqa_recompute_bit_identical_with_dropout(k):
    """Dropout 0.1 (embedding, attention, the norm kernels' residual dropout): 'always' and 'except_last'
    regenerate the same Philox masks, so their gradients equal 'never' bit for bit."""
    cfg = _cfg(dropout=0.1, norm_first=False)
    loss0, g0 = _pipe_grads("never", cfg)
    _, g_other = _pipe_grads("never", cfg, seed=100)
    assert any(not torch.equal(g0[n], g_other[n]) for n in g0)
    for mode in ("except_last", "always"):
        loss, g = _pipe_grads(mode, cfg)
        assert loss == loss0, mode
        for n in g0:
            _assert_same_grad(g[n], g0[n], n, mode)
