"""QK-norm on the CPU: the eager reference against an fp64 formula written out
here (forward and the gradients the kernels' backward computes), the V heads,
the ``qk_norm`` option of the blocks, the ``qwen3_*`` configs, and a QK-norm
model through the engine.  The HIP kernels behind the same ops are tested in
test_gpu_qknorm_kernels.py.

The reference computes in fp32 at least, so fp32 inputs are compared at the
project's fp32 bound (``helpers.rowwise_cases.FP32_TOL``) and fp64 inputs, where
the reference and the formula do the same arithmetic in another order, at 1e-12."""
import dataclasses
import math

import pytest
import torch

from helpers import engine_cases, qknorm_engine
from helpers.rowwise_cases import FP32_TOL

from mipipe import ops
from mipipe.models import CONFIGS, LMConfig, build_lm_blocks
from mipipe.models.transformer import (AttentionCore, SelfAttentionBlock, TransformerEncoderLayer,
                                       transformer_blocks)

B, S, D, EPS = 2, 7, 16, 1e-5
HEADS = [(4, 4), (6, 2), (4, 1)]


def qknorm_fp64(x, wq, wk, eps, cos, sin, n_q, n_k, pos0, dout):
    """``(y, dx, dwq, dwk)`` in fp64, every step written out: the forward of the kernel's header and the
    backward by the closed formulas (no autograd)."""
    x, wq, wk, dout = x.double(), wq.double(), wk.double(), dout.double()
    Bb, Ss, heads, Dd = x.shape
    half = Dd // 2
    n = n_q + n_k
    w = torch.cat((wq.expand(n_q, Dd), wk.expand(n_k, Dd)), 0)                   # [n, D]
    qk = x[:, :, :n]
    rstd = 1.0 / torch.sqrt((qk * qk).sum(-1, keepdim=True) / Dd + eps)
    xhat = qk * rstd
    nrm = xhat * w
    g = dout[:, :, :n]
    if cos is not None:
        c = cos[pos0:pos0 + Ss].double().view(1, Ss, 1, half)
        s = sin[pos0:pos0 + Ss].double().view(1, Ss, 1, half)
        a, b = nrm[..., :half], nrm[..., half:]
        y_qk = torch.cat((a * c - b * s, b * c + a * s), -1)
        ga, gb = g[..., :half], g[..., half:]
        g = torch.cat((ga * c + gb * s, gb * c - ga * s), -1)                     # the inverse rotation
    else:
        y_qk = nrm
    gy = g * w
    cm = (gy * xhat).sum(-1, keepdim=True) / Dd
    dx_qk = rstd * (gy - xhat * cm)
    dw = (g * xhat).sum((0, 1))                                                   # [n, D]
    y = torch.cat((y_qk, x[:, :, n:]), 2)
    dx = torch.cat((dx_qk, dout[:, :, n:]), 2)
    return y, dx, dw[:n_q].sum(0), dw[n_q:].sum(0)


def _inputs(h, hkv, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + 10 * h + hkv)
    x = torch.randn(B, S, h + 2 * hkv, D, generator=g, dtype=torch.float64).to(dtype)
    dout = torch.randn(B, S, h + 2 * hkv, D, generator=g, dtype=torch.float64).to(dtype)
    wq = (1 + 0.3 * torch.randn(D, generator=g, dtype=torch.float64)).to(dtype)
    wk = (1 + 0.3 * torch.randn(D, generator=g, dtype=torch.float64)).to(dtype)
    return x, wq, wk, dout


def _close(out, ref, dtype, what):
    if dtype == torch.float64:
        allowed = 1e-12 * (1 + ref.abs())
    else:
        allowed = FP32_TOL[0] + FP32_TOL[1] * ref.abs()
    over = ((out.double() - ref).abs() - allowed).max().item()
    assert over <= 0, f"{what}: {over:.3e} over the {dtype} bound"


# ------------------------------------------------------------------ 1. the reference against the fp64 formula
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("tables", [True, False])
@pytest.mark.parametrize("pos0", [0, 3])
@pytest.mark.parametrize("h,hkv", HEADS)
def test_reference_against_fp64_formula(h, hkv, pos0, tables, dtype):
    x, wq, wk, dout = _inputs(h, hkv, dtype)
    cos, sin = ops.rope_tables(pos0 + S + 2, D) if tables else (None, None)
    ref_y, ref_dx, ref_dwq, ref_dwk = qknorm_fp64(x, wq, wk, EPS, cos, sin, h, hkv, pos0, dout)
    tag = f"H{h}/{hkv} pos0={pos0} tables={tables} {dtype}"
    for op in (ops.qk_norm_rope_reference, ops.qk_norm_rope_heads):  # CPU tensors: the op IS the reference
        xs, qs, ks = (t.clone().requires_grad_() for t in (x, wq, wk))
        y = op(xs, qs, ks, EPS, cos, sin, h, hkv, pos0)
        assert y.dtype == dtype and y.shape == x.shape
        y.backward(dout)
        _close(y.detach(), ref_y, dtype, tag + " y")
        _close(xs.grad, ref_dx, dtype, tag + " dx")
        _close(qs.grad, ref_dwq, dtype, tag + " dwq")
        _close(ks.grad, ref_dwk, dtype, tag + " dwk")
        # V comes back bit for bit, forward and backward
        assert torch.equal(y[:, :, h + hkv:], x[:, :, h + hkv:])
        assert torch.equal(xs.grad[:, :, h + hkv:], dout[:, :, h + hkv:])


def test_reference_computes_bf16_inputs_in_fp32():
    x, wq, wk, dout = _inputs(4, 2, torch.bfloat16)
    cos, sin = ops.rope_tables(S, D)
    y = ops.qk_norm_rope_reference(x, wq, wk, EPS, cos, sin, 4, 2)
    assert y.dtype == torch.bfloat16
    ref_y = qknorm_fp64(x, wq, wk, EPS, cos, sin, 4, 2, 0, dout)[0]
    # one rounding of an fp32 result: half a bf16 ulp (2**-7 of the binade), at most 2**-8 relative, plus the fp32 term
    over = ((y.double() - ref_y).abs() - (2.0 ** -8 * ref_y.abs() + FP32_TOL[0])).max().item()
    assert over <= 0, over


def test_projection_views_and_bad_arguments():
    x, wq, wk, _ = _inputs(4, 2, torch.float32)
    cos, sin = ops.rope_tables(S, D)
    y4 = ops.qk_norm_rope_projection(x.view(B, S, -1), wq, wk, EPS, cos, sin, 4, n_kv_heads=2)
    assert y4.shape == (B, S, 8, D)
    assert torch.equal(y4, ops.qk_norm_rope_reference(x, wq, wk, EPS, cos, sin, 4, 2))
    x, wq, wk, _ = _inputs(4, 4, torch.float32)
    y5 = ops.qk_norm_rope_projection(x.view(B, S, -1), wq, wk, EPS, None, None, 4)
    assert y5.shape == (B, S, 3, 4, D)
    assert torch.equal(y5.view(B, S, 12, D), ops.qk_norm_rope_reference(x, wq, wk, EPS, None, None, 4, 4))
    with pytest.raises(ValueError, match="n_q"):
        ops.qk_norm_rope_heads(x, wq, wk, EPS, cos, sin, 9, 4)
    with pytest.raises(ValueError, match="wq and wk"):
        ops.qk_norm_rope_heads(x, wq[:8], wk, EPS, cos, sin, 4, 4)
    with pytest.raises(ValueError, match="both cos and sin"):
        ops.qk_norm_rope_heads(x, wq, wk, EPS, cos, None, 4, 4)


# ------------------------------------------------------------------ 2. the blocks
def test_attention_core_owns_the_two_weights():
    kw = dict(norm_first=True, causal=True, layer_norm_eps=1e-6, norm="rms", bias=False, rope=True)
    core = AttentionCore(64, 4, 0.0, n_kv_heads=2, qk_norm=True, **kw)
    assert core.qk_norm and core.eps == 1e-6
    assert core.q_norm_weight.shape == (16,) and core.k_norm_weight.shape == (16,)
    assert torch.equal(core.q_norm_weight, torch.ones(16)) and torch.equal(core.k_norm_weight, torch.ones(16))
    assert not getattr(core.q_norm_weight, "_mipipe_gemm_weight", False)
    assert not getattr(core.k_norm_weight, "_mipipe_gemm_weight", False)
    with torch.no_grad():
        core.q_norm_weight.fill_(3.0)
    core.reset_parameters()
    assert torch.equal(core.q_norm_weight, torch.ones(16))
    names = {n for n, _ in core.named_parameters()}
    assert {"q_norm_weight", "k_norm_weight"} <= names


def test_qk_norm_off_keeps_the_state_dict_keys():
    kw = dict(norm_first=True, causal=True, layer_norm_eps=1e-5, norm="rms", bias=False, rope=True, n_kv_heads=2)
    off = AttentionCore(64, 4, 0.0, **kw)
    assert off.qk_norm is False
    assert set(off.state_dict()) == {"in_proj_weight", "norm_weight"}
    assert not hasattr(off, "q_norm_weight") and not hasattr(off, "k_norm_weight")
    on = AttentionCore(64, 4, 0.0, qk_norm=True, **kw)
    assert set(on.state_dict()) == set(off.state_dict()) | {"q_norm_weight", "k_norm_weight"}
    for cfg_name in ("tiny", "llama_gqa_tiny", "mistral_tiny"):
        assert CONFIGS[cfg_name].qk_norm is False
        with torch.device("meta"):
            keys = torch.nn.Sequential(*build_lm_blocks(CONFIGS[cfg_name])).state_dict().keys()
        assert not [k for k in keys if "q_norm" in k or "k_norm" in k]
    assert LMConfig("x", 1, 32, 4, 64, 100, 8).qk_norm is False
    assert [f.name for f in dataclasses.fields(LMConfig)][-1] == "qk_norm"


def test_keyword_reaches_every_layer_of_the_builders():
    assert SelfAttentionBlock(32, 4, 0.0, qk_norm=True).core.qk_norm
    assert TransformerEncoderLayer(32, 4, 64, 0.0, qk_norm=True)[0].core.qk_norm
    blocks = transformer_blocks(2, 32, 4, 64, 0.0, qk_norm=True)
    assert [b.core.qk_norm for b in blocks if isinstance(b, SelfAttentionBlock)] == [True, True]
    assert not SelfAttentionBlock(32, 4, 0.0).core.qk_norm


def test_lmconfig_qk_norm_reaches_every_core():
    cfg = qknorm_engine.qknorm_cfg()
    blocks = build_lm_blocks(cfg)
    cores = [b.core for b in blocks if isinstance(b, SelfAttentionBlock)]
    assert len(cores) == cfg.num_layers == 2
    assert all(c.qk_norm and c.q_norm_weight.shape == (8,) and c.k_norm_weight.shape == (8,) for c in cores)
    with torch.device("meta"):
        tiny = build_lm_blocks(CONFIGS["qwen3_tiny"])
    assert [b.core.qk_norm for b in tiny if isinstance(b, SelfAttentionBlock)] == [True, True]
    off = build_lm_blocks(dataclasses.replace(cfg, qk_norm=False))
    assert not any(b.core.qk_norm for b in off if isinstance(b, SelfAttentionBlock))


# ------------------------------------------------------------------ 3. configs
def test_params_counts_the_norm_weights():
    cfg = CONFIGS["qwen3_tiny"]
    blocks = build_lm_blocks(cfg)
    real = sum(p.numel() for b in blocks for p in b.parameters())
    dec = blocks[-1]
    real -= (dec.padded - dec.ntoken) * (cfg.d_model + 1)  # the zero rows that pad the vocabulary
    assert cfg.params() == real
    base = dataclasses.replace(cfg, qk_norm=False)
    assert cfg.params() - base.params() == cfg.num_layers * 2 * (cfg.d_model // cfg.nhead)


def test_qwen3_configs_are_what_the_names_say():
    tiny, base = CONFIGS["qwen3_tiny"], CONFIGS["llama_gqa_tiny"]
    assert tiny.qk_norm and dataclasses.replace(tiny, name=base.name, qk_norm=False, notes=base.notes) == base
    c = CONFIGS["qwen3_8b"]
    assert (c.num_layers, c.d_model, c.nhead, c.n_kv_heads, c.d_model // c.nhead, c.dim_feedforward, c.vocab,
            c.seq_len, c.rope_base) == (36, 4096, 32, 8, 128, 12288, 151936, 32768, 1e6)
    assert (c.norm, c.activation, c.bias, c.rope, c.qk_norm, c.causal, c.norm_first, c.positions, c.dropout) == (
        "rms", "swiglu", False, True, True, True, True, "none", 0.0)
    assert "untied" in c.notes and "bias" in c.notes
    l3 = CONFIGS["llama3_8b"]
    assert dataclasses.replace(c, name=l3.name, num_layers=32, dim_feedforward=l3.dim_feedforward, vocab=l3.vocab,
                               seq_len=l3.seq_len, rope_base=l3.rope_base, qk_norm=False, notes=l3.notes) == l3
    # 36 layers of two 128-wide weights on top of the same model without the norm
    assert c.params() - dataclasses.replace(c, qk_norm=False).params() == 36 * 2 * 128


# ------------------------------------------------------------------ 4. a model
@pytest.mark.parametrize("rope,hkv", [(True, 2), (True, 4), (False, 2)])
def test_qk_norm_model_forward_backward_runs(rope, hkv):
    """A forward and backward of the replica on the CPU; every norm weight gets a finite non-zero gradient, and
    the norm is really applied: the same weights without it give another loss."""
    cfg = dataclasses.replace(qknorm_engine.qknorm_cfg(), rope=rope, n_kv_heads=hkv,
                              positions="none" if rope else "sinusoidal")
    torch.manual_seed(0)
    model = torch.nn.Sequential(*build_lm_blocks(cfg)).train()
    tok = torch.randint(0, cfg.vocab, (4, cfg.seq_len + 1), generator=torch.Generator().manual_seed(7))
    x, t = tok[:, :-1], tok[:, 1:].contiguous()
    loss_fn = lambda y: ops.cross_entropy(y.reshape(-1, cfg.vocab), t.reshape(-1))  # noqa: E731
    loss = loss_fn(model(x))
    loss.backward()
    loss = float(loss.detach())
    assert math.isfinite(loss)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    norm_w = [p for n, p in model.named_parameters() if n.endswith(("q_norm_weight", "k_norm_weight"))]
    assert len(norm_w) == 2 * cfg.num_layers
    assert all(p.grad.abs().max().item() > 0 for p in norm_w)
    for b in model:
        if isinstance(b, SelfAttentionBlock):
            b.core.qk_norm = False
    assert float(loss_fn(model(x)).detach()) != loss


# ------------------------------------------------------------------ 5. the engine, two gloo ranks
def test_qk_norm_engine_two_gloo_ranks(monkeypatch):
    """helpers.engine_cases.run_engine_case as test_engine.py runs it, on the QK-norm replica: the spawned
    ranks start in helpers.qknorm_engine.worker, which swaps the helper's config and runs its worker."""
    monkeypatch.setattr(engine_cases, "case_cfg", qknorm_engine.qknorm_cfg)
    monkeypatch.setattr(engine_cases, "worker", qknorm_engine.worker)
    engine_cases.run_engine_case("cpu", 2, "except_last", 1, False, False)
