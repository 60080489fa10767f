"""Logit soft-capping on the CPU: the eager attention ops and ``ops.softcap`` against fp64 formulas written
here, the errors, the ``attn_softcap`` / ``final_softcap`` options of the blocks and of ``LMConfig``, the decoder
split that a final cap rules out, the ``gemma2_tiny`` config, and a capped model through the engine.  The HIP
kernels behind the same keywords are tested in test_gpu_softcap_kernels.py.

The CPU paths compute in fp32 whatever they are given, so the comparisons with the fp64 oracles are at the
project's fp32 bound (``helpers.rowwise_cases.FP32_TOL``)."""
import dataclasses
import math

import pytest
import torch

from helpers import engine_cases, softcap_engine
from helpers.rowwise_cases import FP32_TOL

from mipipe import ops
from mipipe.models import CONFIGS, LMConfig, build_lm_blocks, lm_pipeline_units, split_decoder
from mipipe.models.lm import Decoder
from mipipe.models.transformer import (AttentionCore, SelfAttentionBlock, TransformerEncoderLayer, block_flops,
                                       transformer_blocks)
from mipipe.parallel.stage import block_costs, choose_virtual, plan_stages

B, S, D = 2, 24, 16


def capped_attention_fp64(q, k, v, cap, causal, window):
    """``[B, H, S, D]`` fp64 attention with the scaled scores capped at ``cap * tanh(s / cap)`` before the masks."""
    n = q.shape[-2]
    i = torch.arange(n)[:, None]
    j = torch.arange(n)[None, :]
    s = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(q.shape[-1])
    if cap is not None:
        s = cap * torch.tanh(s / cap)
    if causal:
        s = s.masked_fill(j > i, float("-inf"))
    if window is not None:
        s = s.masked_fill(j <= i - window, float("-inf"))
    return torch.matmul(torch.softmax(s, dim=-1), v)


def _close(out, ref, what):
    allowed = FP32_TOL[0] + FP32_TOL[1] * ref.abs()
    over = ((out.double() - ref).abs() - allowed).max().item()
    assert over <= 0, f"{what}: {over:.3e} over the fp32 bound"


def _inputs(h, hkv, seed=0):
    g = torch.Generator().manual_seed(seed + 10 * h + hkv)
    qkv = 2.0 * torch.randn(B, S, h + 2 * hkv, D, generator=g)  # scores of std ~ 4: a cap of 2 bites
    do = torch.randn(B, S, h, D, generator=g)
    return qkv, do


def _oracle(qkv, do, h, hkv, cap, causal, window):
    """(o [B, S, H, D], dqkv) of the fp64 capped attention on repeated K/V heads (autograd sums each group)."""
    x = qkv.double().requires_grad_()
    q, k, v = (t.transpose(1, 2) for t in (x[:, :, :h], x[:, :, h:h + hkv], x[:, :, h + hkv:]))
    rep = h // hkv
    o = capped_attention_fp64(q, k.repeat_interleave(rep, 1), v.repeat_interleave(rep, 1), cap, causal, window)
    o.backward(do.double().transpose(1, 2))
    return o.detach().transpose(1, 2), x.grad


# ------------------------------------------------------------------ 1. the eager ops
@pytest.mark.parametrize("causal,window", [(False, None), (True, None), (True, 5)])
@pytest.mark.parametrize("h,hkv", [(4, 4), (4, 2), (6, 1)])
def test_eager_ops_against_fp64(h, hkv, causal, window):
    cap = 2.0
    qkv, do = _inputs(h, hkv)
    ref_o, ref_d = _oracle(qkv, do, h, hkv, cap, causal, window)
    un_o, _ = _oracle(qkv, do, h, hkv, None, causal, window)
    assert ((ref_o - un_o).abs() > 1e-2).double().mean() > 0.25  # the cap is visible
    x = qkv.clone().requires_grad_()
    o = ops.attention_gqa_packed(x, hkv, causal=causal, window=window, softcap=cap)
    o.backward(do)
    _close(o.detach(), ref_o, "attention_gqa_packed o")
    _close(x.grad, ref_d, "attention_gqa_packed dqkv")
    if h == hkv:
        x = qkv.clone().requires_grad_()
        o = ops.attention_packed(x.view(B, S, 3, h, D), causal=causal, window=window, softcap=cap)
        o.backward(do)
        _close(o.detach(), ref_o, "attention_packed o")
        _close(x.grad, ref_d, "attention_packed dqkv")
    q, k, v = (t.transpose(1, 2) for t in (qkv[:, :, :h], qkv[:, :, h:h + hkv], qkv[:, :, h + hkv:]))
    o = ops.attention(q, k, v, causal=causal, window=window, softcap=cap)
    _close(o.transpose(1, 2), ref_o, "attention o")
    rep = h // hkv
    o = ops.attention_reference(q, k.repeat_interleave(rep, 1), v.repeat_interleave(rep, 1), causal, 0.0,
                                window=window, softcap=cap)
    _close(o.transpose(1, 2), ref_o, "attention_reference o")


def test_no_cap_is_the_old_result_bit_for_bit():
    qkv, _ = _inputs(4, 2)
    a = ops.attention_gqa_packed(qkv, 2, causal=True)
    b = ops.attention_gqa_packed(qkv, 2, causal=True, softcap=None)
    assert torch.equal(a, b)
    big = ops.attention_gqa_packed(qkv, 2, causal=True, softcap=1e4)  # tanh is the identity at fp32 here
    _close(big, a.double(), "a huge cap")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cap", [1.0, 30.0])
def test_ops_softcap_eager(cap, dtype):
    g = torch.Generator().manual_seed(1)
    x = (3.0 * torch.randn(5, 37, generator=g)).to(dtype)
    dy = torch.randn(5, 37, generator=g).to(dtype)
    leaf = x.clone().requires_grad_()
    y = ops.softcap(leaf, cap)
    y.backward(dy)
    assert y.dtype == dtype and y.shape == x.shape
    ref = cap * torch.tanh(x.double() / cap)
    ref_dx = dy.double() * (1 - torch.tanh(x.double() / cap) ** 2)
    if dtype == torch.float32:
        _close(y.detach(), ref, "softcap")
        _close(leaf.grad, ref_dx, "softcap backward")
    else:
        assert torch.allclose(y.detach().double(), ref, atol=1e-4, rtol=2.0 ** -8)
        assert torch.allclose(leaf.grad.double(), ref_dx, atol=2e-2, rtol=2e-2)
    assert torch.equal(ops.softcap_reference(x, cap), y.detach())
    z = x.clone()
    assert ops.softcap(z, cap, inplace=True) is z and torch.equal(z, y.detach())


# ------------------------------------------------------------------ 2. bad values
@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("nan"), float("inf"), True, "50", [50.0]])
def test_bad_caps_raise(bad):
    qkv, _ = _inputs(4, 4)
    q, k, v = (t.transpose(1, 2) for t in qkv.view(B, S, 3, 4, D).unbind(2))
    with pytest.raises(ValueError, match="softcap"):
        ops.attention(q, k, v, causal=True, softcap=bad)
    with pytest.raises(ValueError, match="softcap"):
        ops.attention_packed(qkv.view(B, S, 3, 4, D), softcap=bad)
    with pytest.raises(ValueError, match="softcap"):
        ops.attention_gqa_packed(qkv, 4, softcap=bad)
    with pytest.raises(ValueError, match="softcap"):
        ops.attention_reference(q, k, v, True, 0.0, softcap=bad)
    with pytest.raises(ValueError, match="cap"):
        ops.softcap(qkv, bad)
    kw = dict(norm_first=True, causal=True, layer_norm_eps=1e-5)
    with pytest.raises(ValueError, match="attn_softcap"):
        AttentionCore(32, 4, 0.0, attn_softcap=bad, **kw)
    with pytest.raises(ValueError, match="attn_softcap"):
        SelfAttentionBlock(32, 4, 0.0, attn_softcap=bad)
    with pytest.raises(ValueError, match="attn_softcap"):
        TransformerEncoderLayer(32, 4, 64, attn_softcap=bad)
    with pytest.raises(ValueError, match="attn_softcap"):
        transformer_blocks(1, 32, 4, 64, 0.0, attn_softcap=bad)
    with pytest.raises(ValueError, match="final_softcap"):
        Decoder(100, 32, final_softcap=bad)


def test_int_caps_are_numbers():
    assert AttentionCore(32, 4, 0.0, norm_first=True, causal=False, layer_norm_eps=1e-5,
                         attn_softcap=50).attn_softcap == 50.0
    assert Decoder(100, 32, final_softcap=30).final_softcap == 30.0


# ------------------------------------------------------------------ 3. the options reach the modules
def test_lmconfig_caps_reach_every_core_and_the_decoder():
    cfg = softcap_engine.softcap_cfg()
    blocks = build_lm_blocks(cfg)
    cores = [b.core for b in blocks if isinstance(b, SelfAttentionBlock)]
    assert len(cores) == cfg.num_layers == 2 and all(c.attn_softcap == 0.5 and c.window == 3 for c in cores)
    assert isinstance(blocks[-1], Decoder) and blocks[-1].final_softcap == 1.0
    with torch.device("meta"):
        tiny = build_lm_blocks(CONFIGS["gemma2_tiny"])
    assert [b.core.attn_softcap for b in tiny if isinstance(b, SelfAttentionBlock)] == [50.0, 50.0]
    assert tiny[-1].final_softcap == 30.0
    plain = build_lm_blocks(dataclasses.replace(cfg, attn_softcap=None, final_softcap=None))
    assert all(b.core.attn_softcap is None for b in plain if isinstance(b, SelfAttentionBlock))
    assert plain[-1].final_softcap is None
    assert LMConfig("x", 1, 32, 4, 64, 100, 8).attn_softcap is None
    assert LMConfig("x", 1, 32, 4, 64, 100, 8).final_softcap is None


def test_decoder_final_cap_on_the_cpu():
    """The capped logits against the formula, the pad columns at exactly 0, and the gradients through autograd."""
    torch.manual_seed(0)
    dec = Decoder(100, 32, final_softcap=1.0)
    assert dec.padded == 256
    x = (8.0 * torch.randn(2, 5, 32)).requires_grad_()
    y = dec(x)
    assert y.shape == (2, 5, 100)
    raw = torch.nn.functional.linear(x.detach().double(), dec.weight.detach().double(), dec.bias.detach().double())
    _close(y.detach(), torch.tanh(raw[..., :100]), "capped logits")
    assert (raw[..., :100].abs() > 1.5).double().mean() > 0.25  # the cap bites
    full = ops.softcap(ops.linear(x.detach(), dec.weight.detach(), dec.bias.detach()), 1.0)
    assert torch.equal(full[..., 100:], torch.zeros_like(full[..., 100:]))
    y.square().sum().backward()
    xd = x.detach().double().requires_grad_()
    wd = dec.weight.detach().double().requires_grad_()
    torch.tanh(torch.nn.functional.linear(xd, wd, dec.bias.detach().double()))[..., :100].square().sum().backward()
    _close(x.grad, xd.grad, "dx")
    _close(dec.weight.grad, wd.grad, "dw")
    assert torch.equal(dec.weight.grad[100:], torch.zeros_like(dec.weight.grad[100:]))


def test_capped_model_forward_backward_runs():
    """A forward and backward of the replica on the CPU; both caps are really applied: the same weights without
    either give another loss."""
    cfg = softcap_engine.softcap_cfg()
    torch.manual_seed(0)
    model = torch.nn.Sequential(*build_lm_blocks(cfg)).train()
    tok = torch.randint(0, cfg.vocab, (4, cfg.seq_len + 1), generator=torch.Generator().manual_seed(7))
    x, t = tok[:, :-1], tok[:, 1:].contiguous()
    loss_fn = lambda y: ops.cross_entropy(y.reshape(-1, cfg.vocab), t.reshape(-1))  # noqa: E731
    loss = loss_fn(model(x))
    loss.backward()
    loss = float(loss.detach())
    assert math.isfinite(loss) and all(p.grad is not None and torch.isfinite(p.grad).all()
                                       for p in model.parameters())
    for b in model:
        if isinstance(b, SelfAttentionBlock):
            b.core.attn_softcap = None
    no_attn = float(loss_fn(model(x)).detach())
    model[-1].final_softcap = None
    no_caps = float(loss_fn(model(x)).detach())
    assert len({loss, no_attn, no_caps}) == 3


# ------------------------------------------------------------------ 4. the decoder split and the planner
def test_split_decoder_refuses_a_capped_decoder():
    with pytest.raises(ValueError, match="final_softcap"):
        split_decoder(Decoder(1000, 32, final_softcap=30.0))
    head, tail = split_decoder(Decoder(1000, 32))
    assert head is not None and tail is not None
    # lm_pipeline_units keeps such a decoder whole, whatever it is asked
    with torch.device("meta"):
        blocks = build_lm_blocks(CONFIGS["gemma2_tiny"])
        units = lm_pipeline_units(blocks, split_decoder=True)
        plain = lm_pipeline_units(build_lm_blocks(CONFIGS["mistral_tiny"]), split_decoder=True)
    assert isinstance(units[-1], Decoder) and len(plain) == len(units) + 1


def test_planner_offers_no_split_for_gemma2_tiny():
    cfg, base = CONFIGS["gemma2_tiny"], CONFIGS["mistral_tiny"]
    n = len(block_costs(cfg, False))
    for v in (1, 2):
        plan = plan_stages(cfg, 2, v, 8, split_decoder=True)
        assert plan.split_decoder is False and sum(plan.balance) == n
    assert plan_stages(base, 2, 1, 8, split_decoder=True).split_decoder is True
    asked = []

    def cost_fn(split):
        asked.append(split)
        return block_costs(cfg, split)

    v, plan = choose_virtual(cfg, 2, 8, split_options=(False, True), cost_fn=cost_fn)
    assert plan.split_decoder is False and asked and not any(asked)
    v, plan = choose_virtual(cfg, 2, 8, split_options=(True,))  # nothing else on offer: still no split
    assert plan.split_decoder is False


# ------------------------------------------------------------------ 5. the config and the costs
def test_gemma2_tiny_is_what_its_notes_say():
    cfg, base = CONFIGS["gemma2_tiny"], CONFIGS["mistral_tiny"]
    assert (cfg.attn_softcap, cfg.final_softcap) == (50.0, 30.0)
    assert (cfg.nhead, cfg.n_kv_heads, cfg.d_model // cfg.nhead, cfg.seq_len, cfg.window) == (4, 2, 64, 192, 48)
    assert dataclasses.replace(cfg, name=base.name, attn_softcap=None, final_softcap=None, notes=base.notes) == base
    assert "50" in cfg.notes and "30" in cfg.notes and "GeGLU" in cfg.notes
    assert cfg.params() == base.params()  # the caps add no parameters


def test_caps_add_no_flops():
    cfg, base = CONFIGS["gemma2_tiny"], CONFIGS["mistral_tiny"]
    assert block_costs(cfg) == block_costs(base)
    kw = dict(norm_first=True, causal=True, layer_norm_eps=1e-5, n_kv_heads=2)
    assert (AttentionCore(32, 4, 0.0, attn_softcap=50.0, **kw).flops_per_token(64)
            == AttentionCore(32, 4, 0.0, **kw).flops_per_token(64))
    assert Decoder(1000, 32, final_softcap=30.0).flops_per_token(64) == Decoder(1000, 32).flops_per_token(64)
    with torch.device("meta"):
        blk = build_lm_blocks(cfg)[1]
    assert block_flops(blk, cfg.seq_len) == 3.0 * blk.flops_per_token(cfg.seq_len)


# ------------------------------------------------------------------ 6. the engine, two gloo ranks
def test_capped_engine_two_gloo_ranks(monkeypatch):
    """helpers.engine_cases.run_engine_case as test_engine.py runs it, on the capped replica: the spawned ranks
    start in helpers.softcap_engine.worker, which swaps the helper's config and runs its worker."""
    monkeypatch.setattr(engine_cases, "case_cfg", softcap_engine.softcap_cfg)
    monkeypatch.setattr(engine_cases, "worker", softcap_engine.worker)
    engine_cases.run_engine_case("cpu", 2, "except_last", 1, False, False)
