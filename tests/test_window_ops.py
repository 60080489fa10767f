"""Sliding-window attention on the CPU: the eager ops against an fp64 band-mask
attention built here, the window that covers the sequence, the errors, the
``mistral_*`` configs and their costs, and a windowed model through the
engine.  The HIP kernels behind the same keyword are tested in
test_gpu_window_kernels.py.

The CPU attention path (``ops.attention_reference``) computes in fp32 whatever
it is given, so the comparisons with the fp64 oracle are at the project's fp32
bound (``helpers.rowwise_cases.FP32_TOL``)."""
import dataclasses
import math

import pytest
import torch

from helpers import engine_cases, window_engine
from helpers.rowwise_cases import FP32_TOL

from mipipe import ops
from mipipe.models import CONFIGS, LMConfig, build_lm_blocks
from mipipe.models.transformer import (AttentionCore, SelfAttentionBlock, TransformerEncoderLayer, block_flops,
                                       transformer_blocks)
from mipipe.parallel.stage import block_costs

B, S, D = 2, 24, 16


def band_attention_fp64(q, k, v, window):
    """``[B, H, S, D]`` fp64 attention where query i sees the keys j with j <= i and j > i - window."""
    n = q.shape[-2]
    i = torch.arange(n, device=q.device)[:, None]
    j = torch.arange(n, device=q.device)[None, :]
    keep = (j <= i) & (j > i - window)
    s = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(q.shape[-1])
    s = s.masked_fill(~keep, float("-inf"))
    return torch.matmul(torch.softmax(s, dim=-1), v)


def _close(out, ref, what):
    allowed = FP32_TOL[0] + FP32_TOL[1] * ref.abs()
    over = ((out.double() - ref).abs() - allowed).max().item()
    assert over <= 0, f"{what}: {over:.3e} over the fp32 bound"


def _inputs(h, hkv, seed=0):
    g = torch.Generator().manual_seed(seed + 10 * h + hkv)
    qkv = torch.randn(B, S, h + 2 * hkv, D, generator=g)
    do = torch.randn(B, S, h, D, generator=g)
    return qkv, do


def _oracle(qkv, do, h, hkv, window):
    """(o [B, S, H, D], dqkv) of the fp64 band attention on repeated K/V heads (autograd sums each group)."""
    x = qkv.double().requires_grad_()
    q, k, v = (t.transpose(1, 2) for t in (x[:, :, :h], x[:, :, h:h + hkv], x[:, :, h + hkv:]))
    rep = h // hkv
    o = band_attention_fp64(q, k.repeat_interleave(rep, 1), v.repeat_interleave(rep, 1), window)
    o.backward(do.double().transpose(1, 2))
    return o.detach().transpose(1, 2), x.grad


# ------------------------------------------------------------------ 1. the eager ops against fp64
@pytest.mark.parametrize("window", [1, 5, 23])
@pytest.mark.parametrize("h,hkv", [(4, 4), (4, 2), (6, 2), (4, 1)])
def test_windowed_ops_against_fp64_band_attention(h, hkv, window):
    qkv, do = _inputs(h, hkv)
    ref_o, ref_d = _oracle(qkv, do, h, hkv, window)
    tag = f"H{h}/{hkv} W{window}"

    x = qkv.clone().requires_grad_()
    o = ops.attention_gqa_packed(x, hkv, causal=True, window=window)
    o.backward(do)
    _close(o, ref_o, tag + " attention_gqa_packed o")
    _close(x.grad, ref_d, tag + " attention_gqa_packed dqkv")

    leaves = [t.transpose(1, 2).clone().requires_grad_() for t in (qkv[:, :, :h], qkv[:, :, h:h + hkv],
                                                                    qkv[:, :, h + hkv:])]
    o = ops.attention(*leaves, causal=True, window=window)
    o.backward(do.transpose(1, 2))
    _close(o.transpose(1, 2), ref_o, tag + " attention o")
    for t, lo, hi, name in ((leaves[0], 0, h, "dq"), (leaves[1], h, h + hkv, "dk"), (leaves[2], h + hkv, None, "dv")):
        _close(t.grad.transpose(1, 2), ref_d[:, :, lo:hi], f"{tag} attention {name}")

    if hkv == h:
        x5 = qkv.view(B, S, 3, h, D).clone().requires_grad_()
        o = ops.attention_packed(x5, causal=True, window=window)
        o.backward(do)
        _close(o, ref_o, tag + " attention_packed o")
        _close(x5.grad.view_as(ref_d), ref_d, tag + " attention_packed dqkv")
        rl = [t.transpose(1, 2).clone().requires_grad_() for t in x5.detach().unbind(2)]
        o = ops.attention_reference(*rl, True, 0.0, window=window)
        o.backward(do.transpose(1, 2))
        _close(o.transpose(1, 2), ref_o, tag + " attention_reference o")
        for t, which in zip(rl, range(3)):
            _close(t.grad.transpose(1, 2), ref_d.view(B, S, 3, h, D)[:, :, which], f"{tag} attention_reference d{which}")
    if window == 1:  # a query sees itself only: o is v (of its group's head)
        rep = h // hkv
        assert torch.equal(ops.attention_gqa_packed(qkv, hkv, causal=True, window=1),
                           qkv[:, :, h + hkv:].repeat_interleave(rep, 2))


# ------------------------------------------------------------------ 2. a window that covers the sequence
@pytest.mark.parametrize("window", [24, 100])
def test_covering_window_is_plain_causal(window):
    qkv, _ = _inputs(4, 2, seed=3)
    assert torch.equal(ops.attention_gqa_packed(qkv, 2, causal=True, window=window),
                       ops.attention_gqa_packed(qkv, 2, causal=True, window=None))
    assert torch.equal(ops.attention_gqa_packed(qkv, 2, causal=True, window=None),
                       ops.attention_gqa_packed(qkv, 2, causal=True))
    q5, _ = _inputs(4, 4, seed=4)
    q5 = q5.view(B, S, 3, 4, D)
    assert torch.equal(ops.attention_packed(q5, causal=True, window=window), ops.attention_packed(q5, causal=True))
    q, k, v = (t.transpose(1, 2) for t in q5.unbind(2))
    assert torch.equal(ops.attention(q, k, v, causal=True, window=window), ops.attention(q, k, v, causal=True))
    assert torch.equal(ops.attention_reference(q, k, v, True, 0.0, window=window),
                       ops.attention_reference(q, k, v, True, 0.0))


# ------------------------------------------------------------------ 3. errors
@pytest.mark.parametrize("causal,window", [(False, 5), (True, 0), (True, -3), (False, 0)])
def test_bad_windows_raise(causal, window):
    qkv, _ = _inputs(4, 4)
    q5 = qkv.view(B, S, 3, 4, D)
    q, k, v = (t.transpose(1, 2) for t in q5.unbind(2))
    with pytest.raises(ValueError, match="window"):
        ops.attention_packed(q5, causal=causal, window=window)
    with pytest.raises(ValueError, match="window"):
        ops.attention_gqa_packed(_inputs(4, 2)[0], 2, causal=causal, window=window)
    with pytest.raises(ValueError, match="window"):
        ops.attention(q, k, v, causal=causal, window=window)
    with pytest.raises(ValueError, match="window"):
        ops.attention_reference(q, k, v, causal, 0.0, window=window)


def test_window_needs_a_causal_block():
    kw = dict(norm_first=True, layer_norm_eps=1e-5)
    with pytest.raises(ValueError, match="window"):
        AttentionCore(32, 4, 0.0, causal=False, window=4, **kw)
    with pytest.raises(ValueError, match="window"):
        AttentionCore(32, 4, 0.0, causal=True, window=0, **kw)
    with pytest.raises(ValueError, match="window"):
        SelfAttentionBlock(32, 4, 0.0, causal=False, window=4)
    with pytest.raises(ValueError, match="window"):
        TransformerEncoderLayer(32, 4, 64, 0.0, window=4)
    with pytest.raises(ValueError, match="window"):
        transformer_blocks(1, 32, 4, 64, 0.0, window=4)
    assert AttentionCore(32, 4, 0.0, causal=True, **kw).window is None


# ------------------------------------------------------------------ 4. configs and costs
def test_mistral_configs_are_what_the_names_say():
    tiny, base = CONFIGS["mistral_tiny"], CONFIGS["llama_gqa_tiny"]
    assert (tiny.seq_len, tiny.window, tiny.d_model // tiny.nhead) == (192, 48, 64)
    assert dataclasses.replace(tiny, name=base.name, seq_len=base.seq_len, window=None, notes=base.notes) == base
    c, l3 = CONFIGS["mistral_7b"], CONFIGS["llama3_8b"]
    assert (c.num_layers, c.d_model, c.nhead, c.n_kv_heads, c.dim_feedforward, c.vocab, c.seq_len, c.window,
            c.rope_base) == (32, 4096, 32, 8, 14336, 32000, 8192, 4096, 10000.0)
    assert dataclasses.replace(c, name=l3.name, vocab=l3.vocab, rope_base=l3.rope_base, window=None,
                               notes=l3.notes) == l3
    # the window adds no parameters
    assert c.params() == dataclasses.replace(l3, vocab=32000).params()
    assert LMConfig("x", 1, 32, 4, 64, 100, 8).window is None


def test_lmconfig_window_reaches_every_core():
    cfg = window_engine.window_cfg()
    blocks = build_lm_blocks(cfg)
    cores = [b.core for b in blocks if isinstance(b, SelfAttentionBlock)]
    assert len(cores) == cfg.num_layers == 2 and all(c.window == 3 and c.causal for c in cores)
    with torch.device("meta"):
        tiny = build_lm_blocks(CONFIGS["mistral_tiny"])
    assert [b.core.window for b in tiny if isinstance(b, SelfAttentionBlock)] == [48, 48]
    with pytest.raises(ValueError, match="window"):
        build_lm_blocks(dataclasses.replace(cfg, causal=False))


def test_windowed_model_forward_backward_runs():
    """A forward and backward of the replica on the CPU; the window is really applied: the same weights
    without it give another loss."""
    cfg = window_engine.window_cfg()
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
            b.core.window = cfg.seq_len  # covers the sequence: plain causal
    assert float(loss_fn(model(x)).detach()) != loss


def test_flops_per_token_prices_the_band():
    kw = dict(norm_first=True, causal=True, layer_norm_eps=1e-5, n_kv_heads=2)
    e, seq = 32, 64
    causal = AttentionCore(e, 4, 0.0, **kw)
    for w in (seq, seq + 1, 1000):
        assert AttentionCore(e, 4, 0.0, window=w, **kw).flops_per_token(seq) == causal.flops_per_token(seq)
    one = AttentionCore(e, 4, 0.0, window=1, **kw)
    assert one.flops_per_token(seq) == 2 * one.qkv_dim * e + 4 * e
    w = 16
    mid = AttentionCore(e, 4, 0.0, window=w, **kw)
    keys = (w * (w + 1) / 2 + (seq - w) * w) / seq
    assert mid.flops_per_token(seq) == 2 * mid.qkv_dim * e + 4 * keys * e
    assert one.flops_per_token(seq) < mid.flops_per_token(seq) < causal.flops_per_token(seq)
    # the stage planner's costs see it: only the attention cores get cheaper
    cfg = CONFIGS["mistral_tiny"]
    a, b = block_costs(cfg), block_costs(dataclasses.replace(cfg, window=None))
    assert len(a) == len(b)
    for i, (ca, cb) in enumerate(zip(a, b)):
        core = i % 4 == 1 and i < 1 + 4 * cfg.num_layers  # [Encoder, (core, out, mlp in, mlp out) x L, ...]
        assert (ca < cb) if core else (ca == cb), i
    with torch.device("meta"):
        blk = build_lm_blocks(cfg)[1]
    assert block_flops(blk, cfg.seq_len) == 3.0 * blk.flops_per_token(cfg.seq_len)


# ------------------------------------------------------------------ 5. the engine, two gloo ranks
def test_windowed_engine_two_gloo_ranks(monkeypatch):
    """helpers.engine_cases.run_engine_case as test_engine.py runs it, on the windowed replica: the spawned
    ranks start in helpers.window_engine.worker, which swaps the helper's config and runs its worker."""
    monkeypatch.setattr(engine_cases, "case_cfg", window_engine.window_cfg)
    monkeypatch.setattr(engine_cases, "worker", window_engine.worker)
    engine_cases.run_engine_case("cpu", 2, "except_last", 1, False, False)
