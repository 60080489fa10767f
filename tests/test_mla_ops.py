"""Multi-head latent attention on the CPU: ``LatentAttentionCore`` against plain eager math, the ``mla=`` option
through the block builders and ``LMConfig``, and ``ops.attention``'s ``k_rope=`` against the concatenated call."""
import dataclasses
import math

import pytest
import torch

from mipipe import ops
from mipipe.models import CONFIGS, MLADims, build_lm_blocks, lm_pipeline_units
from mipipe.models.transformer import LatentAttentionCore, transformer_blocks
from mipipe.parallel.stage import block_costs

CFG = dataclasses.replace(CONFIGS["llama_tiny"], mla=MLADims(kv_lora_rank=64), nhead=2)


def _rms(x, w, eps):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w


def _eager(core, x):
    """linear, RMSNorm, split, rotate, cat, softmax: the core's math written out."""
    m, H, (B, S, _) = core.mla, core.nhead, x.shape
    h = _rms(x, core.norm_weight, core.eps)
    ckv = h @ core.kv_a_weight.T
    if m.q_lora_rank is None:
        q = h @ core.q_weight.T
    else:
        q = _rms(h @ core.q_a_weight.T, core.q_norm_weight, core.eps) @ core.q_b_weight.T
    q = q.view(B, S, H, m.nope_dim + m.rope_dim).transpose(1, 2)
    kv = (_rms(ckv[..., :m.kv_lora_rank], core.kv_norm_weight, core.eps) @ core.kv_b_weight.T)
    kv = kv.view(B, S, H, m.nope_dim + m.v_dim).transpose(1, 2)
    cos, sin = (t.double() for t in ops.rope_tables(S, m.rope_dim, core.rope_base))

    def rot(t):
        a, b = t[..., :m.rope_dim // 2], t[..., m.rope_dim // 2:]
        return torch.cat((a * cos - b * sin, b * cos + a * sin), -1)

    q = torch.cat((q[..., :m.nope_dim], rot(q[..., m.nope_dim:])), -1)
    k = torch.cat((kv[..., :m.nope_dim], rot(ckv[..., m.kv_lora_rank:])[:, None].expand(-1, H, -1, -1)), -1)
    s = q @ k.transpose(-1, -2) / math.sqrt(m.nope_dim + m.rope_dim)
    s = s.masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1), float("-inf"))
    return (torch.softmax(s, -1) @ kv[..., m.nope_dim:]).transpose(1, 2).reshape(B, S, H * m.v_dim)


@pytest.mark.parametrize("q_lora_rank", [None, 24])
def test_core_is_the_eager_composition(q_lora_rank):
    torch.manual_seed(0)
    mla = MLADims(kv_lora_rank=40, q_lora_rank=q_lora_rank, nope_dim=16, rope_dim=8, v_dim=24)
    core = LatentAttentionCore(48, 3, 0.0, mla=mla, norm_first=True, causal=True, layer_norm_eps=1e-5,
                               dtype=torch.float64)
    for p in core.parameters():  # norm weights off their initial ones
        p.data.add_(0.1 * torch.randn_like(p))
    x, do = torch.randn(2, 11, 48, dtype=torch.float64), torch.randn(2, 11, 72, dtype=torch.float64)
    outs = []
    for fn in (lambda t: core.forward_fanout(t, True)[0], lambda t: _eager(core, t)):
        xx = x.clone().requires_grad_()
        core.zero_grad()
        o = fn(xx)
        o.backward(do)
        outs.append([o.detach(), xx.grad] + [p.grad.clone() for p in core.parameters()])
    assert len(outs[0]) == 2 + (5 if q_lora_rank is None else 7)
    # the CPU attention op computes in fp32 whatever its inputs (2^-24 per operation, through a 24-term score, the
    # softmax and the chain of four GEMMs behind it): fp32's usual 1e-5 / 1e-4 rather than an fp64 bound
    for a, r in zip(*outs):
        torch.testing.assert_close(a, r, rtol=1e-4, atol=1e-5)


def test_mla_none_registers_nothing():
    kw = dict(norm_first=True, causal=True, norm="rms", bias=False, rope=True)
    names = lambda bs: [[n for n, _ in b.named_parameters()] + list(b.state_dict()) for b in bs]  # noqa: E731
    assert names(transformer_blocks(2, 64, 2, 128, 0.0, "swiglu", **kw)) == \
        names(transformer_blocks(2, 64, 2, 128, 0.0, "swiglu", mla=None, **kw))
    core = transformer_blocks(1, 64, 2, 128, 0.0, "swiglu", mla=MLADims(kv_lora_rank=32), **kw)[0].core
    assert isinstance(core, LatentAttentionCore) and core.attn_dim == 2 * 128
    assert sorted(n for n, _ in core.named_parameters()) == ["kv_a_weight", "kv_b_weight", "kv_norm_weight",
                                                             "norm_weight", "q_weight"]


@pytest.mark.parametrize("option", [dict(n_kv_heads=1), dict(head_dim=64), dict(window=8), dict(qk_norm=True),
                                    dict(attn_softcap=30.0), dict(attn_sinks=True), dict(rope=False),
                                    dict(norm="layer")])
def test_excluded_options_raise(option):
    with pytest.raises(ValueError, match="mla"):
        dataclasses.replace(CFG, **option)
    kw = {**dict(norm_first=True, causal=True, norm="rms", bias=False, rope=True), **option}
    with pytest.raises(ValueError, match="mla"):
        transformer_blocks(1, 64, 2, 128, 0.0, "swiglu", mla=CFG.mla, **kw)


def test_config_counts_and_costs():
    blocks = build_lm_blocks(CFG)
    real = sum(p.numel() for b in blocks for p in b.parameters())
    real -= (blocks[-1].padded - blocks[-1].ntoken) * (CFG.d_model + 1)  # the zero rows that pad the vocabulary
    assert CFG.params() == real and CFG.attn_dim() == 2 * 128
    costs, units = block_costs(CFG), lm_pipeline_units(blocks)
    assert len(costs) == len(units) == len(block_costs(CONFIGS["llama_tiny"]))
    assert [type(u).__name__ for u in units[1:5]] == ["PackedAttentionCore", "PackedAttentionOutput",
                                                      "PackedFeedForwardIn", "PackedFeedForwardOut"]
    core = blocks[1].core
    assert costs[1] == 3.0 * core.flops_per_token(CFG.seq_len) + 3.0 * 10 * CFG.d_model
    x = torch.randn(2, 16, CFG.d_model)  # the packed [.., E + A] boundary takes the core as it is
    assert torch.allclose(units[2](units[1](x)), blocks[1](x), atol=1e-6)


def test_documents_raise():
    core = build_lm_blocks(CFG)[1].core
    with ops.use_documents(torch.zeros(1, 2, 8, dtype=torch.int32)), pytest.raises(ValueError, match="document"):
        core(torch.randn(1, 8, CFG.d_model))


def test_k_rope_is_the_concatenated_call():
    torch.manual_seed(1)
    q, kn, v, kr = torch.randn(2, 3, 10, 24), torch.randn(2, 3, 10, 16), torch.randn(2, 3, 10, 12), torch.randn(2, 10, 8)
    kk = torch.cat([kn, kr[:, None].expand(-1, 3, -1, -1)], -1)
    for fn in (ops.attention, lambda *a, **kw: ops.attention_reference(*a, 0.0, **kw)):
        assert torch.equal(fn(q, kn, v, True, k_rope=kr), fn(q, kk, v, True))
    with pytest.raises(ValueError, match="k_rope"):
        ops.attention(q, kk, v, True, k_rope=kr)
