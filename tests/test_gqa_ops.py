"""Grouped-query attention on the CPU: the module against a multi-head one with
repeated K/V weight rows, the unchanged default, parameter counts and costs,
the eager ops, and a GQA model through ``Pipe`` and the engine.  The HIP
kernels behind the same ops are tested in test_gpu_gqa_kernels.py.

The CPU attention path (``ops.attention_reference``) computes in fp32 whatever
it is given, so the equivalence tests run in fp32 at the project's fp32 bound
(``helpers.rowwise_cases.FP32_TOL``), not in fp64."""
import copy
import dataclasses

import pytest
import torch

from helpers.rowwise_cases import FP32_TOL

from mipipe import Pipe, ops
from mipipe.models import CONFIGS, LMConfig, build_lm_blocks, lm_pipeline_units
from mipipe.models.transformer import (AttentionCore, SelfAttentionBlock, TransformerEncoderLayer, block_flops,
                                       transformer_blocks)
from mipipe.ops.rope import rope_heads_reference
from mipipe.optim import FlatAdam
from mipipe.parallel import PipelineEngine
from mipipe.parallel.stage import block_costs


def _close(out, ref, what):
    allowed = FP32_TOL[0] + FP32_TOL[1] * ref.abs()
    over = ((out - ref).abs() - allowed).max().item()
    assert over <= 0, f"{what}: {over:.3e} over the fp32 bound"


# ------------------------------------------------------------------ 1. module equivalence
E, H = 32, 4
D = E // H


def _expand_rows(t, hkv):
    """GQA projection rows [(H + 2 Hkv) D, ...] -> MHA rows [3 H D, ...]: K and V heads repeated per group."""
    g = H // hkv
    q, k, v = t[:H * D], t[H * D:(H + hkv) * D], t[(H + hkv) * D:]
    rep = lambda x: x.view(hkv, D, *x.shape[1:]).repeat_interleave(g, dim=0).reshape(H * D, *x.shape[1:])  # noqa: E731
    return torch.cat((q, rep(k), rep(v)))


def _group_sum(t, hkv):
    """MHA gradient rows [3 H D, ...] -> the GQA layout, K and V rows summed over each group."""
    g = H // hkv
    q, k, v = t[:H * D], t[H * D:2 * H * D], t[2 * H * D:]
    red = lambda x: x.view(hkv, g, D, *x.shape[1:]).sum(1).reshape(hkv * D, *x.shape[1:])  # noqa: E731
    return torch.cat((q, red(k), red(v)))


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("rope", [False, True])
@pytest.mark.parametrize("hkv", [2, 1])
def test_gqa_core_equals_mha_with_repeated_rows(hkv, rope, causal):
    kw = dict(norm_first=True, causal=causal, layer_norm_eps=1e-5, rope=rope)
    torch.manual_seed(0)
    gqa = AttentionCore(E, H, 0.0, n_kv_heads=hkv, **kw)
    mha = AttentionCore(E, H, 0.0, **kw)
    assert gqa.in_proj_weight.shape == ((H + 2 * hkv) * D, E) and gqa.in_proj_bias.shape == ((H + 2 * hkv) * D,)
    with torch.no_grad():
        gqa.in_proj_bias.copy_(0.1 * torch.randn(gqa.in_proj_bias.shape))
        mha.in_proj_weight.copy_(_expand_rows(gqa.in_proj_weight, hkv))
        mha.in_proj_bias.copy_(_expand_rows(gqa.in_proj_bias, hkv))
        mha.norm_weight.copy_(gqa.norm_weight)
        mha.norm_bias.copy_(gqa.norm_bias)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 8, E, generator=g)
    do = torch.randn(2, 8, E, generator=g)
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    oa, ob = gqa(xa), mha(xb)
    _close(oa, ob.detach(), "output")
    oa.backward(do)
    ob.backward(do)
    _close(xa.grad, xb.grad, "dx")
    _close(gqa.in_proj_weight.grad, _group_sum(mha.in_proj_weight.grad, hkv), "in_proj_weight.grad")
    _close(gqa.in_proj_bias.grad, _group_sum(mha.in_proj_bias.grad, hkv), "in_proj_bias.grad")


# ------------------------------------------------------------------ 2. default unchanged
@pytest.mark.parametrize("rope", [False, True])
def test_default_n_kv_heads_is_plain_mha(rope):
    x = torch.randn(2, 8, E, generator=torch.Generator().manual_seed(2))

    def build(**kw):
        torch.manual_seed(3)
        return TransformerEncoderLayer(E, H, 64, 0.0, norm_first=True, causal=True, rope=rope, **kw).eval()

    base = build()
    y0 = base(x)
    for kw in ({"n_kv_heads": None}, {"n_kv_heads": H}):
        other = build(**kw)
        assert [(n, p.shape) for n, p in other.named_parameters()] == [(n, p.shape) for n, p in base.named_parameters()]
        assert torch.equal(other(x), y0), kw
    blocks = transformer_blocks(1, E, H, 64, 0.0, n_kv_heads=2)
    assert isinstance(blocks[0], SelfAttentionBlock) and blocks[0].core.n_kv_heads == 2
    assert blocks[0].core.in_proj_weight.shape == ((H + 4) * D, E)


# ------------------------------------------------------------------ 3. counts and costs
def _decoder_padding(cfg):
    """Zero rows (weight and bias) that pad the decoder's vocabulary to a multiple of 256."""
    return ((cfg.vocab + 255) // 256 * 256 - cfg.vocab) * (cfg.d_model + 1)


@pytest.mark.parametrize("name", ["llama_gqa_tiny", "llama3_8b"])
def test_params_matches_built_gqa_model(name):
    cfg = CONFIGS[name]
    with torch.device("meta"):
        blocks = build_lm_blocks(cfg)
    count = sum(p.numel() for b in blocks for p in b.parameters())
    assert cfg.params() == count - _decoder_padding(cfg)
    assert len(block_costs(cfg)) == len(lm_pipeline_units(blocks))


def test_gqa_configs_are_what_the_names_say():
    tiny, base = CONFIGS["llama_gqa_tiny"], CONFIGS["llama_tiny"]
    assert (tiny.nhead, tiny.n_kv_heads, tiny.d_model // tiny.nhead) == (4, 2, 64)
    assert dataclasses.replace(tiny, name=base.name, n_kv_heads=None, notes=base.notes) == base
    c = CONFIGS["llama3_8b"]
    assert (c.num_layers, c.d_model, c.nhead, c.n_kv_heads, c.dim_feedforward, c.vocab, c.rope_base, c.seq_len) == (
        32, 4096, 32, 8, 14336, 128256, 500000.0, 8192)
    # the published 8,030,261,248 (untied embedding and output matrices) plus the decoder's 128,256 bias entries
    assert c.params() == 8_030_261_248 + 128_256
    assert CONFIGS["llama2_7b"].n_kv_heads is None and CONFIGS["llama2_7b"].qkv_dim() == 3 * 4096


def test_costs_shrink_by_the_projections_share():
    cfg = CONFIGS["llama_gqa_tiny"]
    mha = dataclasses.replace(cfg, n_kv_heads=None)
    e, d = cfg.d_model, cfg.d_model // cfg.nhead
    saved = 2 * (cfg.nhead - cfg.n_kv_heads) * d  # projection columns GQA does not compute
    a, b = block_costs(cfg), block_costs(mha)
    assert len(a) == len(b)
    for i, (ca, cb) in enumerate(zip(a, b)):
        core = i % 4 == 1 and i < 1 + 4 * cfg.num_layers  # [Encoder, (core, out, mlp in, mlp out) x L, ...]
        assert cb - ca == (3.0 * 2 * saved * e if core else 0.0), i
    with torch.device("meta"):
        ga, gb = build_lm_blocks(cfg)[1], build_lm_blocks(mha)[1]
    assert gb.flops_per_token(cfg.seq_len) - ga.flops_per_token(cfg.seq_len) == 2 * saved * e
    assert block_flops(gb, cfg.seq_len) - block_flops(ga, cfg.seq_len) == 3.0 * 2 * saved * e  # forward x 3


# ------------------------------------------------------------------ 4. errors
def test_non_dividing_n_kv_heads_raises():
    for bad in (3, 0, 8):
        with pytest.raises(ValueError, match="n_kv_heads"):
            AttentionCore(E, H, 0.0, norm_first=True, causal=True, layer_norm_eps=1e-5, n_kv_heads=bad)
    with pytest.raises(ValueError, match="n_kv_heads"):
        build_lm_blocks(dataclasses.replace(CONFIGS["llama_gqa_tiny"], n_kv_heads=3))
    with pytest.raises(ValueError):
        ops.attention_gqa_packed(torch.randn(1, 4, 7, 8), 2)  # 7 - 4 = 3 query heads over 2 K/V heads
    with pytest.raises(ValueError):
        ops.attention(torch.randn(1, 4, 4, 8), torch.randn(1, 3, 4, 8), torch.randn(1, 3, 4, 8))


def test_load_from_torch_refuses_gqa():
    layer = TransformerEncoderLayer(E, H, 64, 0.0, n_kv_heads=2)
    with pytest.raises(ValueError, match="grouped-query"):
        layer.load_from_torch(torch.nn.TransformerEncoderLayer(E, H, 64, 0.0, batch_first=True))


# ------------------------------------------------------------------ 5. eager ops
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("h,hkv", [(4, 2), (4, 1), (6, 2), (4, 4)])
def test_eager_gqa_ops_equal_reference_on_repeated_heads(h, hkv, causal):
    B, S, d = 2, 8, 16
    g = torch.Generator().manual_seed(h * 10 + hkv)
    qkv = torch.randn(B, S, h + 2 * hkv, d, generator=g)
    q, k, v = (t.transpose(1, 2) for t in (qkv[:, :, :h], qkv[:, :, h:h + hkv], qkv[:, :, h + hkv:]))
    rep = h // hkv
    ref = ops.attention_reference(q, k.repeat_interleave(rep, 1), v.repeat_interleave(rep, 1), causal, 0.0)
    out = ops.attention_gqa_packed(qkv, hkv, causal=causal)
    assert out.shape == (B, S, h, d)
    # the same fp32 arithmetic on tensors laid out differently (a stacked copy against permuted views), so the
    # CPU matmul may block and round differently: the fp32 bound, not bit equality
    _close(out, ref.transpose(1, 2), "attention_gqa_packed")
    _close(ops.attention(q, k, v, causal=causal), ref, "attention")
    # the gradient of a shared K/V head is the sum over its group
    qs = qkv.clone().requires_grad_()
    ops.attention_gqa_packed(qs, hkv, causal=causal).square().sum().backward()
    leaves = [t.detach().clone().requires_grad_() for t in (q, k.repeat_interleave(rep, 1), v.repeat_interleave(rep, 1))]
    ops.attention_reference(*leaves, causal, 0.0).square().sum().backward()
    dk = leaves[1].grad.view(B, hkv, rep, S, d).sum(2).transpose(1, 2)
    dv = leaves[2].grad.view(B, hkv, rep, S, d).sum(2).transpose(1, 2)
    _close(qs.grad[:, :, :h], leaves[0].grad.transpose(1, 2), "dq")
    _close(qs.grad[:, :, h:h + hkv], dk, "dk")
    _close(qs.grad[:, :, h + hkv:], dv, "dv")


@pytest.mark.parametrize("pos0", [0, 3])
def test_rope_heads_reference_rotates_q_and_k_parts(pos0):
    B, S, h, hkv, d = 2, 8, 4, 2, 16
    x = torch.randn(B, S, h + 2 * hkv, d, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    cos, sin = ops.rope_tables(pos0 + S, d)
    out = ops.rope_heads(x, cos, sin, h + hkv, pos0)  # CPU tensors take the reference
    assert torch.equal(out, rope_heads_reference(x, cos, sin, h + hkv, pos0))

    def part(lo, hi):  # the same heads through the [B, S, 3, n, D] reference, as its Q part
        n = hi - lo
        five = torch.stack((x[:, :, lo:hi],) * 3, dim=2)
        return ops.rope_reference(five, cos, sin, pos0)[:, :, 0], n

    assert torch.equal(out[:, :, :h], part(0, h)[0])
    assert torch.equal(out[:, :, h:h + hkv], part(h, h + hkv)[0])
    assert torch.equal(out[:, :, h + hkv:], x[:, :, h + hkv:])
    proj = x.reshape(B, S, -1).float()
    via = ops.rope_projection(proj, cos, sin, h, pos0, n_kv_heads=hkv)
    assert via.shape == (B, S, h + 2 * hkv, d)
    assert torch.equal(via, rope_heads_reference(proj.view(B, S, h + 2 * hkv, d), cos, sin, h + hkv, pos0))
    assert torch.autograd.gradcheck(lambda t: ops.rope_heads(t, cos.double(), sin.double(), h + hkv, pos0),
                                    (x[:1, :3].clone().requires_grad_(),))


# ------------------------------------------------------------------ 6. the model, Pipe and the engine
def _cfg(**kw):
    return dataclasses.replace(CONFIGS["llama_gqa_tiny"], d_model=32, nhead=4, n_kv_heads=2, dim_feedforward=64,
                               vocab=100, seq_len=8, **kw)


def _data(cfg, n, seed=7):
    tok = torch.randint(0, cfg.vocab, (n, cfg.seq_len + 1), generator=torch.Generator().manual_seed(seed))
    return tok[:, :-1], tok[:, 1:].contiguous()


def _loss_fn(cfg):
    return lambda y, t: ops.cross_entropy(y.reshape(-1, cfg.vocab), t.reshape(-1))


def _blocks(cfg):
    torch.manual_seed(0)
    return build_lm_blocks(cfg)


def _run(seq, cfg, x, t):
    loss = _loss_fn(cfg)(seq(x), t)
    loss.backward()
    return float(loss.detach()), [p.grad.clone() for p in seq.parameters()]


def _assert_rel(a, b, what, rel=1e-5):
    scale = b.abs().max().item() + 1e-12
    assert (a - b).abs().max().item() <= rel * scale, what


def test_lmconfig_field_and_built_model():
    cfg = _cfg()
    assert isinstance(cfg, LMConfig) and cfg.qkv_dim() == (4 + 2 * 2) * 8
    blocks = _blocks(cfg)
    assert blocks[1].core.in_proj_weight.shape == (cfg.qkv_dim(), cfg.d_model) and blocks[1].core.in_proj_bias is None
    assert blocks[1].core.n_kv_heads == 2


@pytest.mark.parametrize("checkpoint", ["never", "always"])
def test_gqa_pipe_two_cpu_partitions(checkpoint):
    cfg = _cfg()
    x, t = _data(cfg, 8)
    blocks = _blocks(cfg)
    ref = torch.nn.Sequential(*copy.deepcopy(blocks)).train()
    loss0, g0 = _run(ref, cfg, x, t)
    model = torch.nn.Sequential(*blocks).train()
    pipe = Pipe(model, chunks=4, checkpoint=checkpoint, balance=[3, len(blocks) - 3], copy_same_device=True)
    try:
        loss = _loss_fn(cfg)(pipe(x).local_value(), t)
        loss.backward()
    finally:
        pipe.close()
    assert abs(float(loss.detach()) - loss0) <= 1e-5 * abs(loss0)
    for (n, p), b in zip(model.named_parameters(), g0):
        _assert_rel(p.grad, b, n)


def test_gqa_engine_single_rank_flat_adam():
    """One engine step on the GQA model.  (The multi-rank gloo helper, helpers/engine_cases.py, builds
    its own fixed config in every spawned rank and takes none from the caller, so the engine runs
    here on one rank, as test_llama_ops.py does for llama_tiny.)"""
    cfg = _cfg()
    m, mb = 3, 2
    x, t = _data(cfg, m * mb)
    ref = torch.nn.Sequential(*_blocks(cfg)).train()
    loss0, g0 = _run(ref, cfg, x, t)
    model = torch.nn.Sequential(*_blocks(cfg)).train()
    opt = FlatAdam(model.parameters(), lr=1e-3)
    eng = PipelineEngine(model, chunks=m, checkpoint="except_last", act_shape=(mb, cfg.seq_len),
                         act_dtype=torch.float32, loss_fn=_loss_fn(cfg), device=torch.device("cpu"))
    opt.zero_grad()
    st = eng.step(list(x.split(mb)), list(t.split(mb)))
    opt.fold_grads()
    assert abs(float(st.loss) - loss0) <= 1e-5 * abs(loss0)
    for (n, p), b in zip(model.named_parameters(), g0):
        _assert_rel(p.main_grad, b, n)
