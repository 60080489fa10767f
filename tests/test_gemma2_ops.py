"""The Gemma-2 block on the CPU: the two new eager references (``ops.geglu_reference``,
``ops.rms_norm_residual_reference``) against formulas written out here in fp64, the options'
refusals, the new configs' accounting (parameters, per-layer windows, unit kinds, unit costs, stage
boundary shapes), a 2-layer replica of ``gemma2_block_tiny`` against an independent eager Gemma-2
layer written in this file, and that replica through the engine on two gloo ranks with the stage
boundary between a decoupled attention core and its output.  The HIP kernels behind the same ops
are tested in test_gpu_gemma2_kernels.py.

The references compute in fp32 at least, so fp32 inputs are compared at the project's fp32 bound
(``helpers.rowwise_cases.FP32_TOL``) and fp64 inputs, where reference and formula do the same
arithmetic in another order, at 1e-12."""
import dataclasses
import math

import pytest
import torch

from helpers import engine_cases, gemma2_engine
from helpers.rowwise_cases import FP32_TOL

from mipipe import ops
from mipipe.models import CONFIGS, LMConfig, build_lm_blocks
from mipipe.models.transformer import (AttentionCore, AttentionOutput, FeedForwardBlock, FeedForwardIn,
                                       FeedForwardOut, SelfAttentionBlock, TransformerEncoderLayer, merge_units,
                                       pipeline_units, transformer_blocks)
from mipipe.parallel.stage import StagePlan, block_costs, stage_input_shape, unit_is_packed_core, unit_kind

GEMMA2 = ["gemma2_block_tiny", "gemma2_2b", "gemma2_9b", "gemma2_27b"]
EPS = 1e-5


def _close(out, ref, dtype, what):
    if dtype == torch.float64:
        allowed = 1e-12 * (1 + ref.abs())
    else:
        allowed = FP32_TOL[0] + FP32_TOL[1] * ref.abs()
    assert torch.isfinite(out).all(), what
    over = ((out.double() - ref).abs() - allowed).max().item()
    assert over <= 0, f"{what}: {over:.3e} over the {dtype} bound"


def gelu_tanh_fp64(g):
    return 0.5 * g * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (g + 0.044715 * g ** 3)))


def rms_fp64(x, w, eps=EPS):
    return x / torch.sqrt((x * x).mean(-1, keepdim=True) + eps) * w


# ------------------------------------------------------------------ 1. the references
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_geglu_reference_against_formula(dtype):
    g = torch.Generator().manual_seed(0)
    gu = (torch.randn(5, 3, 32, generator=g, dtype=torch.float64) * 3).to(dtype)
    dh = torch.randn(5, 3, 16, generator=g, dtype=torch.float64).to(dtype)
    gd = gu.clone().double().requires_grad_()
    ref = gelu_tanh_fp64(gd[..., :16]) * gd[..., 16:]
    ref.backward(dh.double())
    for op in (ops.geglu_reference, ops.geglu):  # CPU tensors: the op IS the reference
        gs = gu.clone().requires_grad_()
        h = op(gs)
        assert h.shape == (5, 3, 16) and h.dtype == dtype
        h.backward(dh)
        _close(h.detach(), ref.detach(), dtype, "h")
        _close(gs.grad, gd.grad, dtype, "dgu")
    with pytest.raises(ValueError, match="gate and up"):
        ops.geglu(torch.randn(2, 7))


def test_geglu_reference_dead_gate():
    """A gate of -inf: h = 0 and a zero gradient in both halves, no NaN anywhere."""
    gu = torch.randn(3, 16)
    gu[1, 2] = float("-inf")
    gs = gu.clone().requires_grad_()
    h = ops.geglu_reference(gs)
    h.backward(torch.ones_like(h))
    assert torch.isfinite(h).all() and torch.isfinite(gs.grad).all()
    assert h[1, 2].item() == 0.0 and gs.grad[1, 2].item() == 0.0 and gs.grad[1, 8 + 2].item() == 0.0
    assert gs.grad[1, 3].item() != 0.0


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_rms_norm_residual_reference_against_formula(dtype):
    g = torch.Generator().manual_seed(1)
    x = (2 * torch.randn(4, 5, 24, generator=g, dtype=torch.float64)).to(dtype)
    res = torch.randn(4, 5, 24, generator=g, dtype=torch.float64).to(dtype)
    w = (1 + 0.3 * torch.randn(24, generator=g, dtype=torch.float64)).to(dtype)
    dy = torch.randn(4, 5, 24, generator=g, dtype=torch.float64).to(dtype)
    xd, rd, wd = (t.clone().double().requires_grad_() for t in (x, res, w))
    ref = rd + rms_fp64(xd, wd)
    ref.backward(dy.double())
    for op in (ops.rms_norm_residual_reference, ops.rms_norm_residual):
        xs, rs, ws = (t.clone().requires_grad_() for t in (x, res, w))
        y = op(xs, rs, ws, EPS)
        assert y.shape == x.shape and y.dtype == dtype
        y.backward(dy)
        _close(y.detach(), ref.detach(), dtype, "y")
        _close(xs.grad, xd.grad, dtype, "dx")
        _close(ws.grad, wd.grad, dtype, "dgamma")
        assert torch.equal(rs.grad, dy)
    # the statistics come from x alone: another residual moves y by exactly the difference
    y0 = ops.rms_norm_residual(x.double(), torch.zeros_like(res).double(), w.double(), EPS)
    _close(y0, ref.detach() - res.double(), torch.float64, "zero residual")
    with pytest.raises(ValueError, match="differ"):
        ops.rms_norm_residual(x, res[:, :4], w, EPS)


def test_rms_norm_residual_reference_computes_bf16_in_fp32():
    g = torch.Generator().manual_seed(2)
    x, res = (torch.randn(6, 64, generator=g).bfloat16() for _ in range(2))
    w = (1 + 0.1 * torch.randn(64, generator=g)).bfloat16()
    y = ops.rms_norm_residual_reference(x, res, w, EPS)
    assert y.dtype == torch.bfloat16
    ref = res.double() + rms_fp64(x.double(), w.double())
    over = ((y.double() - ref).abs() - (2.0 ** -8 * ref.abs() + FP32_TOL[0])).max().item()
    assert over <= 0, over


# ------------------------------------------------------------------ 2. the options' refusals and defaults
KW = dict(norm_first=True, layer_norm_eps=1e-5, norm="rms", bias=False)


@pytest.mark.parametrize("bad", [dict(norm_first=False), dict(norm="layer"), dict(dropout=0.1)])
def test_sandwich_norm_refusals(bad):
    kw = dict(KW, dropout=0.0)
    kw.update(bad)
    p = kw.pop("dropout")
    with pytest.raises(ValueError, match="sandwich_norm"):
        AttentionOutput(32, p, sandwich_norm=True, **kw)
    with pytest.raises(ValueError, match="sandwich_norm"):
        FeedForwardOut(32, 64, p, sandwich_norm=True, **kw)
    kw.pop("layer_norm_eps")
    with pytest.raises(ValueError, match="sandwich_norm"):
        SelfAttentionBlock(32, 4, p, sandwich_norm=True, **kw)
    with pytest.raises(ValueError, match="sandwich_norm"):
        FeedForwardBlock(32, 64, p, "geglu", sandwich_norm=True, **kw)
    with pytest.raises(ValueError, match="sandwich_norm"):
        TransformerEncoderLayer(32, 4, 64, p, "geglu", sandwich_norm=True, **kw)
    with pytest.raises(ValueError, match="sandwich_norm"):
        transformer_blocks(1, 32, 4, 64, p, "geglu", sandwich_norm=True, **kw)


def test_post_norm_weight_is_a_plain_parameter_of_ones():
    out = AttentionOutput(32, 0.0, sandwich_norm=True, attn_dim=64, **KW)
    fc = FeedForwardOut(32, 64, 0.0, sandwich_norm=True, **KW)
    assert out.out_proj_weight.shape == (32, 64)
    for mod in (out, fc):
        assert mod.post_norm_weight.shape == (32,) and torch.equal(mod.post_norm_weight, torch.ones(32))
        assert not getattr(mod.post_norm_weight, "_mipipe_gemm_weight", False)
        with torch.no_grad():
            mod.post_norm_weight.fill_(3.0)
        mod.reset_parameters()
        assert torch.equal(mod.post_norm_weight, torch.ones(32))
    # off: no such parameter, the state dict keys of before
    assert set(AttentionOutput(32, 0.0, **KW).state_dict()) == {"out_proj_weight"}
    assert set(FeedForwardOut(32, 64, 0.0, **KW).state_dict()) == {"linear2_weight"}


def test_head_dim_and_global_every_refusals():
    with pytest.raises(ValueError, match="divisible"):
        SelfAttentionBlock(30, 4, 0.0)
    blk = SelfAttentionBlock(30, 4, 0.0, head_dim=16)  # the check applies only without head_dim
    assert blk.core.in_proj_weight.shape == (3 * 64, 30) and blk.out.out_proj_weight.shape == (30, 64)
    for bad in (0, -8, True, 2.0):
        with pytest.raises(ValueError, match="head_dim"):
            AttentionCore(32, 4, 0.0, causal=True, head_dim=bad, **KW)
    for bad in (0.0, -1.0, float("inf"), True):
        with pytest.raises(ValueError, match="attn_scale"):
            AttentionCore(32, 4, 0.0, causal=True, attn_scale=bad, **KW)
    for bad in (1, 0, True):
        with pytest.raises(ValueError, match="global_every"):
            transformer_blocks(2, 32, 4, 64, 0.0, causal=True, window=3, global_every=bad)
        with pytest.raises(ValueError, match="global_every"):
            LMConfig("x", 2, 32, 4, 64, 100, 8, causal=True, window=3, global_every=bad)
    with pytest.raises(ValueError, match="needs a window"):
        transformer_blocks(2, 32, 4, 64, 0.0, causal=True, global_every=2)
    with pytest.raises(ValueError, match="needs a window"):
        LMConfig("x", 2, 32, 4, 64, 100, 8, causal=True, global_every=2)


def test_geglu_is_a_gated_activation():
    fc = FeedForwardIn(32, 64, 0.0, "geglu", **KW)
    assert fc.linear1_weight.shape == (128, 32)
    assert fc.flops_per_token(8) == FeedForwardIn(32, 64, 0.0, "swiglu", **KW).flops_per_token(8) == 2 * 32 * 128
    fc.dropout = 0.1
    with pytest.raises(ValueError, match="geglu"):
        fc.train()(torch.randn(2, 4, 32))
    fc.dropout = 0.0
    x = torch.randn(2, 4, 32)
    gu = ops.rms_norm_reference(x, None, fc.norm_weight, 1e-5, 0.0, True) @ fc.linear1_weight.T
    assert torch.allclose(fc(x), torch.nn.functional.gelu(gu[..., :64], approximate="tanh") * gu[..., 64:],
                          atol=1e-6)
    a = dataclasses.replace(CONFIGS["llama_tiny"], activation="geglu")
    assert a.params() == CONFIGS["llama_tiny"].params()
    assert block_costs(a) == block_costs(CONFIGS["llama_tiny"])


def test_keywords_reach_every_layer_of_the_builders():
    kw = dict(norm_first=True, causal=True, norm="rms", bias=False, rope=True, n_kv_heads=2, window=3,
              sandwich_norm=True, head_dim=16, attn_scale=0.3)
    blocks = transformer_blocks(6, 32, 4, 64, 0.0, "geglu", global_every=3, **kw)
    attn = [b for b in blocks if isinstance(b, SelfAttentionBlock)]
    mlps = [b for b in blocks if isinstance(b, FeedForwardBlock)]
    assert [b.core.window for b in attn] == [3, 3, None, 3, 3, None]
    assert all(b.core.head_dim == 16 and b.core.attn_dim == 64 and b.core.attn_scale == 0.3 for b in attn)
    assert all(b.core.in_proj_weight.shape == (8 * 16, 32) and b.core.rope_cos.shape[1] == 8 for b in attn)
    assert all(b.out.sandwich_norm and b.out.attn_dim == 64 for b in attn)
    assert all(b.fc_out.sandwich_norm and b.fc_in.activation == "geglu" for b in mlps)
    layer = TransformerEncoderLayer(32, 4, 64, 0.0, "geglu", **kw)
    assert layer[0].out.sandwich_norm and layer[1].fc_out.sandwich_norm and layer[0].core.head_dim == 16
    # defaults: today's modules
    plain = transformer_blocks(2, 32, 4, 64, 0.0, causal=True, window=3)
    assert [b.core.window for b in plain if isinstance(b, SelfAttentionBlock)] == [3, 3]
    assert all(b.core.attn_scale is None and b.core.head_dim == 8 and not b.out.sandwich_norm
               for b in plain if isinstance(b, SelfAttentionBlock))
    assert AttentionCore(32, 4, 0.0, causal=True, **KW).flops_per_token(8) == 2 * 96 * 32 + 4 * 4 * 32
    core = AttentionCore(32, 4, 0.0, causal=True, head_dim=16, **KW)
    assert core.flops_per_token(8) == 2 * 192 * 32 + 4 * 4 * 64
    assert AttentionOutput(32, 0.0, attn_dim=64, **KW).flops_per_token(8) == 2 * 32 * 64


# ------------------------------------------------------------------ 3. configs and accounting
def test_gemma2_configs_are_what_the_names_say():
    sizes = {"gemma2_2b": (26, 2304, 8, 4, 256, 9216), "gemma2_9b": (42, 3584, 16, 8, 256, 14336),
             "gemma2_27b": (46, 4608, 32, 16, 128, 36864), "gemma2_block_tiny": (4, 256, 4, 2, 128, 512)}
    for name, want in sizes.items():
        c = CONFIGS[name]
        assert (c.num_layers, c.d_model, c.nhead, c.n_kv_heads, c.head_dim, c.dim_feedforward) == want, name
        assert (c.activation, c.sandwich_norm, c.global_every, c.attn_softcap, c.final_softcap, c.norm, c.bias,
                c.rope, c.rope_base, c.causal, c.norm_first, c.positions, c.dropout, c.scale_embedding) == (
            "geglu", True, 2, 50.0, 30.0, "rms", False, True, 10000.0, True, True, "none", 0.0, True), name
        assert all(word in c.notes for word in ("untied", "bias", "1e-5", "1 + w")), name
        if name != "gemma2_block_tiny":
            assert (c.vocab, c.seq_len, c.window) == (256000, 8192, 4096)
    tiny = CONFIGS["gemma2_block_tiny"]
    assert (tiny.vocab, tiny.seq_len, tiny.window, tiny.attn_scale) == (1000, 192, 48, 0.125)
    assert tiny.attn_scale == (tiny.d_model / tiny.nhead) ** -0.5 != tiny.head_dim ** -0.5
    assert tiny.attn_dim() == 512 != tiny.d_model and tiny.qkv_dim() == 8 * 128
    assert CONFIGS["gemma2_27b"].attn_scale == 144 ** -0.5
    assert CONFIGS["gemma2_2b"].attn_scale is None and CONFIGS["gemma2_9b"].attn_scale is None
    old = CONFIGS["gemma2_tiny"]
    assert (old.activation, old.sandwich_norm, old.head_dim, old.global_every) == ("swiglu", False, None, None)
    assert "no full-size" not in old.notes.lower() and "not a gemma-2 size" not in old.notes.lower()


@pytest.mark.parametrize("name", GEMMA2)
def test_params_equals_the_built_model(name):
    cfg = CONFIGS[name]
    with torch.device("meta"):
        blocks = build_lm_blocks(cfg)
    real = sum(p.numel() for b in blocks for p in b.parameters())
    dec = blocks[-1]
    real -= (dec.padded - dec.ntoken) * (cfg.d_model + 1)  # the zero rows that pad the vocabulary
    assert cfg.params() == real
    e, a, f, L = cfg.d_model, cfg.attn_dim(), cfg.dim_feedforward, cfg.num_layers
    layer = (cfg.qkv_dim() + a) * e + 4 * e + 3 * f * e  # two pre-norms, two post-norms, the 2F gate
    assert cfg.params() == L * layer + e + 2 * cfg.vocab * e + cfg.vocab
    cores = [b.core for b in blocks if isinstance(b, SelfAttentionBlock)]
    assert [c.window for c in cores] == [cfg.window, None] * (L // 2)
    assert all(c.attn_scale == cfg.attn_scale and c.attn_softcap == 50.0 for c in cores)


def test_layer_window_unit_kinds_and_costs():
    cfg = CONFIGS["gemma2_block_tiny"]
    assert [cfg.layer_window(i) for i in range(4)] == [48, None, 48, None]
    g3 = dataclasses.replace(cfg, num_layers=12, global_every=6)  # Gemma-3's five local, one global
    assert [i for i in range(12) if g3.layer_window(i) is None] == [5, 11]
    costs = block_costs(cfg)
    kinds = [unit_kind(cfg, i) for i in range(len(costs))]
    assert kinds == ["enc"] + ["core", "out", "mlp_in", "mlp_out", "core_global", "out", "mlp_in", "mlp_out"] * 2 + [
        "norm", "dec"]
    assert [unit_is_packed_core(cfg, i) for i in range(1, 9)] == [True, False, False, False] * 2
    e, a, s, w = cfg.d_model, cfg.attn_dim(), cfg.seq_len, cfg.window
    local_keys = (w * (w + 1) / 2 + (s - w) * w) / s
    assert costs[1] == 3.0 * (2 * cfg.qkv_dim() * e + 4 * local_keys * a) + 30.0 * e
    assert costs[5] == 3.0 * (2 * cfg.qkv_dim() * e + 4 * (s / 2) * a) + 30.0 * e
    assert costs[5] > costs[1] and costs[1] == costs[9] and costs[5] == costs[13]
    assert costs[2] == 3.0 * (2 * e * a) + 30.0 * e
    assert costs[3] == 3.0 * (2 * e * 2 * cfg.dim_feedforward) + 30.0 * cfg.dim_feedforward
    # the modules agree with the planner on the FLOPs
    with torch.device("meta"):
        blocks = build_lm_blocks(cfg)
    assert 3.0 * blocks[1].core.flops_per_token(s) == costs[1] - 30.0 * e
    assert 3.0 * blocks[3].core.flops_per_token(s) == costs[5] - 30.0 * e
    assert 3.0 * blocks[1].out.flops_per_token(s) == costs[2] - 30.0 * e
    # a window that covers the sequence: local and global cores cost the same, the kinds stay apart
    wide = dataclasses.replace(cfg, window=cfg.seq_len)
    assert block_costs(wide)[1] == block_costs(wide)[5] and unit_kind(wide, 5) == "core_global"


def test_kinds_are_unchanged_without_global_every():
    for name, cfg in CONFIGS.items():
        if cfg.global_every is not None:
            assert name in GEMMA2
            continue
        n = len(block_costs(cfg))
        kinds = [unit_kind(cfg, i) for i in range(n)]
        want = ["enc"] + ["core", "out", "mlp_in", "mlp_out"] * cfg.num_layers + (
            ["norm"] if cfg.norm_first else []) + ["dec"]
        assert kinds == want, name
        assert "core_global" not in [unit_kind(cfg, i, True) for i in range(n + 1)]


def test_stage_input_shape_after_a_core():
    cfg = CONFIGS["gemma2_block_tiny"]
    n = len(block_costs(cfg))
    for cut, want in ((2, (3, 192, 256 + 512)), (6, (3, 192, 256 + 512)), (3, (3, 192, 256)),
                      (4, (3, 192, 256 + 512)), (5, (3, 192, 256))):
        plan = StagePlan([cut, n - cut], [0.0] * n, 1, False)
        assert stage_input_shape(cfg, plan, 1, 3) == want, cut
        assert stage_input_shape(cfg, plan, 0, 3) == (3, 192, 256)
    coupled = CONFIGS["gemma2_tiny"]
    n = len(block_costs(coupled))
    assert stage_input_shape(coupled, StagePlan([2, n - 2], [0.0] * n, 1, False), 1, 3) == (2, 3, 192, 256)
    # A == E through head_dim given explicitly: the stacked boundary, as without it
    same = dataclasses.replace(cfg, head_dim=64)
    assert stage_input_shape(same, StagePlan([6, n + 8 - 6], [0.0] * (n + 8), 1, False), 1, 3) == (2, 3, 192, 256)


# ------------------------------------------------------------------ 4. the replica against an eager Gemma-2 layer
def _eager_gemma2(cfg, params, tok, target):
    """Loss of a Gemma-2 decoder written with plain matmuls on fp64 ``params`` (the model's, by name)."""
    E, H, Hkv, D, S = cfg.d_model, cfg.nhead, cfg.n_kv_heads, cfg.head_dim, tok.shape[1]
    half = D // 2
    pos = torch.arange(S, dtype=torch.float64).unsqueeze(1)
    ang = pos * torch.pow(torch.tensor(cfg.rope_base, dtype=torch.float64),
                          -2.0 * torch.arange(half, dtype=torch.float64) / D)
    cos, sin = ang.cos().float().double(), ang.sin().float().double()  # the model's tables are fp32

    def rope(t):  # [B, S, heads, D], pairs (i, i + D/2)
        a, b = t[..., :half], t[..., half:]
        c, s = cos.view(1, S, 1, half), sin.view(1, S, 1, half)
        return torch.cat((a * c - b * s, b * c + a * s), -1)

    x = params["0.weight"][tok] * math.sqrt(E)
    B = x.shape[0]
    i = torch.arange(S).view(S, 1)
    j = torch.arange(S).view(1, S)
    for layer in range(cfg.num_layers):
        a_, m_ = f"{1 + 2 * layer}.", f"{2 + 2 * layer}."
        h = rms_fp64(x, params[a_ + "core.norm_weight"])
        qkv = (h @ params[a_ + "core.in_proj_weight"].T).view(B, S, H + 2 * Hkv, D)
        q, k, v = rope(qkv[:, :, :H]), rope(qkv[:, :, H:H + Hkv]), qkv[:, :, H + Hkv:]
        k, v = (t.repeat_interleave(H // Hkv, dim=2) for t in (k, v))  # query head h reads K/V head h // G
        s = torch.einsum("bihd,bjhd->bhij", q, k) * cfg.attn_scale
        s = cfg.attn_softcap * torch.tanh(s / cfg.attn_softcap)
        seen = j <= i
        if (layer + 1) % cfg.global_every != 0:  # a local layer: the last `window` keys, the query's own included
            seen = seen & (i - j < cfg.window)
        p = torch.softmax(s.masked_fill(~seen, float("-inf")), -1)
        o = torch.einsum("bhij,bjhd->bihd", p, v).reshape(B, S, H * D)
        x = x + rms_fp64(o @ params[a_ + "out.out_proj_weight"].T, params[a_ + "out.post_norm_weight"])
        h = rms_fp64(x, params[m_ + "fc_in.norm_weight"])
        gu = h @ params[m_ + "fc_in.linear1_weight"].T
        F_ = cfg.dim_feedforward
        hh = gelu_tanh_fp64(gu[..., :F_]) * gu[..., F_:]
        x = x + rms_fp64(hh @ params[m_ + "fc_out.linear2_weight"].T, params[m_ + "fc_out.post_norm_weight"])
    n = 1 + 2 * cfg.num_layers
    x = rms_fp64(x, params[f"{n}.weight"])
    logits = (x @ params[f"{n + 1}.weight"].T + params[f"{n + 1}.bias"])[..., :cfg.vocab]
    logits = cfg.final_softcap * torch.tanh(logits / cfg.final_softcap)
    logp = torch.log_softmax(logits, -1)
    return -logp.gather(-1, target.unsqueeze(-1)).mean()


@pytest.fixture(scope="module")
def replica():
    cfg = gemma2_engine.gemma2_cfg()
    assert (cfg.num_layers, cfg.d_model, cfg.nhead, cfg.n_kv_heads, cfg.head_dim, cfg.seq_len, cfg.window) == (
        2, 32, 4, 2, 16, 8, 3)
    torch.manual_seed(0)
    blocks = build_lm_blocks(cfg)
    model = torch.nn.Sequential(*blocks).train()
    with torch.no_grad():  # every norm weight off 1, the decoder's bias off 0: a dropped one shows
        for n, p in model.named_parameters():
            if n.endswith(("norm_weight", f"{1 + 2 * cfg.num_layers}.weight")):
                p.add_(0.3 * torch.randn_like(p))
            if n.endswith(".bias"):
                p[:cfg.vocab].add_(0.1 * torch.randn(cfg.vocab))
    tok = torch.randint(0, cfg.vocab, (4, cfg.seq_len + 1), generator=torch.Generator().manual_seed(7))
    return cfg, blocks, model, tok[:, :-1], tok[:, 1:].contiguous()


def test_replica_matches_the_eager_gemma2_layer(replica):
    cfg, blocks, model, x, t = replica
    model.zero_grad()
    loss = ops.cross_entropy(model(x).reshape(-1, cfg.vocab), t.reshape(-1))
    loss.backward()
    params = {n: p.detach().double().requires_grad_() for n, p in model.named_parameters()}
    assert sum(n.endswith("post_norm_weight") for n in params) == 2 * cfg.num_layers
    ref = _eager_gemma2(cfg, params, x, t)
    ref.backward()
    _close(loss.detach(), ref.detach(), torch.float32, "loss")
    for n, p in model.named_parameters():
        g = params[n].grad
        assert g.abs().max().item() > 0 or n.endswith(".bias") or n.endswith(f"{2 + 2 * cfg.num_layers}.weight"), n
        _close(p.grad, g, torch.float32, n)
    # every option is live: dropping any one of them changes the loss
    for attr, off in (("attn_scale", None), ("window", None), ("attn_softcap", None)):
        core = blocks[1].core
        keep = getattr(core, attr)
        setattr(core, attr, off)
        other = float(ops.cross_entropy(model(x).reshape(-1, cfg.vocab), t.reshape(-1)).detach())
        setattr(core, attr, keep)
        assert other != float(loss.detach()), attr


def test_replica_pipeline_units_give_the_same_output(replica):
    cfg, blocks, model, x, _ = replica
    with torch.no_grad():
        y = model(x)
        units = pipeline_units(blocks)
        assert len(units) == 1 + 4 * cfg.num_layers + 2
        h, shapes = x, []
        for u in units:  # unit by unit, as stages that hold one unit each would
            h = u(h)
            shapes.append(tuple(h.shape))
        assert torch.equal(h, y)
        E, A, F_ = cfg.d_model, cfg.attn_dim(), cfg.dim_feedforward
        assert shapes[1:5] == [(4, 8, E + A), (4, 8, E), (4, 8, E + F_), (4, 8, E)]
        n = len(units)
        for idx in range(1, n):
            plan = StagePlan([idx, n - idx], [0.0] * n, 1, False)
            assert stage_input_shape(cfg, plan, 1, 4) == shapes[idx - 1], idx
        merged = merge_units(units)
        assert len(merged) == len(blocks)
        assert torch.equal(torch.nn.Sequential(*merged)(x), y)
    # the packed boundary carries the gradient of both parts
    xs = torch.randn(2, 8, cfg.d_model).requires_grad_()
    blk = blocks[1]
    torch.nn.Sequential(*pipeline_units([blk]))(xs).sum().backward()
    g_units = xs.grad.clone()
    xs.grad = None
    blk(xs).sum().backward()
    assert torch.allclose(g_units, xs.grad, atol=1e-6)


# ------------------------------------------------------------------ 5. the engine, two gloo ranks
def test_gemma2_engine_two_gloo_ranks_cut_after_a_decoupled_core(monkeypatch):
    """helpers.engine_cases.run_engine_case as test_engine.py runs it, on the Gemma-2 replica and with the stage
    boundary between layer 1's (global, decoupled) attention core and its output: the spawned ranks start in
    helpers.gemma2_engine.worker, which swaps the helper's config and plan and runs its worker."""
    cfg = gemma2_engine.gemma2_cfg()
    plan = gemma2_engine.cut_after_core(cfg, 2)
    assert unit_kind(cfg, plan.slice(1).start - 1) == "core_global"
    assert stage_input_shape(cfg, plan, 1, 2) == (2, 8, 32 + 64)
    monkeypatch.setattr(engine_cases, "case_cfg", gemma2_engine.gemma2_cfg)
    monkeypatch.setattr(engine_cases, "worker", gemma2_engine.worker)
    engine_cases.run_engine_case("cpu", 2, "except_last", 1, False, False)
