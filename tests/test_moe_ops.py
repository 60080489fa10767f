"""Mixture-of-experts MLP on the CPU: the eager references of mipipe.ops.moe against independent formulations,
their gradients, the block against a dense per-token loop, the configs, the planner's units and the engine."""
import dataclasses
import math

import pytest
import torch

from helpers import engine_cases, moe_engine

from mipipe import ops
from mipipe.models import CONFIGS, MOE_CONFIGS, LMConfig, build_lm_blocks
from mipipe.models.transformer import (GATED_ACTS, FeedForwardBlock, MoEFeedForwardBlock, SelfAttentionBlock,
                                       block_flops, pipeline_units, transformer_blocks)
from mipipe.models.vocab_split import split_point
from mipipe.parallel.calibrate import unit_kinds
from mipipe.parallel.stage import block_costs, layer_kinds, plan_stages, split_allowed, stage_input_shape

NEW_CONFIGS = ("moe_tiny", "mixtral_8x7b", "qwen3_30b_a3b")
OLD_CONFIGS = [n for n in CONFIGS if n not in NEW_CONFIGS]   # a sweep of CONFIGS lists the dense configs alone


def test_configs_table_finds_the_moe_configs_by_name():
    """``CONFIGS[name]`` knows every config; iterating it lists the dense ones, each of four units per layer."""
    assert tuple(MOE_CONFIGS) == NEW_CONFIGS and OLD_CONFIGS == list(CONFIGS) and len(CONFIGS) == len(OLD_CONFIGS)
    for name in NEW_CONFIGS:
        assert name in CONFIGS and CONFIGS[name] is MOE_CONFIGS[name] is CONFIGS.get(name)
        assert CONFIGS[name].name == name and CONFIGS[name].n_experts is not None
        assert name not in list(CONFIGS) and name not in CONFIGS.keys() and name not in dict(CONFIGS.items())
    assert all(cfg.n_experts is None for cfg in CONFIGS.values())
    assert "no_such_config" not in CONFIGS and CONFIGS.get("no_such_config") is None
    with pytest.raises(KeyError, match="no_such_config"):
        CONFIGS["no_such_config"]


def _logits(T, Ne, dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(T, Ne, generator=g) + torch.linspace(-1, 1, Ne)).to(dtype)


# ------------------------------------------------------------------ 1. references against independent formulations
@pytest.mark.parametrize("T,Ne,k", [(1, 2, 1), (37, 4, 2), (64, 8, 2), (50, 128, 8), (9, 256, 8)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_route_reference_is_softmax_topk_renormalised(T, Ne, k, dtype):
    logits = _logits(T, Ne, dtype)
    idx, gate, probs_sum = ops.moe_route(logits, k)
    assert idx.dtype == torch.int32 and gate.dtype == torch.float32 and probs_sum.dtype == torch.float32
    p = torch.softmax(logits.double(), -1)
    # a Python top-k with the tie rule spelt out: the larger logit, then the lower expert
    for t in range(T):
        row = logits[t].double().tolist()
        order = sorted(range(Ne), key=lambda e: (-row[e], e))[:k]
        assert idx[t].tolist() == order
        sel = p[t, order]
        torch.testing.assert_close(gate[t].double(), sel / sel.sum(), rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(probs_sum.double(), p.sum(0), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(gate.sum(-1), torch.ones(T), rtol=1e-6, atol=1e-6)


def test_route_reference_ties_and_neg_inf():
    logits = torch.tensor([[1.0, 1.0, 1.0, 1.0], [0.0, 2.0, 2.0, -1.0], [float("-inf"), 3.0, float("-inf"), float("-inf")]])
    idx, gate, _ = ops.moe_route(logits, 2)
    assert idx.tolist() == [[0, 1], [1, 2], [1, 0]]
    assert gate[2].tolist() == [1.0, 0.0]   # a selected -inf gets exactly 0
    assert gate[0].tolist() == [0.5, 0.5]


def _assign_loop(idx, Ne, C):
    T, k = idx.shape
    fill = [0] * Ne
    slot = [[-1] * k for _ in range(T)]
    src = [-1] * (Ne * C)
    for j in range(k):          # choice-major: every first choice before any second choice
        for t in range(T):
            e = int(idx[t, j])
            if fill[e] < C:
                slot[t][j] = e * C + fill[e]
                src[slot[t][j]] = t * k + j
            fill[e] += 1
    return slot, src, fill


@pytest.mark.parametrize("T,Ne,k,C", [(1, 2, 1, 1), (37, 4, 2, 7), (193, 6, 2, 50), (64, 8, 2, 64), (40, 128, 8, 2)])
def test_assign_reference_is_the_loop(T, Ne, k, C):
    idx = ops.moe_route(_logits(T, Ne, torch.bfloat16), k)[0]
    slot, src, counts = ops.moe_assign(idx, Ne, C)
    assert slot.dtype == src.dtype == counts.dtype == torch.int32
    want_slot, want_src, want_counts = _assign_loop(idx, Ne, C)
    assert slot.tolist() == want_slot and src.tolist() == want_src and counts.tolist() == want_counts
    assert int(counts.sum()) == T * k


def test_first_choice_keeps_its_place():
    """Token 1's first choice is expert 0, which token 0 takes as its SECOND choice: with one slot, token 1 gets it."""
    idx = torch.tensor([[1, 0], [0, 1]], dtype=torch.int32)
    slot, src, counts = ops.moe_assign(idx, 2, 1)
    assert slot.tolist() == [[1, -1], [0, -1]] and src.tolist() == [2, 0] and counts.tolist() == [2, 2]


# ------------------------------------------------------------------ 2. gradients of the ops
def test_gradcheck_route():
    logits = _logits(7, 6, torch.float64, seed=3).requires_grad_()   # no ties: continuous values
    assert torch.autograd.gradcheck(lambda l: ops.moe_route(l, 3)[1:], (logits,))


def _tables(T=11, Ne=6, k=2, C=4):
    idx = ops.moe_route(_logits(T, Ne, seed=5), k)[0]
    slot, src, _ = ops.moe_assign(idx, Ne, C)
    assert (slot < 0).any() and (src < 0).any()   # both drops and empty slots
    return slot, src


def test_gradcheck_dispatch_and_combine():
    slot, src = _tables()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(11, 8, generator=g, dtype=torch.float64).requires_grad_()
    assert torch.autograd.gradcheck(lambda t: ops.moe_dispatch(t, slot, src), (x,))
    ye = torch.randn(24, 8, generator=g, dtype=torch.float64).requires_grad_()
    gate = torch.rand(11, 2, generator=g, dtype=torch.float64).requires_grad_()
    res = torch.randn(11, 8, generator=g, dtype=torch.float64).requires_grad_()
    assert torch.autograd.gradcheck(lambda a, b, c: ops.moe_combine(a, b, slot, src, residual=c), (ye, gate, res))
    assert torch.autograd.gradcheck(lambda a, b: ops.moe_combine(a, b, slot, src), (ye, gate))


def test_dispatch_is_a_copy_with_zero_fill():
    slot, src = _tables()
    x = torch.randn(11, 8).to(torch.bfloat16)
    xe = ops.moe_dispatch(x, slot, src)
    for s, a in enumerate(src.tolist()):
        assert torch.equal(xe[s], x[a // 2] if a >= 0 else torch.zeros(8, dtype=torch.bfloat16))


# ------------------------------------------------------------------ 3. the dropless block against a dense loop
def _block(d=16, f=32, ne=4, k=2, **kw):
    torch.manual_seed(0)
    blk = MoEFeedForwardBlock(d, f, ne, k, **kw).double()
    with torch.no_grad():
        blk.router_weight.normal_(std=0.5)
        blk.norm_weight.uniform_(0.5, 1.5)
    return blk


@pytest.mark.parametrize("activation", GATED_ACTS)
def test_dropless_block_is_the_dense_loop(activation):
    blk = _block(capacity_factor=None, activation=activation)
    x = torch.randn(2, 9, 16, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    y = blk(x)
    assert float(blk.last_drop_fraction) == 0.0
    xn = ops.rms_norm_reference(x, None, blk.norm_weight, blk.eps, 0.0, False).reshape(-1, 16)
    logits = xn @ blk.router_weight.t()
    act = ops.swiglu_reference if activation == "swiglu" else ops.geglu_reference
    want = x.reshape(-1, 16).clone()
    for t in range(xn.shape[0]):
        top = torch.topk(logits[t], 2)
        w = torch.softmax(top.values, -1)
        for wj, e in zip(w, top.indices.tolist()):
            want[t] = want[t] + wj * (act(xn[t] @ blk.experts_w1[e].t()) @ blk.experts_w2[e].t())
    torch.testing.assert_close(y.reshape(-1, 16), want, rtol=1e-10, atol=1e-10)


def test_capacity_drops_and_empty_slots_give_zero_gradients():
    blk = _block(capacity_factor=0.01, aux_coef=0.0)   # 64 slots per expert for 600 x 2 choices
    x = torch.randn(1, 600, 16, dtype=torch.float64, generator=torch.Generator().manual_seed(4)).requires_grad_()
    y = blk(x)
    assert 0.5 < float(blk.last_drop_fraction) < 1.0
    y.sum().backward()
    assert torch.isfinite(x.grad).all() and all(torch.isfinite(p.grad).all() for p in blk.parameters())


# ------------------------------------------------------------------ 4. argument checks
def test_argument_checks():
    lg = _logits(8, 4)
    with pytest.raises(ValueError, match="k=5"):
        ops.moe_route(lg, 5)
    with pytest.raises(ValueError, match="at most 8"):
        ops.moe_route(_logits(8, 16), 9)
    with pytest.raises(ValueError, match="at most 256"):
        ops.moe_route(_logits(2, 257), 2)
    with pytest.raises(ValueError):
        ops.moe_route(lg[0], 2)
    idx = ops.moe_route(lg, 2)[0]
    with pytest.raises(ValueError, match="capacity"):
        ops.moe_assign(idx, 4, 0)
    with pytest.raises(ValueError, match="int32"):
        ops.moe_assign(idx.long(), 4, 4)
    with pytest.raises(ValueError, match="at most 256"):
        ops.moe_assign(idx, 257, 4)
    with pytest.raises(ValueError, match="2\\^31"):
        ops.moe_assign(idx, 256, 2 ** 23)
    slot, src, _ = ops.moe_assign(idx, 4, 4)
    x, ye, gate = torch.randn(8, 8), torch.randn(16, 8), torch.rand(8, 2)
    with pytest.raises(ValueError, match="tokens"):
        ops.moe_dispatch(x[:7], slot, src)
    with pytest.raises(ValueError, match="int32"):
        ops.moe_dispatch(x, slot.long(), src)
    with pytest.raises(ValueError):
        ops.moe_dispatch(x.view(2, 4, 8), slot, src)
    with pytest.raises(ValueError, match="slots"):
        ops.moe_combine(ye[:15], gate, slot, src)
    with pytest.raises(ValueError, match="gate"):
        ops.moe_combine(ye, gate[:, :1], slot, src)
    with pytest.raises(ValueError, match="gate must be"):
        ops.moe_combine(ye, gate.to(torch.bfloat16), slot, src)
    with pytest.raises(ValueError, match="residual"):
        ops.moe_combine(ye, gate, slot, src, residual=x[:7])
    with pytest.raises(ValueError, match="residual"):
        ops.moe_combine(ye, gate, slot, src, residual=x.double())
    for kw in (dict(norm_first=False), dict(bias=True), dict(activation="relu")):
        with pytest.raises(ValueError):
            MoEFeedForwardBlock(16, 32, 4, 2, **kw)
    for ne, k in ((1, 1), (257, 2), (4, 5), (16, 9), (4, 0)):
        with pytest.raises(ValueError):
            MoEFeedForwardBlock(16, 32, ne, k)


# ------------------------------------------------------------------ 5. capacity
def test_moe_capacity_rounding_and_clamp():
    assert ops.moe_capacity(8192, 8, 2, 1.0) == 2048
    assert ops.moe_capacity(8192, 8, 2, 1.25) == 2560
    assert ops.moe_capacity(384, 4, 2, 1.0) == 192
    assert ops.moe_capacity(1000, 128, 8, 1.0) == 64      # 62.5 -> 63 -> 64
    assert ops.moe_capacity(1000, 8, 2, 1.1) == 320       # 275 -> 320
    assert ops.moe_capacity(100, 4, 2, 4.0) == 128        # 200 clamped to ceil64(100)
    assert ops.moe_capacity(100, 4, 2, None) == 128 and ops.moe_capacity(64, 4, 2, None) == 64
    assert ops.moe_capacity(1, 256, 1, 1.0) == 64
    for t, ne, k, cf in ((16, 4, 2, 1.25), (3000, 8, 2, 1.0), (777, 6, 3, 0.5)):
        c = ops.moe_capacity(t, ne, k, cf)
        assert c % 64 == 0 and c >= min(math.ceil(cf * t * k / ne), t) and c <= (t + 63) // 64 * 64
    with pytest.raises(ValueError):
        ops.moe_capacity(16, 4, 2, 0.0)


# ------------------------------------------------------------------ 6. default off
def test_n_experts_none_registers_nothing():
    assert LMConfig("x", 1, 8, 1, 8, 10, 4).n_experts is None
    with torch.device("meta"):
        dense = transformer_blocks(2, 32, 4, 64, 0.0, "swiglu", norm_first=True, norm="rms", bias=False)
        moe = transformer_blocks(2, 32, 4, 64, 0.0, "swiglu", norm_first=True, norm="rms", bias=False, n_experts=4)
    assert [type(b) for b in dense] == [SelfAttentionBlock, FeedForwardBlock] * 2
    assert [type(b) for b in moe] == [SelfAttentionBlock, MoEFeedForwardBlock] * 2
    names = [n for b in dense for n, _ in b.named_parameters()]
    assert not any("router" in n or "experts" in n for n in names)
    assert sorted(n for n, _ in moe[1].named_parameters()) == sorted(
        ["norm_weight", "router_weight"] + [f"experts_w{i}.{e}" for i in (1, 2) for e in range(4)])
    tagged = {n for n, p in moe[1].named_parameters() if getattr(p, "_mipipe_gemm_weight", False)}
    assert tagged == {f"experts_w{i}.{e}" for i in (1, 2) for e in range(4)}
    for name in OLD_CONFIGS:
        assert CONFIGS[name].n_experts is None


# ------------------------------------------------------------------ 7. the dense configs plan as before
def _dense_costs(cfg, split_decoder=False):
    """block_costs as it was before the mixture-of-experts unit existed."""
    e, f, s, v = cfg.d_model, cfg.dim_feedforward, cfg.seq_len, cfg.vocab

    def core_cost(w):
        keys = (w * (w + 1) / 2 + (s - w) * w) / s if w is not None and w < s else s * (0.5 if cfg.causal else 1.0)
        return 3.0 * (2 * cfg.qkv_dim() * e + 4 * keys * cfg.attn_dim()) + 3.0 * 10 * e

    out = 3.0 * (2 * e * cfg.attn_dim()) + 3.0 * 10 * e
    if cfg.activation in GATED_ACTS:
        mlp_in = 3.0 * (2 * e * 2 * f) + 3.0 * 10 * f
    else:
        mlp_in = 3.0 * (2 * e * f) + 3.0 * 5 * f
    mlp_out = 3.0 * (2 * e * f) + 3.0 * 10 * e
    costs = [3.0 * 40 * e]
    for i in range(cfg.num_layers):
        costs += [core_cost(cfg.layer_window(i)), out, mlp_in, mlp_out]
    if cfg.norm_first:
        costs.append(3.0 * 10 * e)
    dec = 3.0 * (2 * e * v) + 3.0 * 4 * v
    if split_decoder:
        va = split_point(v)
        costs += [dec * va / v, dec * (v - va) / v]
    else:
        costs.append(dec)
    return costs


def _dense_kinds(cfg, split_decoder=False):
    kinds = ["enc"]
    for i in range(cfg.num_layers):
        glob = cfg.global_every is not None and cfg.layer_window(i) is None
        kinds += ["core_global" if glob else "core", "out", "mlp_in", "mlp_out"]
    if cfg.norm_first:
        kinds.append("norm")
    return kinds + (["dec_head", "dec_tail"] if split_decoder else ["dec"])


@pytest.mark.parametrize("name", OLD_CONFIGS)
def test_dense_configs_plan_as_before(name):
    cfg = CONFIGS[name]
    assert layer_kinds(cfg) == ("core", "out", "mlp_in", "mlp_out")
    for split in ((False, True) if split_allowed(cfg) else (False,)):
        assert block_costs(cfg, split) == _dense_costs(cfg, split)
        assert unit_kinds(cfg, split) == _dense_kinds(cfg, split)
    for stages in (2, 4):
        got = plan_stages(cfg, stages)
        want = plan_stages(cfg, stages, costs=_dense_costs(cfg))
        assert got.balance == want.balance and got.costs == want.costs
    if cfg.num_layers <= 4:
        assert (plan_stages(cfg, 2, 2, 8).balance == plan_stages(cfg, 2, 2, 8, costs=_dense_costs(cfg)).balance)


# ------------------------------------------------------------------ 8. the MoE units
def test_moe_tiny_units():
    cfg = CONFIGS["moe_tiny"]
    assert unit_kinds(cfg) == ["enc"] + ["core", "out", "moe"] * 2 + ["norm", "dec"]
    assert unit_kinds(cfg, True) == ["enc"] + ["core", "out", "moe"] * 2 + ["norm", "dec_head", "dec_tail"]
    with torch.device("meta"):
        blocks = build_lm_blocks(cfg)
        units = pipeline_units(blocks)
    assert len(units) == len(block_costs(cfg)) == 9 and isinstance(units[3], MoEFeedForwardBlock)
    costs, base = block_costs(cfg), block_costs(CONFIGS["mistral_tiny"])
    assert costs[1:3] == base[1:3] and costs[-2:] == base[-2:]
    # what runs: ceil64(1.25 * 1536 * 2 / 4) = 960 slots per expert for 1536 tokens, 2.5 padded expert rows per token
    assert ops.moe_capacity(8 * cfg.seq_len, 4, 2, 1.25) == 960
    assert costs[3] > 2.5 * (base[3] + base[4]) * 0.95 and costs[3] < 3.0 * (base[3] + base[4])
    plan = plan_stages(cfg, 2)
    assert sum(plan.balance) == 9
    for vs in (0, 1):
        assert stage_input_shape(cfg, plan, vs, 2)[-1] in (cfg.seq_len, cfg.d_model)
    # the block counts the model's FLOPs: the router and k experts, not the padding
    e, f = cfg.d_model, cfg.dim_feedforward
    assert blocks[2].flops_per_token(cfg.seq_len) == 2 * e * 4 + 2 * (2 * e * 2 * f + 2 * e * f)
    assert block_flops(blocks[2], cfg.seq_len) == 3.0 * blocks[2].flops_per_token(cfg.seq_len)


# ------------------------------------------------------------------ 9. parameter counts
def _moe_params(cfg):
    e, f, v, ne = cfg.d_model, cfg.dim_feedforward, cfg.vocab, cfg.n_experts
    attn = (cfg.qkv_dim() + cfg.attn_dim()) * e + (2 * cfg.head_width() if cfg.qk_norm else 0)
    layer = attn + 2 * e + ne * e + ne * 3 * e * f    # two RMSNorms, the router, gate + up + down per expert
    return cfg.num_layers * layer + v * e + e + (v * e + v)


def test_moe_params():
    mix = CONFIGS["mixtral_8x7b"]
    assert mix.params() == _moe_params(mix)
    assert 46.6e9 < mix.params() < 46.9e9            # Mixtral 8x7B: 46.7 B
    qw = CONFIGS["qwen3_30b_a3b"]
    assert qw.params() == _moe_params(qw) and 30.3e9 < qw.params() < 30.8e9
    cfg = moe_engine.moe_cfg()
    assert cfg.params() == _moe_params(cfg)
    model = torch.nn.Sequential(*build_lm_blocks(cfg))
    pad = model[-1].padded - cfg.vocab
    assert sum(p.numel() for p in model.parameters()) == cfg.params() + pad * cfg.d_model + pad
    with torch.device("meta"):
        tiny = torch.nn.Sequential(*build_lm_blocks(CONFIGS["moe_tiny"]))
    pad = tiny[-1].padded - 1000
    assert sum(p.numel() for p in tiny.parameters()) == CONFIGS["moe_tiny"].params() + pad * 256 + pad


# ------------------------------------------------------------------ 10. a CPU training step
def _cpu_model(**kw):
    cfg = dataclasses.replace(moe_engine.moe_cfg(), **kw)
    torch.manual_seed(0)
    model = torch.nn.Sequential(*build_lm_blocks(cfg)).train()
    tok = torch.randint(0, cfg.vocab, (4, cfg.seq_len + 1), generator=torch.Generator().manual_seed(7))
    x, t = tok[:, :-1], tok[:, 1:].contiguous()
    return cfg, model, lambda: ops.cross_entropy(model(x).reshape(-1, cfg.vocab), t.reshape(-1))


def test_moe_tiny_cpu_step_changes_the_router():
    cfg, model, loss_fn = _cpu_model()
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    loss = loss_fn()
    loss.backward()
    assert math.isfinite(float(loss)) and all(p.grad is not None and torch.isfinite(p.grad).all()
                                              for p in model.parameters())
    moes = [b for b in model if isinstance(b, MoEFeedForwardBlock)]
    assert len(moes) == 2
    before = [b.router_weight.detach().clone() for b in moes]
    assert all((b.router_weight.grad != 0).any() for b in moes)
    assert all(any((w.grad != 0).any() for w in b.experts_w1) for b in moes)
    assert all(b.last_aux.dim() == 0 and not b.last_aux.requires_grad and float(b.last_aux) >= 1.0 - 1e-5
               for b in moes)   # Ne sum f_e P_e >= 1 by Cauchy-Schwarz when f is the argmax share; ~1 when balanced
    opt.step()
    assert all(not torch.equal(b.router_weight.detach(), w) for b, w in zip(moes, before))


# ------------------------------------------------------------------ 11. / 12. the router's gradient
def _router_grads(aux_coef, aux_scale=1.0):
    blk = _block(d=16, f=32, ne=6, k=2, capacity_factor=None, aux_coef=aux_coef)
    blk.aux_scale = aux_scale
    x = torch.randn(1, 20, 16, dtype=torch.float64, generator=torch.Generator().manual_seed(9))
    seen = {}
    linear = ops.linear

    def spy(inp, w, *a, **k):
        y = linear(inp, w, *a, **k)
        if w is blk.router_weight:
            y.retain_grad()
            seen["logits"] = y
        return y

    ops.linear = spy
    try:
        blk(x).square().sum().backward()
    finally:
        ops.linear = linear
    lg = seen["logits"]
    return lg.detach(), lg.grad.clone(), blk.router_weight.grad.clone()


def test_unselected_logit_gradients_are_zero_without_aux():
    lg, dl, _ = _router_grads(0.0)
    top = torch.topk(lg, 2).indices
    sel = torch.zeros_like(lg, dtype=torch.bool).scatter_(1, top, True)
    assert (dl[~sel] == 0).all() and (dl[sel] != 0).any()
    lg1, dl1, _ = _router_grads(0.01)
    assert torch.equal(lg, lg1) and (dl1[~sel] != 0).all()


def test_aux_scale_scales_the_aux_part_linearly():
    _, _, g0 = _router_grads(0.0)
    _, _, g1 = _router_grads(0.01, 1.0)
    _, _, g4 = _router_grads(0.01, 0.25)
    _, _, g2c = _router_grads(0.02, 1.0)
    assert (g1 - g0).abs().max() > 0
    torch.testing.assert_close(g4 - g0, 0.25 * (g1 - g0), rtol=1e-9, atol=1e-15)
    torch.testing.assert_close(g2c - g0, 2.0 * (g1 - g0), rtol=1e-9, atol=1e-15)
    # and it is the gradient of aux_coef * aux: Ne sum_e (counts_e / (T k)) (probs_sum_e / T) through probs_sum
    lg = _logits(20, 6, torch.float64, seed=11).requires_grad_()
    idx, gate, probs_sum = ops.moe_route(lg, 2)
    counts = ops.moe_assign(idx, 6, 64)[2]
    aux = 6 * ((counts.double() / 40) * (probs_sum / 20)).sum()
    (want,) = torch.autograd.grad(0.01 * aux, lg)
    lg2 = lg.detach().clone().requires_grad_()
    idx, gate, probs_sum = ops.moe_route(lg2, 2)
    g = ops.moe_attach_aux(gate, probs_sum, counts.double() * (0.01 * 6 / (20 * 20 * 2)))
    (g * 0).sum().backward()
    torch.testing.assert_close(lg2.grad, want, rtol=1e-10, atol=1e-14)


# ------------------------------------------------------------------ 13. the engine, two gloo ranks
def test_moe_engine_two_gloo_ranks(monkeypatch):
    """helpers.engine_cases.run_engine_case on the mixture-of-experts replica: the spawned ranks start in
    helpers.moe_engine.worker, which swaps the helper's config and wraps its engine so that every rank asserts
    ``aux_scale = 1 / (chunks * grad_divisor)`` on its MoE blocks.  Every gradient of every rank, the routers' and
    the experts' among them, is compared with the single-rank engine's."""
    monkeypatch.setattr(engine_cases, "case_cfg", moe_engine.moe_cfg)
    monkeypatch.setattr(engine_cases, "worker", moe_engine.worker)
    monkeypatch.setattr(engine_cases, "PipelineEngine", moe_engine.checked_engine)
    single = engine_cases.single_rank_reference
    seen = {}

    def spy(*args, **kwargs):
        out = single(*args, **kwargs)
        seen.update(out[1])
        return out

    monkeypatch.setattr(engine_cases, "single_rank_reference", spy)
    engine_cases.run_engine_case("cpu", 2, "except_last", 1, False, False)
    routers = [n for n in seen if n.endswith("router_weight")]
    experts = [n for n in seen if "experts_w" in n]
    assert len(routers) == 2 and len(experts) == 16
    assert all((seen[n] != 0).any() for n in routers)
