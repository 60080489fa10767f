"""The sigmoid router on the CPU: the reference against a transcription of Hugging Face's DeepSeek-V3 gate, the
argument checks of the op, the block and ``LMConfig``, the defaults, the fp32 ``router_bias``, the bias update and
the shared experts' accounting."""
import dataclasses

import pytest
import torch

from mipipe import checkpoint, ops
from mipipe.models import CONFIGS
from mipipe.models.lm import LMConfig
from mipipe.models.transformer import MoEFeedForwardBlock
from mipipe.parallel.stage import block_costs, moe_cost


def _hf_gate(logits, bias, k, n_group, topk_group, norm_topk_prob, scale):
    """DeepSeekV3TopkRouter of transformers, line by line (its ``get_topk_indices`` and ``forward``)."""
    T = logits.shape[0]
    scores = logits.sigmoid()
    scores_for_choice = scores + bias[None]
    group_scores = scores_for_choice.view(T, n_group, -1).topk(2, dim=-1)[0].sum(dim=-1)
    group_idx = torch.topk(group_scores, k=topk_group, dim=-1, sorted=False)[1]
    group_mask = torch.zeros_like(group_scores).scatter_(1, group_idx, 1)
    score_mask = group_mask.unsqueeze(-1).expand(-1, n_group, logits.shape[1] // n_group).reshape(T, -1)
    scores_for_choice = scores_for_choice.masked_fill(~score_mask.bool(), 0.0)
    topk_indices = torch.topk(scores_for_choice, k=k, dim=-1, sorted=False)[1]
    topk_weights = scores.gather(1, topk_indices)
    if norm_topk_prob:
        topk_weights = topk_weights / (topk_weights.sum(dim=-1, keepdim=True) + 1e-20)
    return topk_indices, topk_weights * scale


@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("Ne,k,n_group,topk_group", [(256, 8, 8, 4), (16, 2, 4, 2), (6, 2, 1, 1)])
def test_reference_is_the_hugging_face_gate(Ne, k, n_group, topk_group, norm):
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(97, Ne, generator=g, dtype=torch.float64)
    bias = torch.rand(Ne, generator=g, dtype=torch.float64) * 0.4    # c > 0: the 0.0 fill never wins
    idx, gate, probs = ops.moe_route(logits, k, score="sigmoid", bias=bias, n_group=n_group, topk_group=topk_group,
                                     renormalize=norm, scale=2.5)
    h_idx, h_w = _hf_gate(logits, bias, k, n_group, topk_group, norm, 2.5)
    assert torch.equal(idx.long().sort(-1).values, h_idx.sort(-1).values)
    assert torch.allclose(gate.sort(-1).values, h_w.sort(-1).values, rtol=1e-12, atol=0)
    s = logits.sigmoid()
    assert torch.allclose(probs, (s / s.sum(-1, keepdim=True)).sum(0), rtol=1e-12) and idx.dtype == torch.int32
    c = (s + bias).gather(1, idx.long())
    assert (c[:, :-1] >= c[:, 1:]).all()                             # idx is in descending c


def test_value_errors():
    lg = torch.zeros(4, 8)
    softmax_only = [dict(n_group=2), dict(scale=2.0), dict(renormalize=False), dict(topk_group=2),
                    dict(bias=torch.zeros(8))]
    sigmoid = [("n_group", dict(n_group=3)), ("n_group", dict(n_group=0)), ("n_group", dict(n_group=8)),
               ("topk_group", dict(n_group=4, topk_group=5)), ("topk_group", dict(n_group=4, topk_group=0)),
               ("topk_group", dict(topk_group=2)), ("bias", dict(bias=torch.zeros(7))),
               ("bias", dict(bias=torch.zeros(8, dtype=torch.int32))), ("scale", dict(scale=float("inf")))]
    for name, kw in [("score", dict(score="tanh"))] + [("sigmoid", kw) for kw in softmax_only] + \
            [(n, dict(score="sigmoid", **kw)) for n, kw in sigmoid]:
        with pytest.raises(ValueError, match=name):
            ops.moe_route(lg, 2, **kw)
    with pytest.raises(ValueError, match="topk_group"):   # 1 group of 2 experts holds fewer than k = 3
        ops.moe_route(lg, 3, score="sigmoid", n_group=4, topk_group=1)
    for kw in (dict(router="tanh"), dict(n_group=2), dict(routed_scale=2.0), dict(norm_topk_prob=False),
               dict(bias_update_rate=1e-3), dict(router="sigmoid", n_group=3),
               dict(router="sigmoid", n_group=4, topk_group=5), dict(router="sigmoid", n_shared_experts=-1),
               dict(router="sigmoid", bias_update_rate=-1.0), dict(router="sigmoid", n_group=8),
               dict(router="sigmoid", routed_scale=float("nan"))):
        with pytest.raises(ValueError):
            MoEFeedForwardBlock(16, 32, 8, 2, **kw)
        cfg_kw = {{"router": "moe_router", "bias_update_rate": "moe_bias_rate", "n_shared_experts": "n_shared_experts"}
                  .get(a, "moe_" + a): v for a, v in kw.items()}
        with pytest.raises(ValueError):
            dataclasses.replace(CONFIGS["moe_tiny"], n_experts=8, **cfg_kw)


def test_defaults_are_todays():
    lg = torch.randn(33, 8, generator=torch.Generator().manual_seed(1))
    for a, b in zip(ops.moe_route(lg, 2), ops.moe_route_reference(lg, 2)):
        assert torch.equal(a, b)
    assert torch.equal(ops.moe_route(lg, 2)[1], torch.softmax(lg.sort(-1, descending=True).values[:, :2], -1))
    sd = MoEFeedForwardBlock(16, 32, 4, 2).state_dict()
    assert not {"router_bias", "expert_load", "shared_w1", "shared_w2"} & set(sd)
    names = [f.name for f in dataclasses.fields(LMConfig)]
    i = names.index("expert_gemm")
    assert names[i - 1] == "moe_aux_coef" and names[-1] == "qk_norm"
    assert names[i + 1:-1] == ["moe_router", "moe_n_group", "moe_topk_group", "moe_routed_scale", "moe_norm_topk_prob",
                               "n_shared_experts", "moe_bias_rate"]


def _block(**kw):
    torch.manual_seed(0)
    return MoEFeedForwardBlock(16, 32, 8, 2, capacity_factor=None, router="sigmoid", n_group=4, topk_group=2,
                               routed_scale=2.5, **kw)


def test_router_bias_stays_fp32_and_round_trips():
    blk = _block(n_shared_experts=1, bias_update_rate=1e-3)
    blk.router_bias.copy_(torch.arange(8) * 1e-3 + 1.0)             # 1.001 is not a bf16 value
    want = blk.router_bias.clone()
    blk.to(torch.bfloat16)
    assert blk.router_bias.dtype == torch.float32 and torch.equal(blk.router_bias, want)
    assert blk.shared_w1.dtype == torch.bfloat16 and blk.expert_load.dtype == torch.int32
    assert blk.double().router_bias.dtype == torch.float32
    other = _block(n_shared_experts=1).to(torch.bfloat16)
    other.load_state_dict(blk.state_dict())
    assert torch.equal(other.router_bias, want) and other.router_bias.dtype == torch.float32


def test_update_router_bias_and_the_skip_under_recompute():
    blk = _block(bias_update_rate=1e-3)
    x = torch.randn(2, 24, 16, generator=torch.Generator().manual_seed(2)).requires_grad_()
    with torch.no_grad():
        blk(x)
    assert int(blk.expert_load.sum()) == 0                          # no graph, no count
    checkpoint(blk, x).sum().backward()                             # forward + recompute: counted once
    assert int(blk.expert_load.sum()) == 48 * 2
    blk(x)
    load = blk.expert_load.clone()
    assert int(load.sum()) == 2 * 48 * 2
    blk.update_router_bias()
    assert torch.equal(blk.router_bias, 1e-3 * torch.sign(load.sum() - 8 * load.long()).float())
    assert (blk.expert_load == 0).all()
    still = _block()                                                # rate 0: a no-op, the load stays
    still(x)
    still.update_router_bias()
    assert int(still.expert_load.sum()) == 96 and (still.router_bias == 0).all()
    bias, load = torch.zeros(6), torch.tensor([10, 2, 6, 6, 0, 12], dtype=torch.int32)   # mean 6
    ops.moe_bias_update(bias, load, 0.5)
    assert bias.tolist() == [-0.5, 0.5, 0.0, 0.0, 0.5, -0.5] and load.tolist() == [0] * 6


def test_shared_experts_are_counted():
    base = dataclasses.replace(CONFIGS["moe_tiny"], moe_router="sigmoid", moe_n_group=2)
    one = dataclasses.replace(base, n_shared_experts=1)
    e, f, L = base.d_model, base.dim_feedforward, base.num_layers
    assert base.params() == CONFIGS["moe_tiny"].params() and moe_cost(base) == moe_cost(CONFIGS["moe_tiny"])
    assert one.params() - base.params() == L * 3 * e * f
    shared = 3.0 * (2 * e * 2 * f) + 3.0 * 10 * f + 3.0 * (2 * e * f)
    assert moe_cost(one) - moe_cost(base) == shared
    assert sum(block_costs(one)) - sum(block_costs(base)) == L * shared
    blk = MoEFeedForwardBlock(e, f, 4, 2, n_shared_experts=1)
    assert blk.flops_per_token(192) - MoEFeedForwardBlock(e, f, 4, 2).flops_per_token(192) == 6 * e * f
    assert sum(p.numel() for p in blk.parameters()) == e + 4 * e + 5 * 3 * e * f
