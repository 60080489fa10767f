"""The dropless mixture-of-experts path on the CPU: the row bound of the sorted layout against a brute force, the
sorted assignment and the grouped linear against plain Python loops, the grouped block against the ``"loop"`` block,
the option's errors, the planner's price and the engine on two gloo ranks."""
import dataclasses
import itertools

import pytest
import torch

from helpers import engine_cases, moe_grouped_engine

from mipipe import ops
from mipipe.models import CONFIGS, LMConfig, build_lm_blocks
from mipipe.models.transformer import MoEFeedForwardBlock, transformer_blocks
from mipipe.parallel.stage import block_costs, moe_cost, plan_stages


# ------------------------------------------------------------------ 1. the row bound
def _sorted_rows(total, ne, align):
    n = min(ne, total)
    return align * (n + (total - n) // align)


def _brute(total, ne, align):
    return align * max(sum(-(-c // align) for c in counts)
                       for counts in itertools.product(range(total + 1), repeat=ne) if sum(counts) == total)


@pytest.mark.parametrize("align", [2, 4])
@pytest.mark.parametrize("ne", [1, 2, 3, 4])
def test_row_bound_is_the_brute_force_maximum(align, ne):
    for total in range(1, 14):
        assert _sorted_rows(total, ne, align) == _brute(total, ne, align), total


def test_moe_sorted_rows_bounds_random_counts():
    assert ops.moe_sorted_rows(8192, 8, 2) == 128 * (8 + (16384 - 8) // 128) == 17280
    assert ops.moe_sorted_rows(1, 256, 1) == 128 and ops.moe_sorted_rows(3, 2, 2) == 256
    g = torch.Generator().manual_seed(0)
    for T, ne, k in ((37, 4, 2), (1000, 128, 8), (9, 256, 8), (4100, 8, 2), (129, 2, 1)):
        assert ops.moe_sorted_rows(T, ne, k) == _sorted_rows(T * k, ne, 128)
        for _ in range(50):
            conc = torch.rand(ne, generator=g) ** 4 + 1e-6
            counts = torch.bincount(torch.multinomial(conc, T * k, replacement=True, generator=g), minlength=ne)
            assert int(((counts + 127) // 128 * 128).sum()) <= ops.moe_sorted_rows(T, ne, k)
    with pytest.raises(ValueError):
        ops.moe_sorted_rows(0, 4, 2)


# ------------------------------------------------------------------ 2. the assignment against a plain loop
def _loop_assign(idx, ne):
    T, k = idx.shape
    rows = ops.moe_sorted_rows(T, ne, k)
    counts = [0] * ne
    pos = {}
    for j in range(k):             # choice-major: every token's first choice, then every second
        for t in range(T):
            e = int(idx[t, j])
            if 0 <= e < ne:
                pos[(t, j)] = counts[e]
                counts[e] += 1
    offsets = [0]
    for c in counts:
        offsets.append(offsets[-1] + (c + 127) // 128 * 128)
    slot = [[-1] * k for _ in range(T)]
    src = [-1] * rows
    for (t, j), p in pos.items():
        s = offsets[int(idx[t, j])] + p
        slot[t][j] = s
        src[s] = t * k + j
    tile_expert = [-1] * (rows // 128)
    for e in range(ne):
        for tile in range(offsets[e] // 128, offsets[e + 1] // 128):
            tile_expert[tile] = e
    return slot, src, counts, offsets, tile_expert


def _check_assign(idx, ne):
    got = ops.moe_assign_sorted(idx, ne)
    assert got[0].data_ptr() != idx.data_ptr() and all(t.dtype == torch.int32 for t in got)
    want = _loop_assign(idx, ne)
    for g, w, name in zip(got, want, ("slot", "src", "counts", "offsets", "tile_expert")):
        assert g.tolist() == w, name
    return got


def _idx(T, ne, k, seed=0):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(T, ne, generator=g) + torch.linspace(-1, 1, ne)
    return ops.moe_route(logits, k)[0]


@pytest.mark.parametrize("T,Ne,k", [(1, 2, 1), (37, 4, 2), (130, 2, 2), (50, 128, 8), (9, 256, 8)])
def test_assign_sorted_reference_against_a_loop(T, Ne, k):
    idx = _idx(T, Ne, k)
    slot, src, counts, offsets, tile_expert = _check_assign(idx, Ne)
    a = torch.arange(T * k, dtype=torch.int32).view(T, k)
    assert torch.equal(src[slot.long()], a)                        # src[slot[a]] == a
    big = T * k + 1                                                # an unbinding capacity: the same pos
    slot_c, _, counts_c = ops.moe_assign_reference(idx, Ne, big)
    assert torch.equal(slot - offsets[idx.long()], slot_c - idx * big) and torch.equal(counts, counts_c)
    assert offsets[0] == 0 and torch.equal(offsets[1:] - offsets[:-1], (counts + 127) // 128 * 128)
    assert src.shape == (ops.moe_sorted_rows(T, Ne, k),) and int((src >= 0).sum()) == T * k
    live = int(offsets[-1]) // 128
    assert (tile_expert[live:] == -1).all() and (tile_expert[:live] >= 0).all()
    # dispatch and combine take the tables as they are
    x = torch.randn(T, 8, generator=torch.Generator().manual_seed(1))
    xe = ops.moe_dispatch(x, slot, src)
    assert torch.equal(xe[slot[:, 0].long()], x) and (xe[src < 0] == 0).all()
    gate = torch.full((T, k), 1.0 / k)
    torch.testing.assert_close(ops.moe_combine(xe, gate, slot, src), x)


def test_assign_sorted_special_counts_and_a_wild_index():
    # expert 0: no tokens; 1: exactly 128; 2: 129; 3: 3 -- in a shuffled order
    idx = torch.cat([torch.full((128,), 1), torch.full((129,), 2), torch.full((3,), 3)]).to(torch.int32)
    idx = idx[torch.randperm(260, generator=torch.Generator().manual_seed(1))].view(260, 1)
    slot, src, counts, offsets, tile_expert = _check_assign(idx, 4)
    assert counts.tolist() == [0, 128, 129, 3] and offsets.tolist() == [0, 0, 128, 384, 512]
    assert tile_expert.tolist() == [1, 2, 2, 3, -1, -1]
    wild = idx.clone()
    wild[5, 0], wild[77, 0] = 4, -1
    slot, src, counts, offsets, tile_expert = _check_assign(wild, 4)
    assert (slot < 0).view(-1).nonzero().view(-1).tolist() == [5, 77] and int(counts.sum()) == 258


def test_assign_sorted_refusals():
    idx = _idx(8, 4, 2)
    with pytest.raises(ValueError):
        ops.moe_assign_sorted(idx.long(), 4)
    with pytest.raises(ValueError):
        ops.moe_assign_sorted(idx, 257)
    with pytest.raises(ValueError):
        ops.moe_assign_sorted(idx[0], 4)
    with pytest.raises(ValueError):
        ops.moe_assign_sorted(idx[:0], 4)


# ------------------------------------------------------------------ 3. the grouped linear against a per-expert loop
def test_grouped_linear_reference_against_a_loop():
    T, Ne, k, K, N = 150, 5, 2, 12, 7
    idx = _idx(T, Ne, k, seed=3)
    idx[idx == 4] = 0                                   # expert 4 gets nothing
    idx[:, 1] = torch.where(idx[:, 1] == idx[:, 0], (idx[:, 0] + 1) % 4, idx[:, 1])
    slot, src, counts, offsets, tile_expert = ops.moe_assign_sorted(idx, Ne)
    assert counts[4] == 0
    g = torch.Generator().manual_seed(4)
    x = torch.randn(src.shape[0], K, dtype=torch.float64, generator=g).requires_grad_()
    ws = [torch.randn(N, K, dtype=torch.float64, generator=g).requires_grad_() for _ in range(Ne)]
    dy = torch.randn(src.shape[0], N, dtype=torch.float64, generator=g)
    y = ops.grouped_linear(x, ws, tile_expert, offsets)
    y.backward(dy)
    got = [y.detach(), x.grad] + [w.grad for w in ws]
    x2 = x.detach().clone().requires_grad_()
    ws2 = [w.detach().clone().requires_grad_() for w in ws]
    off = offsets.tolist()
    parts = [x2[off[e]:off[e + 1]] @ ws2[e].t() for e in range(Ne)]
    y2 = torch.cat(parts + [x2.new_zeros(x2.shape[0] - off[-1], N)])
    y2.backward(dy)
    want = [y2.detach(), x2.grad] + [w.grad if w.grad is not None else torch.zeros_like(w) for w in ws2]
    for a, b in zip(got, want):
        torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12)
    assert (y[off[-1]:] == 0).all() and (x.grad[off[-1]:] == 0).all() and (ws[4].grad == 0).all()
    assert ops.grouped_linear_reference(x, ws, tile_expert, offsets).equal(y)


def test_grouped_linear_refusals():
    x, w = torch.zeros(256, 8), torch.zeros(4, 8)
    te, off = torch.zeros(2, dtype=torch.int32), torch.tensor([0, 256], dtype=torch.int32)
    ops.grouped_linear(x, [w], te, off)
    for bad in ((x[:100], [w], te, off), (x, [], te, off), (x, [w, w[:2]], te, off), (x, [w.double()], te, off),
                (x, [w], te.long(), off), (x, [w], te[:1], off), (x, [w], te, off[:1]), (x, [torch.zeros(4, 9)], te, off)):
        with pytest.raises(ValueError):
            ops.grouped_linear(*bad)


# ------------------------------------------------------------------ 4. the block
def _blocks(**kw):
    torch.manual_seed(0)
    loop = MoEFeedForwardBlock(32, 64, 4, 2, capacity_factor=None, **kw).double()
    grouped = MoEFeedForwardBlock(32, 64, 4, 2, capacity_factor=None, expert_gemm="grouped", **kw).double()
    grouped.load_state_dict(loop.state_dict())
    return loop, grouped


@pytest.mark.parametrize("activation", ["swiglu", "geglu"])
def test_grouped_block_is_the_loop_block_without_a_capacity(activation):
    loop, grouped = _blocks(activation=activation)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(3, 50, 32, dtype=torch.float64, generator=g)
    dy = torch.randn(3, 50, 32, dtype=torch.float64, generator=g)
    outs = []
    for blk in (loop, grouped):
        xi = x.clone().requires_grad_()
        y = blk(xi)
        y.backward(dy)
        outs.append([y.detach(), xi.grad] + [p.grad for p in blk.parameters()])
        assert float(blk.last_drop_fraction) == 0.0
    assert len(outs[0]) == 2 + 2 + 8
    for a, b in zip(*outs):
        assert (a != 0).any()
        torch.testing.assert_close(a, b, rtol=1e-10, atol=1e-12)
    assert torch.equal(loop.last_aux, grouped.last_aux)


def test_expert_gemm_errors():
    with pytest.raises(ValueError, match="capacity_factor=None"):
        MoEFeedForwardBlock(32, 64, 4, 2, expert_gemm="grouped")            # the default factor 1.25
    with pytest.raises(ValueError, match="capacity_factor=None"):
        MoEFeedForwardBlock(32, 64, 4, 2, capacity_factor=1.0, expert_gemm="grouped")
    with pytest.raises(ValueError, match="expert_gemm"):
        MoEFeedForwardBlock(32, 64, 4, 2, expert_gemm="sorted")
    with pytest.raises(ValueError, match="capacity_factor=None"):
        dataclasses.replace(CONFIGS["moe_tiny"], expert_gemm="grouped")
    with pytest.raises(ValueError, match="expert_gemm"):
        dataclasses.replace(CONFIGS["moe_tiny"], expert_gemm="x")
    with pytest.raises(ValueError, match="capacity_factor=None"):
        transformer_blocks(1, 32, 4, 64, 0.0, "swiglu", norm_first=True, norm="rms", bias=False, n_experts=4,
                           expert_gemm="grouped")
    assert MoEFeedForwardBlock(32, 64, 4, 2).expert_gemm == "loop"
    assert LMConfig("x", 1, 8, 1, 8, 10, 4).expert_gemm == "loop"
    names = [f.name for f in dataclasses.fields(LMConfig)]     # with the other MoE fields; qk_norm stays the last
    assert names[names.index("moe_aux_coef") + 1] == "expert_gemm" and names[-1] == "qk_norm"
    cfg = dataclasses.replace(CONFIGS["moe_tiny"], expert_gemm="grouped", capacity_factor=None)
    with torch.device("meta"):
        blocks = build_lm_blocks(cfg)
    assert [b.expert_gemm for b in blocks if isinstance(b, MoEFeedForwardBlock)] == ["grouped"] * 2


# ------------------------------------------------------------------ 5. the planner
def test_moe_cost_prices_the_grouped_rows():
    base = CONFIGS["moe_tiny"]
    cfg = dataclasses.replace(base, expert_gemm="grouped", capacity_factor=None)
    e, f, ne, k = cfg.d_model, cfg.dim_feedforward, cfg.n_experts, cfg.experts_per_token
    for tokens in (None, 384, 8192):
        t = 8 * cfg.seq_len if tokens is None else tokens
        rows = k + 64.0 * ne / t
        want = (3.0 * (2 * e * ne) + 3.0 * 10 * ne
                + rows * (3.0 * (2 * e * 2 * f) + 3.0 * 10 * f + 3.0 * (2 * e * f))
                + 3.0 * 10 * e + 3.0 * 5 * e * (rows + k))
        assert moe_cost(cfg, tokens) == want
    # cheaper than the same model without a capacity on the loop (Ne / k = 2 times the rows), and than factor 1.25
    nodrop = dataclasses.replace(base, capacity_factor=None)
    assert moe_cost(cfg) < moe_cost(base) < moe_cost(nodrop)
    assert block_costs(cfg)[3] == moe_cost(cfg) and block_costs(base)[3] == moe_cost(base)
    assert sum(plan_stages(cfg, 2).balance) == 9


def test_dense_and_loop_configs_plan_as_before():
    dense = CONFIGS["mistral_tiny"]
    assert dense.expert_gemm == "loop" and dense.n_experts is None
    again = dataclasses.replace(dense, capacity_factor=None)   # the MoE fields do not reach a dense plan
    assert block_costs(dense) == block_costs(again)
    assert plan_stages(dense, 2).balance == plan_stages(again, 2).balance
    base = CONFIGS["moe_tiny"]
    rows = base.n_experts * ops.moe_capacity(8 * base.seq_len, base.n_experts, base.experts_per_token, 1.25)
    assert rows == 4 * 960 and moe_cost(base) == moe_cost(dataclasses.replace(base, expert_gemm="loop"))


# ------------------------------------------------------------------ 6. the engine, two gloo ranks
def test_moe_grouped_engine_two_gloo_ranks(monkeypatch):
    """helpers.engine_cases.run_engine_case on the grouped replica, as test_moe_engine_two_gloo_ranks does for the
    loop: every gradient of every rank is compared with the single-rank engine's."""
    monkeypatch.setattr(engine_cases, "case_cfg", moe_grouped_engine.moe_cfg)
    monkeypatch.setattr(engine_cases, "worker", moe_grouped_engine.worker)
    monkeypatch.setattr(engine_cases, "PipelineEngine", moe_grouped_engine.checked_engine)
    single = engine_cases.single_rank_reference
    seen = {}

    def spy(*args, **kwargs):
        out = single(*args, **kwargs)
        seen.update(out[1])
        return out

    monkeypatch.setattr(engine_cases, "single_rank_reference", spy)
    engine_cases.run_engine_case("cpu", 2, "except_last", 1, False, False)
    experts = [n for n in seen if "experts_w" in n]
    assert len(experts) == 16 and any((seen[n] != 0).any() for n in experts)
