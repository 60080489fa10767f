"""Attention sinks off the GPU: ``attention_reference(sinks=)`` against an independent fp64 concat-softmax under
every mask, its gradients (``dsinks`` included) by ``gradcheck``, the ``-inf`` sink, the argument checks, the
modules and ``LMConfig`` fields, the ``sink_tiny`` config and its costs, and the pipeline engine on two gloo ranks.
The kernels are in tests/test_gpu_sink_kernels.py."""
import dataclasses
import math

import pytest
import torch

from helpers import engine_cases, sink_engine

from mipipe import ops
from mipipe.models import CONFIGS, LMConfig, build_lm_blocks
from mipipe.models.transformer import (AttentionCore, SelfAttentionBlock, TransformerEncoderLayer, block_flops,
                                       transformer_blocks)
from mipipe.parallel.stage import block_costs

B, H, S, D = 2, 4, 24, 16


def _inputs(dtype=torch.float32, seed=0, heads=H, hkv=H, s=S, d=D):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, heads, s, d, generator=g, dtype=torch.float64).to(dtype)
    k = torch.randn(B, hkv, s, d, generator=g, dtype=torch.float64).to(dtype)
    v = torch.randn(B, hkv, s, d, generator=g, dtype=torch.float64).to(dtype)
    return q, k, v


def _docs(s=S):
    """Two rows of documents whose edges are not shared: lengths (5, 11, 8) and (24,)."""
    rows = []
    for lens in ((5, 11, 8), (s,)):
        start = torch.cat([torch.full((n,), sum(lens[:i])) for i, n in enumerate(lens)])
        end = torch.cat([torch.full((n,), sum(lens[:i + 1])) for i, n in enumerate(lens)])
        rows.append(torch.stack((start, end)))
    return torch.stack(rows).to(torch.int32)


def _concat_softmax(q, k, v, sinks, causal, window=None, softcap=None, docs=None):
    """fp64, masks from ``arange``, the sink as one more column of the scores: Hugging Face gpt-oss's
    ``softmax(cat([scores, sinks], -1))[..., :-1]``."""
    q, k, v = q.double(), k.double(), v.double()
    g = q.shape[1] // k.shape[1]
    k, v = k.repeat_interleave(g, 1), v.repeat_interleave(g, 1)
    n = q.shape[-2]
    s = q @ k.transpose(-1, -2) / math.sqrt(q.shape[-1])
    if softcap is not None:
        s = softcap * torch.tanh(s / softcap)
    i, j = torch.arange(n)[:, None], torch.arange(n)[None, :]
    if causal:
        s = s.masked_fill(j > i, float("-inf"))
    if window is not None:
        s = s.masked_fill(j <= i - window, float("-inf"))
    if docs is not None:
        s = s.masked_fill((j[None] < docs[:, 0].long()[:, :, None])[:, None], float("-inf"))
    col = sinks.double().view(1, -1, 1, 1).expand(s.shape[0], -1, n, 1)
    return torch.softmax(torch.cat((s, col), dim=-1), dim=-1)[..., :-1] @ v


# ------------------------------------------------------------------ 1. the reference
@pytest.mark.parametrize("causal,window,softcap,docs", [
    (False, None, None, False), (True, None, None, False), (True, 5, None, False), (False, None, 2.0, False),
    (True, None, 2.0, False), (True, 5, 2.0, False), (True, None, None, True), (True, 5, 2.0, True)])
@pytest.mark.parametrize("sink_dtype", [torch.float32, torch.float64])
def test_reference_against_concat_softmax(causal, window, softcap, docs, sink_dtype):
    q, k, v = _inputs(torch.float64)
    sinks = torch.linspace(-1.0, 4.0, H, dtype=sink_dtype)
    bounds = _docs() if docs else None
    ref = _concat_softmax(q, k, v, sinks, causal, window, softcap, bounds)
    out = ops.attention_reference(q, k, v, causal, 0.0, window=window, softcap=softcap, doc_bounds=bounds,
                                  sinks=sinks)
    assert out.dtype == torch.float64 and (out - ref).abs().max().item() < 1e-12
    plain = ops.attention_reference(q, k, v, causal, 0.0, window=window, softcap=softcap, doc_bounds=bounds)
    assert (out - plain).abs().max().item() > 1e-2  # the sinks really take mass
    # fp32 inputs: fp32 math, the reference's own precision
    out32 = ops.attention_reference(q.float(), k.float(), v.float(), causal, 0.0, window=window, softcap=softcap,
                                    doc_bounds=bounds, sinks=sinks.float())
    assert out32.dtype == torch.float32 and (out32.double() - ref).abs().max().item() < 1e-5


def test_ops_on_the_cpu_are_the_reference_and_gqa_sinks_are_per_query_head():
    q, k, v = _inputs(torch.float32, seed=1, heads=4, hkv=2)
    sinks = torch.linspace(0.0, 3.0, 4)
    ref = _concat_softmax(q, k, v, sinks, True, 5)
    assert (ops.attention(q, k, v, causal=True, window=5, sinks=sinks).double() - ref).abs().max().item() < 1e-5
    qkv = torch.cat([t.transpose(1, 2) for t in (q, k, v)], dim=2).contiguous()  # [B, S, H + 2 Hkv, D]
    o = ops.attention_gqa_packed(qkv, 2, causal=True, window=5, sinks=sinks)
    assert (o.transpose(1, 2).double() - ref).abs().max().item() < 1e-5
    q, k, v = _inputs(torch.float32, seed=2)
    packed = torch.stack([t.transpose(1, 2) for t in (q, k, v)], dim=2).contiguous()
    o = ops.attention_packed(packed, causal=False, sinks=sinks)
    assert (o.transpose(1, 2).double() - _concat_softmax(q, k, v, sinks, False)).abs().max().item() < 1e-5


@pytest.mark.parametrize("causal,window,softcap", [(False, None, None), (True, None, None), (True, 3, 2.0)])
def test_gradcheck_with_dsinks(causal, window, softcap):
    q, k, v = (t.requires_grad_() for t in _inputs(torch.float64, seed=3, heads=2, hkv=2, s=8, d=4))
    sinks = torch.tensor([0.5, -1.0], dtype=torch.float64, requires_grad=True)

    def f(q, k, v, sinks):
        return ops.attention(q, k, v, causal=causal, window=window, softcap=softcap, sinks=sinks)

    assert torch.autograd.gradcheck(f, (q, k, v, sinks))
    # and dsinks is the closed form: -sum_{b,i} p_sink * delta, delta = rowsum(dO * O)
    o = f(q, k, v, sinks)
    do = torch.randn(o.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    (ds,) = torch.autograd.grad(o, sinks, do)
    with torch.no_grad():
        s = q @ k.transpose(-1, -2) / 2.0
        if softcap is not None:
            s = softcap * torch.tanh(s / softcap)
        i, j = torch.arange(8)[:, None], torch.arange(8)[None, :]
        if causal:
            s = s.masked_fill(j > i, float("-inf"))
        if window is not None:
            s = s.masked_fill(j <= i - window, float("-inf"))
        col = sinks.view(1, -1, 1, 1).expand(B, -1, 8, 1)
        lse = torch.logsumexp(torch.cat((s, col), -1), -1)
        closed = -(torch.exp(sinks.view(1, -1, 1) - lse) * (do * o).sum(-1)).sum((0, 2))
    assert (ds - closed).abs().max().item() < 1e-12


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_minus_inf_sinks_are_the_sinkless_bits(dtype):
    q, k, v = _inputs(dtype, seed=5)
    none = torch.full((H,), float("-inf"))
    for causal, window, softcap in ((False, None, None), (True, None, None), (True, 5, 2.0)):
        a = ops.attention_reference(q, k, v, causal, 0.0, window=window, softcap=softcap, sinks=none)
        b = ops.attention_reference(q, k, v, causal, 0.0, window=window, softcap=softcap)
        assert torch.equal(a, b)
    leaves = [t.clone().requires_grad_() for t in (q, k, v)]
    sk = none.clone().requires_grad_()
    ops.attention(*leaves, causal=True, sinks=sk).float().sum().backward()
    assert torch.equal(sk.grad, torch.zeros(H)) and all(torch.isfinite(t.grad.float()).all() for t in leaves)
    # one head without a sink among heads with one
    mixed = torch.tensor([1.0, float("-inf"), 2.0, 0.0])
    a = ops.attention_reference(q, k, v, True, 0.0, sinks=mixed)
    b = ops.attention_reference(q, k, v, True, 0.0)
    assert torch.equal(a[:, 1], b[:, 1]) and not torch.equal(a[:, 0], b[:, 0])


def test_large_sink_is_finite():
    q, k, v = _inputs(torch.float32, seed=6)
    o = ops.attention_reference(q, k, v, True, 0.0, sinks=torch.full((H,), 100.0))
    assert torch.isfinite(o).all() and o.abs().max().item() < 1e-30


# ------------------------------------------------------------------ 2. the argument checks
def test_sinks_argument_checks():
    q, k, v = _inputs(torch.float32)
    packed = torch.stack([t.transpose(1, 2) for t in (q, k, v)], dim=2).contiguous()
    gqa = torch.cat([t.transpose(1, 2) for t in (q, k[:, :2], v[:, :2])], dim=2).contiguous()
    calls = (lambda s: ops.attention(q, k, v, causal=True, sinks=s),
             lambda s: ops.attention_packed(packed, causal=True, sinks=s),
             lambda s: ops.attention_gqa_packed(gqa, 2, causal=True, sinks=s),
             lambda s: ops.attention_reference(q, k, v, True, 0.0, sinks=s))
    bad = (torch.zeros(H + 1), torch.zeros(2), torch.zeros(1, H), torch.zeros(H, 1), torch.zeros(()),
           torch.zeros(H, dtype=torch.float64), torch.zeros(H, dtype=torch.bfloat16),
           torch.zeros(H, dtype=torch.int32), [0.0] * H, 0.0)
    for call in calls:
        for s in bad:
            with pytest.raises(ValueError, match="sinks"):
                call(s)
        assert call(torch.zeros(H)).shape == call(None).shape
    # the activations' dtype is allowed next to fp32, and the gradient comes back in the sinks' dtype
    qb, kb, vb = (t.bfloat16() for t in (q, k, v))
    for dt in (torch.float32, torch.bfloat16):
        sk = torch.zeros(H, dtype=dt, requires_grad=True)
        ops.attention(qb, kb, vb, causal=True, sinks=sk).float().sum().backward()
        assert sk.grad.dtype == dt and sk.grad.abs().max() > 0
    # under grouped-query attention the length is the number of QUERY heads
    with pytest.raises(ValueError, match="sinks"):
        ops.attention_gqa_packed(gqa, 2, causal=True, sinks=torch.zeros(2))


# ------------------------------------------------------------------ 3. the modules
def test_default_off_registers_nothing():
    kw = dict(norm_first=True, causal=True, layer_norm_eps=1e-5, n_kv_heads=2)
    torch.manual_seed(0)
    off = AttentionCore(32, 4, 0.0, **kw)
    torch.manual_seed(0)
    on = AttentionCore(32, 4, 0.0, attn_sinks=True, **kw)
    assert off.attn_sinks is False and not hasattr(off, "sinks")
    assert set(on.state_dict()) - set(off.state_dict()) == {"sinks"}
    assert on.sinks.shape == (4,) and torch.equal(on.sinks.detach(), torch.zeros(4))
    assert not getattr(on.sinks, "_mipipe_gemm_weight", False)  # the attention backward writes its gradient
    assert torch.equal(on.in_proj_weight, off.in_proj_weight)   # the other parameters draw what they drew
    assert AttentionCore(32, 4, 0.0, attn_sinks=True, dtype=torch.bfloat16, **kw).sinks.dtype == torch.bfloat16
    for mod in (SelfAttentionBlock(32, 4, 0.0, norm_first=True, causal=True),
                TransformerEncoderLayer(32, 4, 64, 0.0, norm_first=True, causal=True),
                torch.nn.Sequential(*transformer_blocks(2, 32, 4, 64, 0.0, norm_first=True, causal=True))):
        assert not any(n.endswith("sinks") for n in mod.state_dict())
    assert "core.sinks" in SelfAttentionBlock(32, 4, 0.0, causal=True, attn_sinks=True).state_dict()
    assert "0.core.sinks" in TransformerEncoderLayer(32, 4, 64, 0.0, attn_sinks=True).state_dict()
    blocks = torch.nn.Sequential(*transformer_blocks(2, 32, 4, 64, 0.0, causal=True, attn_sinks=True))
    assert [n for n in blocks.state_dict() if n.endswith("sinks")] == ["0.core.sinks", "2.core.sinks"]
    assert LMConfig("x", 1, 32, 4, 64, 100, 8).attn_sinks is False


@pytest.mark.parametrize("kw", [dict(), dict(n_kv_heads=2), dict(n_kv_heads=2, window=5, rope=True),
                                dict(qk_norm=True, n_kv_heads=2), dict(qk_norm=True, attn_softcap=2.0),
                                dict(causal=False)])
def test_core_passes_its_sinks_to_the_op(kw):
    """Every branch of the core's forward (packed, grouped-query, rotated, QK-normed) uses the parameter: moving it
    moves the output, and -inf gives the core without sinks."""
    kw = dict(dict(norm_first=True, causal=True, layer_norm_eps=1e-5), **kw)
    torch.manual_seed(0)
    on = AttentionCore(32, 4, 0.0, attn_sinks=True, **kw)
    torch.manual_seed(0)
    off = AttentionCore(32, 4, 0.0, **kw)
    x = torch.randn(2, 12, 32, generator=torch.Generator().manual_seed(1))
    y0 = on(x)
    with torch.no_grad():
        on.sinks.copy_(torch.linspace(1.0, 3.0, 4))
    y1 = on(x)
    assert not torch.equal(y0, y1) and not torch.equal(y0, off(x))
    y1.sum().backward()
    assert on.sinks.grad is not None and (on.sinks.grad != 0).all()
    with torch.no_grad():
        on.sinks.fill_(float("-inf"))
    assert torch.equal(on(x), off(x))


def test_core_sinks_under_documents():
    torch.manual_seed(0)
    core = AttentionCore(32, 4, 0.0, norm_first=True, causal=True, layer_norm_eps=1e-5, attn_sinks=True)
    x = torch.randn(2, S, 32, generator=torch.Generator().manual_seed(2))
    with ops.use_documents(_docs()):
        y = core(x)
    assert not torch.equal(y, core(x))
    # the first document of row 0 alone is that document's rows
    assert torch.allclose(y[0, :5], core(x[:, :5])[0], atol=1e-6)


# ------------------------------------------------------------------ 4. the config and the costs
def test_sink_tiny_is_what_its_notes_say():
    cfg, base = CONFIGS["sink_tiny"], CONFIGS["mistral_tiny"]
    assert cfg.attn_sinks is True and cfg.global_every is None
    assert dataclasses.replace(cfg, name=base.name, attn_sinks=False, notes=base.notes) == base
    assert cfg.params() == base.params() + cfg.num_layers * cfg.nhead
    with torch.device("meta"):
        blocks = build_lm_blocks(cfg)
    dec = blocks[-1]
    pad = (dec.weight.shape[0] - cfg.vocab) * (cfg.d_model + 1)  # the decoder's zero rows, which params() leaves out
    assert sum(p.numel() for b in blocks for p in b.parameters()) - pad == cfg.params()
    cores = [b.core for b in blocks if isinstance(b, SelfAttentionBlock)]
    assert len(cores) == 2 and all(c.attn_sinks and c.sinks.shape == (4,) and c.window == 48 for c in cores)
    assert not [n for n, _ in torch.nn.Sequential(*build_lm_blocks(dataclasses.replace(
        sink_engine.sink_cfg(), attn_sinks=False))).named_parameters() if "sinks" in n]


def test_sinks_add_no_flops():
    cfg, base = CONFIGS["sink_tiny"], CONFIGS["mistral_tiny"]
    assert block_costs(cfg) == block_costs(base)
    kw = dict(norm_first=True, causal=True, layer_norm_eps=1e-5, n_kv_heads=2)
    assert (AttentionCore(32, 4, 0.0, attn_sinks=True, **kw).flops_per_token(64)
            == AttentionCore(32, 4, 0.0, **kw).flops_per_token(64))
    with torch.device("meta"):
        blk = build_lm_blocks(cfg)[1]
    assert block_flops(blk, cfg.seq_len) == 3.0 * blk.flops_per_token(cfg.seq_len)


def test_sink_tiny_cpu_step_changes_sinks():
    cfg = sink_engine.sink_cfg()
    torch.manual_seed(0)
    model = torch.nn.Sequential(*build_lm_blocks(cfg)).train()
    tok = torch.randint(0, cfg.vocab, (4, cfg.seq_len + 1), generator=torch.Generator().manual_seed(7))
    x, t = tok[:, :-1], tok[:, 1:].contiguous()
    loss_fn = lambda y: ops.cross_entropy(y.reshape(-1, cfg.vocab), t.reshape(-1))  # noqa: E731
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    loss = loss_fn(model(x))
    loss.backward()
    loss = loss.detach()
    assert math.isfinite(float(loss)) and all(p.grad is not None and torch.isfinite(p.grad).all()
                                              for p in model.parameters())
    sinks = [b.core.sinks for b in model if isinstance(b, SelfAttentionBlock)]
    assert len(sinks) == 2 and all((s.grad != 0).all() for s in sinks)
    opt.step()
    assert all((s.detach() != 0).all() for s in sinks)
    # the sinks are really in the softmax: the same weights without them give another loss
    with torch.no_grad():
        for s in sinks:
            s.fill_(float("-inf"))
        assert float(loss_fn(model(x))) != float(loss)


# ------------------------------------------------------------------ 5. the engine, two gloo ranks
def test_sink_engine_two_gloo_ranks(monkeypatch):
    """helpers.engine_cases.run_engine_case as test_engine.py runs it, on the replica with sinks: the spawned
    ranks start in helpers.sink_engine.worker, which swaps the helper's config and runs its worker.  Every
    gradient of every rank is compared with the single-rank engine's, both ``sinks`` among them."""
    monkeypatch.setattr(engine_cases, "case_cfg", sink_engine.sink_cfg)
    monkeypatch.setattr(engine_cases, "worker", sink_engine.worker)
    single = engine_cases.single_rank_reference
    seen = {}

    def spy(*args, **kwargs):
        out = single(*args, **kwargs)
        seen.update(out[1])
        return out

    monkeypatch.setattr(engine_cases, "single_rank_reference", spy)
    engine_cases.run_engine_case("cpu", 2, "except_last", 1, False, False)
    names = [n for n in seen if n.endswith("core.sinks")]
    assert len(names) == 2 and all(seen[n].shape == (4,) and (seen[n] != 0).all() for n in names)
