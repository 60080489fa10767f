"""The LLaMA-style block on the CPU: the eager references of RMSNorm, SwiGLU
and RoPE against independent formulations, the autograd wrappers' CPU paths,
and a small RMSNorm / SwiGLU / RoPE / bias-free model through the pipeline
units, ``Pipe`` and the engine.  The HIP kernels behind the same ops are
tested in test_gpu_llama_kernels.py."""
import copy
import dataclasses

import pytest
import torch
import torch.nn.functional as F

from mipipe import Pipe, ops
from mipipe.models import CONFIGS, TargetSequential, build_lm_blocks, lm_pipeline_units
from mipipe.models.transformer import merge_units
from mipipe.optim import FlatAdam
from mipipe.parallel import PipelineEngine
from mipipe.parallel.stage import block_costs


# ------------------------------------------------------------------ references
@pytest.mark.parametrize("residual", [False, True])
def test_rms_norm_reference_matches_torch(residual):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(5, 24, dtype=torch.float64, generator=g)
    res = torch.randn(5, 24, dtype=torch.float64, generator=g) if residual else None
    w = 1 + 0.1 * torch.randn(24, dtype=torch.float64, generator=g)
    y = ops.rms_norm_reference(x, res, w, 1e-6, 0.0, True)
    ref = F.rms_norm(x + res if residual else x, (24,), w, 1e-6)
    assert y.dtype == torch.float64
    assert torch.allclose(y, ref, rtol=0, atol=1e-13)


def test_swiglu_reference_matches_silu_times_up():
    g = torch.Generator().manual_seed(1)
    gu = 3 * torch.randn(7, 32, dtype=torch.float64, generator=g)
    ref = F.silu(gu[:, :16]) * gu[:, 16:]
    assert torch.allclose(ops.swiglu_reference(gu), ref, rtol=0, atol=1e-14)
    assert torch.equal(ops.swiglu(gu), ops.swiglu_reference(gu))  # CPU tensors take the reference


def test_swiglu_reference_neg_inf_gate():
    """silu's limit at -inf: h = 0 and zero gradients, where F.silu gives nan."""
    gu = torch.tensor([[float("-inf"), 1.0, 2.0, 3.0]], dtype=torch.float64, requires_grad=True)
    h = ops.swiglu_reference(gu)
    assert h[0, 0].item() == 0.0 and torch.isfinite(h).all()
    h.sum().backward()
    assert torch.isfinite(gu.grad).all() and gu.grad[0, 0].item() == 0.0 and gu.grad[0, 2].item() == 0.0


def _rope_complex(qkv, cos, sin, pos0):
    """Halves (a, b) as a + ib times r exp(i angle), angle and modulus (1 to fp32 rounding)
    taken from the tables the reference reads."""
    B, S, _, H, D = qkv.shape
    c, s = cos[pos0:pos0 + S].double(), sin[pos0:pos0 + S].double()
    rot = torch.polar(torch.hypot(c, s), torch.atan2(s, c)).view(1, S, 1, 1, D // 2)
    qk = qkv[:, :, :2]
    z = torch.complex(qk[..., :D // 2], qk[..., D // 2:]) * rot
    return torch.cat((torch.cat((z.real, z.imag), dim=-1), qkv[:, :, 2:]), dim=2)


ROPE_SHAPE = (2, 8, 3, 64)  # B, S, H, D


@pytest.mark.parametrize("pos0", [0, 5])
def test_rope_reference_matches_complex_rotation(pos0):
    B, S, H, D = ROPE_SHAPE
    qkv = torch.randn(B, S, 3, H, D, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    cos, sin = ops.rope_tables(pos0 + S, D)
    assert cos.dtype == torch.float32 and cos.shape == (pos0 + S, D // 2)
    out = ops.rope_reference(qkv, cos, sin, pos0)
    assert out.dtype == torch.float64
    assert (out - _rope_complex(qkv, cos, sin, pos0)).abs().max().item() < 1e-12
    assert torch.equal(out[:, :, 2], qkv[:, :, 2])


def test_rope_tables_angles():
    cos, sin = ops.rope_tables(16, 64, 10000.0)
    i = torch.arange(32, dtype=torch.float64)
    ang = torch.arange(16, dtype=torch.float64)[:, None] * 10000.0 ** (-2 * i / 64)
    assert torch.equal(cos, ang.cos().float()) and torch.equal(sin, ang.sin().float())


def test_rope_reference_inverse_returns_input():
    B, S, H, D = ROPE_SHAPE
    qkv = torch.randn(B, S, 3, H, D, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    cos, sin = ops.rope_tables(S + 5, D)
    back = ops.rope_reference(ops.rope_reference(qkv, cos, sin, 5), cos, sin, 5, inverse=True)
    # cos^2 + sin^2 of the fp32 tables is 1 to 2^-23
    assert (back - qkv).abs().max().item() < 1e-6


def test_rope_scores_depend_on_relative_position_only():
    """q'.k' is unchanged when pos0 shifts both (angles built in fp64 here, so the
    identity holds to fp64 rounding)."""
    B, S, H, D = ROPE_SHAPE
    qkv = torch.randn(B, S, 3, H, D, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    i = torch.arange(D // 2, dtype=torch.float64)
    ang = torch.arange(S + 5, dtype=torch.float64)[:, None] * 10000.0 ** (-2 * i / D)
    cos, sin = ang.cos(), ang.sin()

    def scores(pos0):
        r = ops.rope_reference(qkv, cos, sin, pos0)
        return torch.einsum("bshd,bthd->bhst", r[:, :, 0], r[:, :, 1])

    assert (scores(0) - scores(5)).abs().max().item() < 1e-10


# ------------------------------------------------------------------ autograd wrappers, CPU paths
def test_gradcheck_rms_norm():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 16, dtype=torch.float64, generator=g, requires_grad=True)
    res = torch.randn(3, 16, dtype=torch.float64, generator=g, requires_grad=True)
    w = (1 + 0.1 * torch.randn(16, dtype=torch.float64, generator=g)).requires_grad_()
    assert torch.autograd.gradcheck(lambda a, r, ww: ops.add_dropout_rms_norm(a, r, ww, 1e-5, 0.0, True), (x, res, w))
    assert torch.autograd.gradcheck(lambda a, ww: sum(ops.rms_norm_fanout(a, ww, 1e-5)), (x, w))


def test_gradcheck_swiglu():
    gu = torch.randn(3, 16, dtype=torch.float64, generator=torch.Generator().manual_seed(6), requires_grad=True)
    assert ops.swiglu(gu).shape == (3, 8)
    assert torch.autograd.gradcheck(ops.swiglu, (gu,))


def test_gradcheck_rope_packed():
    qkv = torch.randn(2, 3, 3, 2, 16, dtype=torch.float64, generator=torch.Generator().manual_seed(7),
                      requires_grad=True)
    cos, sin = ops.rope_tables(8, 16)
    assert torch.autograd.gradcheck(lambda t: ops.rope_packed(t, cos.double(), sin.double(), 2), (qkv,))
    with pytest.raises(ValueError):
        ops.rope_packed(qkv[:, :, :2], cos, sin)


# ------------------------------------------------------------------ the model
def _cfg(**kw):
    return dataclasses.replace(CONFIGS["llama_tiny"], d_model=32, nhead=4, dim_feedforward=64, vocab=100, seq_len=8,
                               **kw)


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


def test_llama_block_has_what_it_says():
    cfg = _cfg()
    blocks = _blocks(cfg)
    names = [n for n, _ in torch.nn.Sequential(*blocks).named_parameters()]
    assert not any("bias" in n for n in names[:-1]) and names[-1].endswith("bias")  # only the decoder's
    assert not hasattr(blocks[0], "pe") and not hasattr(blocks[0], "pos_weight")
    mlp = blocks[2]
    assert mlp.fc_in.linear1_weight.shape == (2 * cfg.dim_feedforward, cfg.d_model)
    assert mlp.fc_out.linear2_weight.shape == (cfg.d_model, cfg.dim_feedforward)
    assert blocks[1].core.rope and blocks[1].core.rope_cos.shape[0] == 0  # grown on demand
    x, _ = _data(cfg, 2)
    torch.nn.Sequential(*blocks)(x)
    assert blocks[1].core.rope_cos.shape == (cfg.seq_len, cfg.d_model // cfg.nhead // 2)
    assert "rope_cos" not in blocks[1].core.state_dict()


def test_llama_position_dependence():
    """No position table at the embedding: the positions enter through RoPE, so a
    causal model's logits at the last token change when the earlier tokens swap."""
    cfg = _cfg()
    model = torch.nn.Sequential(*_blocks(cfg)).eval()
    x, _ = _data(cfg, 1)
    x[0, 0], x[0, 1] = 3, 4
    y = model(x)
    x2 = x.clone()
    x2[0, 0], x2[0, 1] = 4, 3
    assert not torch.allclose(y[0, -1], model(x2)[0, -1], atol=1e-6)


def test_swiglu_dropout_between_gate_and_linear2_raises():
    cfg = _cfg(act_dropout=0.1)
    model = torch.nn.Sequential(*_blocks(cfg)).train()
    with pytest.raises(ValueError, match="swiglu"):
        model(_data(cfg, 2)[0])
    model.eval()
    model(_data(cfg, 2)[0])  # not in training mode: no dropout, no error


def test_llama_units_merged_and_plain_agree():
    cfg = _cfg()
    x, t = _data(cfg, 4)
    plain = torch.nn.Sequential(*_blocks(cfg)).train()
    units = TargetSequential(*lm_pipeline_units(_blocks(cfg))).train()
    merged = TargetSequential(*merge_units(lm_pipeline_units(_blocks(cfg)))).train()
    assert len(units) == 1 + 4 * cfg.num_layers + 2 and len(merged) == len(plain)
    loss0, g0 = _run(plain, cfg, x, t)
    for name, seq in (("units", units), ("merged", merged)):
        loss, g = _run(seq, cfg, x, t)
        assert abs(loss - loss0) <= 1e-5 * abs(loss0), name
        assert len(g) == len(g0)
        for a, b, (n, _) in zip(g, g0, plain.named_parameters()):
            _assert_rel(a, b, (name, n))


@pytest.mark.parametrize("checkpoint", ["never", "except_last", "always"])
def test_llama_pipe_two_cpu_partitions(checkpoint):
    cfg = _cfg()
    x, t = _data(cfg, 8)
    blocks = _blocks(cfg)
    ref = torch.nn.Sequential(*copy.deepcopy(blocks)).train()
    loss0, g0 = _run(ref, cfg, x, t)
    model = torch.nn.Sequential(*blocks).train()
    pipe = Pipe(model, chunks=4, checkpoint=checkpoint, balance=[3, len(blocks) - 3], copy_same_device=True)
    try:
        assert len(pipe.partitions) == 2
        loss = _loss_fn(cfg)(pipe(x).local_value(), t)
        loss.backward()
    finally:
        pipe.close()
    assert abs(float(loss.detach()) - loss0) <= 1e-5 * abs(loss0)
    for (n, p), b in zip(model.named_parameters(), g0):
        _assert_rel(p.grad, b, n)


def test_llama_engine_single_rank_flat_adam():
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


# ------------------------------------------------------------------ bookkeeping
def _decoder_padding(cfg):
    """Zero rows (weight and bias) that pad the decoder's vocabulary to a multiple of 256."""
    return ((cfg.vocab + 255) // 256 * 256 - cfg.vocab) * (cfg.d_model + 1)


@pytest.mark.parametrize("name", ["llama_tiny", "tiny", "gpt2_xl", "llama2_7b"])
def test_params_matches_built_model(name):
    cfg = CONFIGS[name]
    with torch.device("meta"):
        blocks = build_lm_blocks(cfg)
    count = sum(p.numel() for b in blocks for p in b.parameters())
    assert cfg.params() == count - _decoder_padding(cfg)
    assert len(block_costs(cfg)) == len(lm_pipeline_units(blocks))


def test_llama2_7b_is_llama2_7b():
    cfg = CONFIGS["llama2_7b"]
    # the published 6,738,415,616 plus the decoder's 32,000 bias entries
    assert cfg.params() == 6_738_415_616 + 32_000
    gated, plain = block_costs(cfg), block_costs(dataclasses.replace(cfg, activation="gelu"))
    assert gated[3] > 1.9 * plain[3] and gated[1] == plain[1] and gated[4] == plain[4]  # only the first MLP GEMM doubles


TINY_PARAMS = [
    ("0.weight", (1000, 256)),
    ("1.core.in_proj_weight", (768, 256)), ("1.core.in_proj_bias", (768,)),
    ("1.out.out_proj_weight", (256, 256)), ("1.out.out_proj_bias", (256,)),
    ("1.out.norm_weight", (256,)), ("1.out.norm_bias", (256,)),
    ("2.fc_in.linear1_weight", (512, 256)), ("2.fc_in.linear1_bias", (512,)),
    ("2.fc_out.linear2_weight", (256, 512)), ("2.fc_out.linear2_bias", (256,)),
    ("2.fc_out.norm_weight", (256,)), ("2.fc_out.norm_bias", (256,)),
    ("3.core.in_proj_weight", (768, 256)), ("3.core.in_proj_bias", (768,)),
    ("3.out.out_proj_weight", (256, 256)), ("3.out.out_proj_bias", (256,)),
    ("3.out.norm_weight", (256,)), ("3.out.norm_bias", (256,)),
    ("4.fc_in.linear1_weight", (512, 256)), ("4.fc_in.linear1_bias", (512,)),
    ("4.fc_out.linear2_weight", (256, 512)), ("4.fc_out.linear2_bias", (256,)),
    ("4.fc_out.norm_weight", (256,)), ("4.fc_out.norm_bias", (256,)),
    ("5.weight", (1024, 256)), ("5.bias", (1024,)),
]


def test_default_config_is_untouched():
    with torch.device("meta"):
        model = torch.nn.Sequential(*build_lm_blocks(CONFIGS["tiny"]))
    assert [(n, tuple(p.shape)) for n, p in model.named_parameters()] == TINY_PARAMS
    assert [n for n, _ in model.named_buffers()] == ["0.pe"]
    cfg = CONFIGS["tiny"]
    assert (cfg.norm, cfg.bias, cfg.rope, cfg.encoder_positions()) == ("layer", True, False, "sinusoidal")
    assert CONFIGS["gpt2_xl"].encoder_positions() == "learned"
