"""Attention sinks on the GPU: the generic forward kernels with the sink folded in after the key loop (non-causal,
causal, causal + window; soft cap; documents; grouped-query heads; dropout; checkpoint recompute), the sinkless
backward kernels on the forward's ``lse``, the ``dsinks`` reduction, the dispatch that keeps a call with sinks off
the S = 128, wide and long-sequence kernels, the padded shapes and the eager fallbacks, the binding's refusals and
the ``sink_tiny`` model.  Everything here but the stated fallbacks runs native code from mipipe/_C.so: the tests
fail if the extension is missing.

Random ``randn`` inputs have scores of about N(0, 1) and an ``lse`` of 2 to 5, so sinks of ``linspace(3, 6, H)``
take a third to nine tenths of each row's mass: the fp64 references with and without them differ beyond the bf16
bound in at least a quarter of the elements of each of ``o``, ``dq``, ``dk`` and ``dv`` -- asserted before every
comparison, so a kernel that ignored the sinks cannot pass (``linspace(0, 2)`` moves under a tenth)."""
import copy
import math
import sys
import warnings

import pytest
import torch

from helpers.gqa_cases import gqa_inputs
from test_gpu_document_kernels import _bounds, _keep
from test_gpu_kernels import _attn_keep_mask, _tol
from test_gpu_llama_kernels import _assert_model_close, _data, _loss_fn

from mipipe import checkpoint, ops
from mipipe.models import CONFIGS, build_lm_blocks
from mipipe.models.transformer import AttentionCore, SelfAttentionBlock
from mipipe.optim import FlatAdam

pytestmark = pytest.mark.gpu

DEV = "cuda"
B = 2
NEG_INF = float("-inf")


@pytest.fixture(scope="module")
def k():
    from mipipe._native_loader import kernels

    return kernels()


def _sinks(H):
    return torch.linspace(3.0, 6.0, H, device=DEV)


def _reference(qkv, do, H, Hkv, sinks, causal=True, W=None, cap=None, lengths=None, keep=None, p=0.0,
               dtype=torch.float64):
    """Attention on ``qkv [B, S, H + 2 Hkv, D]`` with repeated K/V heads, every step in ``dtype``: the scores
    capped, masked from ``arange`` (or document ids), then the sink as one more column of the softmax (``sinks =
    None``: none).  Returns (o [B, S, H, D], dqkv, dsinks, bound): ``bound[h] = sum_{b,i} p_sink |delta|``, the
    size of the terms ``dsinks[h]`` sums."""
    x = qkv.to(dtype).requires_grad_()
    sk = None if sinks is None else sinks.to(dtype).clone().requires_grad_()
    q, kk, v = (t.transpose(1, 2) for t in (x[:, :, :H], x[:, :, H:H + Hkv], x[:, :, H + Hkv:]))
    g = H // Hkv
    kk, v = kk.repeat_interleave(g, 1), v.repeat_interleave(g, 1)
    S = q.shape[-2]
    s = torch.matmul(q, kk.transpose(-1, -2)) / math.sqrt(q.shape[-1])
    if cap is not None:
        s = cap * torch.tanh(s / cap)
    i = torch.arange(S, device=s.device)[:, None]
    j = torch.arange(S, device=s.device)[None, :]
    if lengths is not None:
        s = s.masked_fill(~_keep(lengths, S, W, s.device)[:, None], NEG_INF)
    else:
        if causal:
            s = s.masked_fill(j > i, NEG_INF)
        if W is not None:
            s = s.masked_fill(j <= i - W, NEG_INF)
    if sk is not None:
        full = torch.cat((s, sk.view(1, H, 1, 1).expand(s.shape[0], H, S, 1)), dim=-1)
        pr = torch.softmax(full, dim=-1)[..., :-1]
    else:
        pr = torch.softmax(s, dim=-1)
    if keep is not None:
        pr = pr * keep.to(pr.device).to(dtype) / (1 - p)
    o = torch.matmul(pr, v)
    dout = do.to(dtype).transpose(1, 2)
    o.backward(dout)
    if sk is None:
        return o.detach().transpose(1, 2), x.grad, None, None
    with torch.no_grad():
        p_sink = torch.exp(sk.view(1, H, 1) - torch.logsumexp(full, dim=-1))
        bound = (p_sink * (dout * o).sum(-1).abs()).sum((0, 2))
    return o.detach().transpose(1, 2), x.grad, sk.grad, bound


def _run_op(qkv, do, H, Hkv, sinks, causal=True, W=None, cap=None, bounds=None, p=0.0, seed=11):
    """(o, dqkv, dsinks) of the op on ``qkv [B, S, H + 2 Hkv, D]``: attention_packed for Hkv == H (the same bytes
    viewed [B, S, 3, H, D]), attention_gqa_packed otherwise."""
    x = qkv.clone().requires_grad_()
    sk = None if sinks is None else sinks.clone().requires_grad_()
    torch.manual_seed(seed)
    kw = dict(causal=causal, dropout_p=p, training=True, window=W, softcap=cap, doc_bounds=bounds, sinks=sk)
    if Hkv == H:
        Bn, S, _, D = qkv.shape
        o = ops.attention_packed(x.view(Bn, S, 3, H, D), **kw)
    else:
        o = ops.attention_gqa_packed(x, Hkv, **kw)
    o.backward(do)
    torch.cuda.synchronize()
    return o.detach(), x.grad, None if sk is None else sk.grad


def _run_binding(k, qkv, do, H, Hkv, sinks, causal=True, W=0, cap=0.0, p=0.0, seed=11, want_dsinks=True):
    """The two bindings on the head slices of ``qkv``: (o, lse, dqkv, dsinks, (seed, offset))."""
    q, kk, v = qkv[:, :, :H], qkv[:, :, H:H + Hkv], qkv[:, :, H + Hkv:]
    scale = 1.0 / math.sqrt(qkv.shape[-1])
    torch.manual_seed(seed)
    o, lse, sd, off, bits = k.attention_fwd(q, kk, v, causal, p, scale, window=W, softcap=cap, sinks=sinks)
    assert bits.numel() == 0 or sinks is None
    d = torch.empty_like(qkv)
    ds = torch.full((H,), 7.0, device=DEV) if (sinks is not None and want_dsinks) else None
    k.attention_bwd(do, q, kk, v, o, lse, causal, p, scale, sd, off, d[:, :, :H], d[:, :, H:H + Hkv],
                    d[:, :, H + Hkv:], bits if bits.numel() else None, 0, W, cap, None, sinks, ds)
    torch.cuda.synchronize()
    return o, lse, d, ds, (sd, off)


def _parts(o, d, H, Hkv):
    return (("o", o), ("dq", d[:, :, :H]), ("dk", d[:, :, H:H + Hkv]), ("dv", d[:, :, H + Hkv:]))


def _assert_parts_close(o, dqkv, ref_o, ref_d, H, Hkv, dtype, tag):
    atol, rtol = _tol(dtype)
    for (name, out), (_, r) in zip(_parts(o, dqkv, H, Hkv), _parts(ref_o, ref_d, H, Hkv)):
        err = (out.double() - r.double()).abs()
        print(f"{tag} {name}: max|err| {err.max().item():.3e}, "
              f"max excess {(err - atol - rtol * r.double().abs()).max().item():.3e}")
        assert torch.isfinite(out.float()).all(), f"{tag}: {name} not finite"
        assert torch.allclose(out.double(), r.double(), atol=atol, rtol=rtol), f"{tag}: {name}"


def _assert_sinks_bite(ref_o, ref_d, un_o, un_d, H, Hkv, tag):
    """On the references alone: the sinks move at least 25 % of the elements of each of o, dq, dk and dv beyond
    the bound the kernels are then held to."""
    atol, rtol = _tol(torch.bfloat16)
    for (name, r), (_, u) in zip(_parts(ref_o, ref_d, H, Hkv), _parts(un_o, un_d, H, Hkv)):
        moved = ((r - u).abs() > atol + rtol * r.abs()).double().mean().item()
        print(f"{tag} {name}: the sinks move {100 * moved:.1f} % of the elements beyond the bound")
        assert moved >= 0.25, f"{tag}: the sinks move only {100 * moved:.1f} % of {name}"


def _assert_dsinks_loose(ds, ref_ds, bound, tag):
    """``dsinks`` is a cancelling sum: the project's bf16 relative bound on each term's magnitude."""
    err = (ds.double() - ref_ds).abs()
    print(f"{tag} dsinks: {ds.tolist()} ref {ref_ds.tolist()} |err| {err.tolist()} bound {(2e-2 * bound).tolist()}")
    assert torch.isfinite(ds).all() and (err <= 2e-2 * bound).all(), f"{tag}: dsinks"


# ------------------------------------------------------------------ 1. against fp64
#        S,   D,  causal, W
GRID = [(192, 64, True, None), (192, 128, True, None), (192, 256, True, None), (64, 256, True, None),
        (128, 64, True, None), (128, 128, True, None),      # not the S = 128 one-pass kernels
        (256, 64, True, None), (320, 64, True, None),       # not the wide or the long-sequence kernels
        (192, 64, False, None), (128, 128, False, None),
        (192, 64, True, 17), (192, 128, True, 48)]


@pytest.mark.parametrize("H,Hkv", [(4, 4), (6, 2), (4, 1)])
@pytest.mark.parametrize("S,D,causal,W", GRID)
def test_sinks_against_fp64(k, S, D, causal, W, H, Hkv):
    assert k.attention_supported(S, D)
    qkv, do = gqa_inputs(B, S, H, Hkv, D, seed=2)
    sinks = _sinks(H)
    ref_o, ref_d, ref_ds, bound = _reference(qkv, do, H, Hkv, sinks, causal, W)
    un_o, un_d, _, _ = _reference(qkv, do, H, Hkv, None, causal, W)
    tag = f"S{S} D{D} {'causal' if causal else 'full'} W{W} H{H}/{Hkv}"
    _assert_sinks_bite(ref_o, ref_d, un_o, un_d, H, Hkv, tag)
    o, dqkv, ds = _run_op(qkv, do, H, Hkv, sinks, causal, W)
    _assert_parts_close(o, dqkv, ref_o, ref_d, H, Hkv, torch.bfloat16, tag)
    assert ds.dtype == torch.float32 and ds.shape == (H,)
    _assert_dsinks_loose(ds, ref_ds, bound, tag)


def test_sinks_separate_tensors(k):
    """``ops.attention`` on separate ``[B, H, S, D]`` tensors, with sinks in the activations' dtype."""
    S, D, H = 192, 64, 4
    qkv, do = gqa_inputs(B, S, H, H, D, seed=3)
    sinks = _sinks(H).to(torch.bfloat16)
    leaves = [t.transpose(1, 2).contiguous().requires_grad_() for t in qkv.view(B, S, 3, H, D).unbind(2)]
    sk = sinks.clone().requires_grad_()
    o = ops.attention(*leaves, causal=True, sinks=sk)
    o.backward(do.transpose(1, 2))
    ref_o, ref_d, ref_ds, bound = _reference(qkv, do, H, H, sinks)
    dqkv = torch.cat([t.grad.transpose(1, 2) for t in leaves], dim=2)
    _assert_parts_close(o.detach().transpose(1, 2), dqkv, ref_o, ref_d, H, H, torch.bfloat16, "ops.attention")
    assert sk.grad.dtype == torch.bfloat16
    # the fp32 sum rounded once to bf16: 2^-8 relative on top of the loose bound
    assert ((sk.grad.double() - ref_ds).abs() <= 2e-2 * bound + 2.0 ** -8 * ref_ds.abs()).all()


# ------------------------------------------------------------------ 2. dsinks
@pytest.mark.parametrize("H,Hkv", [(4, 4), (6, 2), (4, 1)])
@pytest.mark.parametrize("S,D,causal,W", [(192, 64, True, None), (64, 256, True, None), (320, 64, True, None),
                                          (192, 64, False, None), (192, 128, True, 48)])
def test_dsinks_loose_tight_and_deterministic(k, S, D, causal, W, H, Hkv):
    qkv, do = gqa_inputs(B, S, H, Hkv, D, seed=2)
    sinks = _sinks(H)
    tag = f"S{S} D{D} {'causal' if causal else 'full'} W{W} H{H}/{Hkv}"
    o, lse, _, ds, _ = _run_binding(k, qkv, do, H, Hkv, sinks, causal, W or 0)
    # loose, against fp64
    _, _, ref_ds, bound = _reference(qkv, do, H, Hkv, sinks, causal, W)
    _assert_dsinks_loose(ds, ref_ds, bound, tag)
    # tight, against the kernel's own outputs: the reduction itself, at the fp32 bound on the terms' magnitudes
    delta = (do.double() * o.double()).sum(-1).transpose(1, 2)                    # [B, H, S]
    terms = torch.exp(sinks.double().view(1, H, 1) - lse.double()) * delta
    own = -terms.sum((0, 2))
    err = (ds.double() - own).abs()
    print(f"{tag} dsinks against its own inputs: |err| {err.tolist()} bound {(1e-4 * terms.abs().sum((0, 2))).tolist()}")
    assert (err <= 1e-4 * terms.abs().sum((0, 2))).all(), f"{tag}: the dsinks reduction"
    # the same bits on every run
    _, _, _, ds2, _ = _run_binding(k, qkv, do, H, Hkv, sinks, causal, W or 0)
    assert torch.equal(ds, ds2)
    # accumulating (the fp32 main_grad path) adds exactly the stored value
    q, kk, v = qkv[:, :, :H], qkv[:, :, H:H + Hkv], qkv[:, :, H + Hkv:]
    acc = torch.full((H,), 0.5, device=DEV)
    d = torch.empty_like(qkv)
    k.attention_bwd(do, q, kk, v, o, lse, causal, 0.0, 1.0 / math.sqrt(D), 0, 0, d[:, :, :H], d[:, :, H:H + Hkv],
                    d[:, :, H + Hkv:], None, 0, W or 0, 0.0, None, sinks, acc, True)
    assert torch.equal(acc, 0.5 + ds)


# ------------------------------------------------------------------ 3. exactness
@pytest.mark.parametrize("cap", [0.0, 2.0])
@pytest.mark.parametrize("D", [64, 128])
def test_minus_inf_sinks_are_the_sinkless_bits(k, D, cap):
    """W = 48 at S = 192, so the call without sinks runs the generic kernels too."""
    S, H, Hkv, W = 192, 6, 2, 48
    qkv, do = gqa_inputs(B, S, H, Hkv, D, seed=4)
    none = torch.full((H,), NEG_INF, device=DEV)
    o0, lse0, d0, _, _ = _run_binding(k, qkv, do, H, Hkv, None, True, W, cap)
    o1, lse1, d1, ds, _ = _run_binding(k, qkv, do, H, Hkv, none, True, W, cap)
    assert torch.equal(o0, o1) and torch.equal(lse0, lse1) and torch.equal(d0, d1)
    assert torch.equal(ds, torch.zeros(H, device=DEV))
    # one head without a sink among heads with one: that head's bits alone
    mixed = _sinks(H)
    mixed[1] = NEG_INF
    o2, lse2, d2, ds2, _ = _run_binding(k, qkv, do, H, Hkv, mixed, True, W, cap)
    assert torch.equal(o2[:, :, 1], o0[:, :, 1]) and torch.equal(lse2[:, 1], lse0[:, 1])
    assert torch.equal(d2[:, :, 1], d0[:, :, 1]) and not torch.equal(o2[:, :, 0], o0[:, :, 0])
    assert ds2[1] == 0 and (ds2[[0, 2, 3, 4, 5]] != 0).all()


@pytest.mark.parametrize("causal,W", [(True, None), (False, None), (True, 48)])
def test_large_sinks_stay_finite(k, causal, W):
    S, D, H, Hkv = 192, 64, 4, 2
    qkv, do = gqa_inputs(B, S, H, Hkv, D, seed=5)
    o, lse, d, ds, _ = _run_binding(k, qkv, do, H, Hkv, torch.full((H,), 100.0, device=DEV), causal, W or 0)
    assert torch.isfinite(o.float()).all() and o.float().abs().max().item() < 1e-30
    assert torch.isfinite(lse).all() and (lse - 100.0).abs().max().item() < 1e-3
    assert torch.isfinite(d.float()).all() and torch.isfinite(ds).all()


# ------------------------------------------------------------------ 4. combinations
@pytest.mark.parametrize("H,Hkv", [(4, 4), (6, 2)])
@pytest.mark.parametrize("S,D,causal,W", [(192, 64, True, None), (192, 128, True, 48), (128, 64, False, None)])
def test_sinks_with_a_softcap(k, S, D, causal, W, H, Hkv):
    cap = 2.0
    qkv, do = gqa_inputs(B, S, H, Hkv, D, seed=6)
    sinks = _sinks(H)
    ref_o, ref_d, ref_ds, bound = _reference(qkv, do, H, Hkv, sinks, causal, W, cap)
    un_o, un_d, _, _ = _reference(qkv, do, H, Hkv, None, causal, W, cap)
    tag = f"cap{cap} S{S} D{D} {'causal' if causal else 'full'} W{W} H{H}/{Hkv}"
    _assert_sinks_bite(ref_o, ref_d, un_o, un_d, H, Hkv, tag)
    o, dqkv, ds = _run_op(qkv, do, H, Hkv, sinks, causal, W, cap)
    _assert_parts_close(o, dqkv, ref_o, ref_d, H, Hkv, torch.bfloat16, tag)
    _assert_dsinks_loose(ds, ref_ds, bound, tag)


@pytest.mark.parametrize("H,Hkv", [(4, 4), (6, 2)])
@pytest.mark.parametrize("D,W,cap", [(64, None, None), (128, 48, None), (64, 48, 2.0)])
def test_sinks_with_documents(k, D, W, cap, H, Hkv):
    """Document edges off the 64-row tiles, another packing in each batch row."""
    S = 192
    lengths = [[37, 100, 1, 54], [70, 122]]
    qkv, do = gqa_inputs(B, S, H, Hkv, D, seed=7)
    sinks = _sinks(H)
    ref_o, ref_d, ref_ds, bound = _reference(qkv, do, H, Hkv, sinks, True, W, cap, lengths)
    un_o, un_d, _, _ = _reference(qkv, do, H, Hkv, None, True, W, cap, lengths)
    tag = f"docs D{D} W{W} cap{cap} H{H}/{Hkv}"
    _assert_sinks_bite(ref_o, ref_d, un_o, un_d, H, Hkv, tag)
    o, dqkv, ds = _run_op(qkv, do, H, Hkv, sinks, True, W, cap, _bounds(lengths, S))
    _assert_parts_close(o, dqkv, ref_o, ref_d, H, Hkv, torch.bfloat16, tag)
    _assert_dsinks_loose(ds, ref_ds, bound, tag)


@pytest.mark.parametrize("S,D,W", [(192, 64, None), (192, 128, 48)])
def test_sinks_dropout_exact_mask(k, S, D, W):
    """p = 0.2: dropout acts on the real keys' probabilities, with the sinkless call's Philox mask."""
    H, p = 2, 0.2
    qkv, do = gqa_inputs(B, S, H, H, D, seed=8)
    sinks = _sinks(H)
    o, lse, d, ds, draw = _run_binding(k, qkv, do, H, H, sinks, True, W or 0, p=p)
    keep = _attn_keep_mask(B, H, S, p, *draw)
    assert abs(keep.float().mean().item() - (1 - p)) < 0.02
    ref_o, ref_d, ref_ds, bound = _reference(qkv, do, H, H, sinks, True, W, keep=keep, p=p)
    _assert_parts_close(o, d, ref_o, ref_d, H, H, torch.bfloat16, f"dropout S{S} D{D} W{W}")
    _assert_dsinks_loose(ds, ref_ds, bound, f"dropout S{S} D{D} W{W}")
    # the mask is the sinkless call's: the same draw, and with sinks of -inf the sinkless generic kernels' bits
    # (a window of S - 1 keeps the sinkless call on them; it masks key 0 for the last query only)
    Wg = W or S - 1
    o0, lse0, d0, _, draw0 = _run_binding(k, qkv, do, H, H, None, True, Wg, p=p)
    o1, lse1, d1, _, draw1 = _run_binding(k, qkv, do, H, H, torch.full((H,), NEG_INF, device=DEV), True, Wg, p=p)
    assert draw0 == draw1 == draw
    assert torch.equal(o0, o1) and torch.equal(lse0, lse1) and torch.equal(d0, d1)
    o2, _, _ = _run_op(qkv, do, H, H, sinks, True, W, p=p, seed=12)
    assert not torch.equal(o, o2)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("S,D", [(100, 64), (192, 80), (100, 80)])
def test_sinks_padded_shapes_run_native(k, S, D, causal):
    """Each padding alone and both together.  S = 100: end padding, causal; non-causal the padded keys are masked
    through a spare feature (at D = 64 the head dim goes to 128 to have one), whose -32768 * scale still
    underflows against a running max the sink can only raise.  D = 80: zero features up to 128."""
    A = sys.modules["mipipe.ops.attention"]
    H = 4
    assert not k.attention_supported(S, D)
    key = (S, D, torch.bfloat16, "sinks")
    noted = set(A._noted)
    A._noted.discard(key)  # a note would warn, whatever ran before
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for Hkv in (4, 2):
            qkv, do = gqa_inputs(B, S, H, Hkv, D, seed=9)
            sinks = _sinks(H)
            o, dqkv, ds = _run_op(qkv, do, H, Hkv, sinks, causal)
            ref_o, ref_d, ref_ds, bound = _reference(qkv, do, H, Hkv, sinks, causal)
            tag = f"padded S{S} D{D} {'causal' if causal else 'full'} H{H}/{Hkv}"
            _assert_parts_close(o, dqkv, ref_o, ref_d, H, Hkv, torch.bfloat16, tag)
            _assert_dsinks_loose(ds, ref_ds, bound, tag)
    assert key not in A._noted  # no eager path was noted for this shape
    A._noted |= noted


def test_sinks_checkpoint_recompute_bit_exact(k):
    """S = 256, D = 64 is a long-sequence shape: without sinks the first forward would leave keep words for the
    recompute.  A call with sinks has none and regenerates the same mask from the restored draw."""
    A = sys.modules["mipipe.ops.attention"]
    S, E = 256, 256
    torch.manual_seed(0)
    core = AttentionCore(E, 4, 0.1, norm_first=True, causal=True, layer_norm_eps=1e-5, n_kv_heads=2,
                         attn_sinks=True).to(DEV, torch.bfloat16).train()
    with torch.no_grad():
        core.sinks.copy_(_sinks(4))
    assert core.head_dim == 64 and k.attention_long_supported(S, core.head_dim)
    g = torch.Generator(device=DEV).manual_seed(8)
    base = torch.randn(B, S, E, device=DEV, generator=g).to(torch.bfloat16)
    do = torch.randn(B, S, E, device=DEV, generator=g).to(torch.bfloat16)

    def run(ckpt):
        core.zero_grad()
        x = base.clone().requires_grad_()
        torch.manual_seed(7)
        o = checkpoint(core, x) if ckpt else core(x)
        o.backward(do)
        torch.cuda.synchronize()
        return o.detach(), x.grad, core.in_proj_weight.grad.clone(), core.sinks.grad.clone()

    A.clear_keep_words()
    before = dict(A.keep_stats)
    o1, g1, w1, s1 = run(True)
    assert A.keep_stats == before and not A._keep_words
    o0, g0, w0, s0 = run(False)
    assert torch.equal(o1, o0) and torch.equal(g1, g0) and torch.equal(w1, w0) and torch.equal(s1, s0)
    assert s0.dtype == torch.bfloat16 and (s0 != 0).all()
    core.eval()
    with torch.no_grad():
        assert not torch.equal(core(base), o0)  # the dropout was really there


# ------------------------------------------------------------------ 5. fallbacks and refusals
def test_sinks_fp32_uses_eager_reference_and_warns_once(k):
    A = sys.modules["mipipe.ops.attention"]
    S, D, H, Hkv = 64, 64, 4, 2
    qkv, do = gqa_inputs(B, S, H, Hkv, D, seed=11)
    qkv, do = qkv.float(), do.float()
    sinks = _sinks(H)
    A._noted.discard((S, D, torch.float32, "sinks"))
    with pytest.warns(UserWarning, match="Attention with sinks is native in bf16 only"):
        o, dqkv, ds = _run_op(qkv, do, H, Hkv, sinks)
    ref_o, ref_d, ref_ds, bound = _reference(qkv, do, H, Hkv, sinks)
    _assert_parts_close(o, dqkv, ref_o, ref_d, H, Hkv, torch.float32, "fp32")
    assert ((ds.double() - ref_ds).abs() <= 1e-4 * bound + 1e-4).all()
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # once per shape
        o2, _, _ = _run_op(qkv, do, H, Hkv, sinks)
    assert torch.equal(o2, o)


def test_binding_refuses_bad_sinks(k):
    H = 4
    qkv, _ = gqa_inputs(B, 64, H, H, 64)
    q, kk, v = qkv.view(B, 64, 3, H, 64).unbind(2)
    good = _sinks(H)
    bad = {"bf16": (q.float(), kk.float(), v.float(), good),                        # fp32 q/k/v with sinks
           r"\[H\]": (q, kk, v, _sinks(H + 1)),                                      # wrong length
           "fp32": (q, kk, v, good.to(torch.bfloat16)),                             # not fp32
           "contiguous": (q, kk, v, _sinks(2 * H)[::2]),                            # not contiguous
           "device": (q, kk, v, good.cpu())}                                        # not on the device
    for match, (a, b, c, s) in bad.items():
        with pytest.raises(RuntimeError, match=match):
            k.attention_fwd(a, b, c, True, 0.0, 0.125, sinks=s)
    with pytest.raises(RuntimeError, match=r"\[H\]"):
        k.attention_fwd(q, kk, v, True, 0.0, 0.125, sinks=good.view(1, H))
    o, lse, _, _, _ = k.attention_fwd(q, kk, v, True, 0.0, 0.125, sinks=good)
    dq, dk, dv = torch.empty_like(qkv).view(B, 64, 3, H, 64).unbind(2)  # q's layout
    args = (o, q, kk, v, o, lse, True, 0.0, 0.125, 0, 0, dq, dk, dv)
    for match, s in ((r"\[H\]", _sinks(H + 1)), ("fp32", good.to(torch.bfloat16)), ("device", good.cpu())):
        with pytest.raises(RuntimeError, match=match):
            k.attention_bwd(*args, sinks=s)
    with pytest.raises(RuntimeError, match="dsinks"):
        k.attention_bwd(*args, dsinks=torch.empty(H, device=DEV))                  # dsinks without sinks
    for ds in (torch.empty(H + 1, device=DEV), torch.empty(H, device=DEV, dtype=torch.bfloat16), torch.empty(H)):
        with pytest.raises(RuntimeError, match="dsinks"):
            k.attention_bwd(*args, sinks=good, dsinks=ds)
    k.attention_bwd(*args, sinks=good)  # no dsinks asked for: none written
    torch.cuda.synchronize()


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("S,D", [(128, 64), (256, 64), (192, 128)])
def test_no_sinks_is_todays_path_bit_exact(k, S, D, p):
    """``sinks=None`` through the binding is the call without the argument: the same kernels (the long-sequence
    ones return keep bits, whose words above the diagonal are never written, so only their shape is compared)."""
    H, Hkv = 4, 2
    qkv, do = gqa_inputs(B, S, H, Hkv, D, seed=6)
    q, kk, v = qkv[:, :, :H], qkv[:, :, H:H + Hkv], qkv[:, :, H + Hkv:]
    scale = 1.0 / math.sqrt(D)
    torch.manual_seed(11)
    a = k.attention_fwd(q, kk, v, True, p, scale)
    torch.manual_seed(11)
    b = k.attention_fwd(q, kk, v, True, p, scale, sinks=None)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2:4] == b[2:4] and a[4].shape == b[4].shape
    if S == 256 and p > 0:
        assert a[4].numel() > 0  # the long-sequence kernels, as ever
    grads = []
    for fwd, kw in ((a, {}), (b, {"sinks": None, "dsinks": None})):
        d = torch.empty_like(qkv)
        k.attention_bwd(do, q, kk, v, fwd[0], fwd[1], True, p, scale, fwd[2], fwd[3], d[:, :, :H],
                        d[:, :, H:H + Hkv], d[:, :, H + Hkv:], fwd[4] if fwd[4].numel() else None, 0, **kw)
        grads.append(d)
    assert torch.equal(grads[0], grads[1])


# ------------------------------------------------------------------ 6. the model
def test_sink_tiny_bf16_matches_cpu_fp32(k):
    """sink_tiny's blocks (bf16-rounded weights, the sinks moved off 0) against the fp32 eager model on the CPU:
    one step; ``sinks``' gradient goes straight into the fp32 ``main_grad``, not through ``.grad``."""
    cfg = CONFIGS["sink_tiny"]
    torch.manual_seed(0)
    blocks = build_lm_blocks(cfg, dtype=torch.bfloat16)
    cores = [b.core for b in blocks if isinstance(b, SelfAttentionBlock)]
    assert len(cores) == 2 and all(c.attn_sinks and c.sinks.dtype == torch.bfloat16 and c.window == 48 for c in cores)
    with torch.no_grad():
        for c in cores:
            c.sinks.copy_(torch.linspace(1.0, 4.0, cfg.nhead))
    ref = torch.nn.Sequential(*copy.deepcopy(blocks)).float().train()
    x, t = _data(cfg, 8)
    ref_loss = _loss_fn(cfg)(ref(x), t)
    ref_loss.backward()
    ref_grads = {n: p.grad for n, p in ref.named_parameters()}
    # On the references alone: at initialisation the loss hardly feels the sinks (under 0.1 %), the gradients do.
    # Without sinks every QKV projection's gradient is off by more than ten times the bound the model is held to.
    plain = copy.deepcopy(ref)
    plain.zero_grad()
    with torch.no_grad():
        for b in plain:
            if isinstance(b, SelfAttentionBlock):
                b.core.sinks.fill_(NEG_INF)
    _loss_fn(cfg)(plain(x), t).backward()
    for n, p in plain.named_parameters():
        if n.endswith("core.in_proj_weight"):
            moved = (p.grad - ref_grads[n]).abs().max().item() / ref_grads[n].abs().max().item()
            print(f"{n}: without sinks the gradient is off by {moved:.2f} of its max")
            assert moved > 0.2, n

    model = torch.nn.Sequential(*copy.deepcopy(blocks)).to(DEV).train()
    opt = FlatAdam(model.parameters(), lr=1e-3)
    opt.zero_grad()
    loss = _loss_fn(cfg)(model(x.to(DEV)), t.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    sinks = {n: p for n, p in model.named_parameters() if n.endswith("core.sinks")}
    assert len(sinks) == 2
    for n, p in sinks.items():
        assert p.grad is None and p.main_grad.dtype == torch.float32, n
        assert (p.main_grad != 0).all() and (ref_grads[n] != 0).all(), n
    opt.fold_grads()
    torch.cuda.synchronize()
    grads = {n: p.main_grad.clone() for n, p in model.named_parameters()}
    _assert_model_close(float(loss.detach()), grads, float(ref_loss.detach()), ref_grads)
    opt.step()  # (lr 1e-3 moves the fp32 master, not every bf16 copy of a sink of 1 to 4)
    torch.cuda.synchronize()
    assert all(torch.isfinite(p.detach().float()).all() for p in model.parameters())
