"""Document-masked attention on the GPU (packed sequences): the generic attention
kernels with per-row bounds (``doc_bounds [B, 2, S]``: query i sees the keys
``start[i] <= j <= i``), their tile skipping on both sides, the window merged at
run time, the dispatch that keeps a call with bounds off the S = 128, wide and
long-sequence kernels, dropout, checkpoint recompute, the padded shapes, the
fp32 fallback, the binding's argument checks and ``mistral_tiny`` on a packed
batch.  Everything here but the fp32 fallback runs native code from
mipipe/_C.so: the tests fail if the extension is missing.

Shapes are the smallest that reach each path: S = 192 has three 64-key tiles, so
a query tile can skip a tile before its first document and a key tile the query
tiles after its last one; the packings put boundaries on a tile edge (64), one
past it (65), mid tile (130, 100, 17) and hold one-token documents, whose rows
find every earlier visited tile wholly masked.  The oracle's mask comes from
document ids built from the lengths (``id[i] == id[j]`` and ``j <= i``), not
from the bounds tensor or the op's own mask code."""
import copy
import math
import sys
import warnings

import pytest
import torch

from helpers.gqa_cases import gqa_inputs
from test_gpu_kernels import _attn_keep_mask, _tol
from test_gpu_llama_kernels import _assert_model_close, _data, _gpu_step, _loss_fn

from mipipe import checkpoint, ops
from mipipe.models import CONFIGS, build_lm_blocks
from mipipe.models.transformer import AttentionCore
from mipipe.optim import FlatAdam
from mipipe.parallel import PipelineEngine
from mipipe.utils.data import document_bounds, document_bounds_from_lengths

pytestmark = pytest.mark.gpu

DEV = "cuda"
B = 2


@pytest.fixture(scope="module")
def k():
    from mipipe._native_loader import kernels

    return kernels()


def _rows(lengths):
    """One packing per batch row: a flat list is used for both rows."""
    return [lengths] * B if isinstance(lengths[0], int) else lengths


def _keep(lengths, S, W, device):
    """keep[b, i, j] from document ids: same document, j <= i, and j > i - W under a window."""
    ids = torch.stack([torch.repeat_interleave(torch.arange(len(r)), torch.tensor(r)) for r in _rows(lengths)]).to(device)
    assert ids.shape == (B, S)
    i = torch.arange(S, device=device)[:, None]
    j = torch.arange(S, device=device)[None, :]
    keep = (ids[:, :, None] == ids[:, None, :]) & (j <= i)
    if W is not None:
        keep &= j > i - W
    return keep


def _doc_reference(qkv, do, H, Hkv, lengths, W=None, softcap=None, dtype=torch.float64, keep=None, p=0.0):
    """Document-masked attention on ``qkv [B, S, H + 2 Hkv, D]`` with repeated K/V heads, every step in
    ``dtype``: (o [B, S, H, D], dqkv); autograd sums each group.  ``keep [B, H, S, S]``: a dropout mask."""
    x = qkv.to(dtype).requires_grad_()
    q, kk, v = (t.transpose(1, 2) for t in (x[:, :, :H], x[:, :, H:H + Hkv], x[:, :, H + Hkv:]))
    g = H // Hkv
    kk, v = kk.repeat_interleave(g, 1), v.repeat_interleave(g, 1)
    S = q.shape[-2]
    s = torch.matmul(q, kk.transpose(-1, -2)) / math.sqrt(q.shape[-1])
    if softcap is not None:
        s = softcap * torch.tanh(s / softcap)
    s = s.masked_fill(~_keep(lengths, S, W, s.device)[:, None], float("-inf"))
    pr = torch.softmax(s, dim=-1)
    if keep is not None:
        pr = pr * keep.to(pr.device).to(dtype) / (1 - p)
    o = torch.matmul(pr, v)
    o.backward(do.to(dtype).transpose(1, 2))
    return o.detach().transpose(1, 2), x.grad


def _bounds(lengths, S):
    b = document_bounds_from_lengths(_rows(lengths), S, device=DEV)
    assert b.shape == (B, 2, S) and b.dtype == torch.int32
    return b


def _run_op(qkv, do, H, Hkv, bounds, W=None, softcap=None, p=0.0, seed=11):
    """(o, dqkv) of the op with ``doc_bounds`` on ``qkv [B, S, H + 2 Hkv, D]``: attention_packed for Hkv == H
    (the same bytes viewed [B, S, 3, H, D]), attention_gqa_packed otherwise."""
    x = qkv.clone().requires_grad_()
    torch.manual_seed(seed)
    kw = dict(causal=True, dropout_p=p, training=True, window=W, softcap=softcap, doc_bounds=bounds)
    if Hkv == H:
        Bn, S, _, D = qkv.shape
        o = ops.attention_packed(x.view(Bn, S, 3, H, D), **kw)
    else:
        o = ops.attention_gqa_packed(x, Hkv, **kw)
    o.backward(do)
    torch.cuda.synchronize()
    return o.detach(), x.grad


def _assert_parts_close(o, dqkv, ref_o, ref_d, H, Hkv, dtype, tag):
    atol, rtol = _tol(dtype)
    for name, out, r in (("o", o, ref_o), ("dq", dqkv[:, :, :H], ref_d[:, :, :H]),
                         ("dk", dqkv[:, :, H:H + Hkv], ref_d[:, :, H:H + Hkv]),
                         ("dv", dqkv[:, :, H + Hkv:], ref_d[:, :, H + Hkv:])):
        err = (out.double() - r.double()).abs()
        print(f"{tag} {name}: max|err| {err.max().item():.3e}, "
              f"max excess {(err - atol - rtol * r.double().abs()).max().item():.3e}")
        assert torch.isfinite(out.float()).all(), f"{tag}: {name} not finite"
        assert torch.allclose(out.double(), r.double(), atol=atol, rtol=rtol), f"{tag}: {name}"


# ------------------------------------------------------------------ 1. against fp64
HEADS = [(4, 4), (6, 2), (4, 1)]
# a packing for every S: uneven, off the tile edges, another one per batch row
PACK = {64: [[1, 20, 43], [64]],
        128: [[1, 63, 1, 63], [50, 78]],        # not the S = 128 one-pass kernels
        192: [[100, 92], [17, 175]],
        256: [[70, 58, 128], [1, 255]],         # not the long-sequence kernels
        320: [[128, 70, 122], [33, 287]]}
SD = [(192, 64), (192, 128), (64, 256), (192, 256), (128, 64), (128, 128), (256, 64), (320, 64)]
# S = 192: one-token documents and boundaries at 64, 65 and 130; tile-aligned; one document; per-row bounds
PACK192 = [[1, 63, 1, 65, 62], [64, 128], [192], [[100, 92], [17, 175]]]


@pytest.mark.parametrize("H,Hkv", HEADS)
@pytest.mark.parametrize("S,D", SD)
def test_documents_against_fp64(k, S, D, H, Hkv):
    assert k.attention_supported(S, D)
    qkv, do = gqa_inputs(B, S, H, Hkv, D, seed=2)
    o, dqkv = _run_op(qkv, do, H, Hkv, _bounds(PACK[S], S))
    ref_o, ref_d = _doc_reference(qkv, do, H, Hkv, PACK[S])
    _assert_parts_close(o, dqkv, ref_o, ref_d, H, Hkv, torch.bfloat16, f"S{S} D{D} H{H}/{Hkv}")


@pytest.mark.parametrize("H,Hkv", HEADS)
@pytest.mark.parametrize("W,softcap", [(None, None), (17, None), (64, None), (None, 50.0), (64, 50.0)])
@pytest.mark.parametrize("pack", range(len(PACK192)))
def test_documents_packings_windows_softcap(k, pack, W, softcap, H, Hkv):
    S, D = 192, 64
    lengths = PACK192[pack]
    qkv, do = gqa_inputs(B, S, H, Hkv, D, seed=3)
    o, dqkv = _run_op(qkv, do, H, Hkv, _bounds(lengths, S), W=W, softcap=softcap)
    ref_o, ref_d = _doc_reference(qkv, do, H, Hkv, lengths, W=W, softcap=softcap)
    _assert_parts_close(o, dqkv, ref_o, ref_d, H, Hkv, torch.bfloat16, f"{lengths} W{W} cap{softcap} H{H}/{Hkv}")


def test_one_document_equals_the_generic_causal_kernels(k):
    """One document per row is the causal mask: the same numbers as the generic causal kernels give (S = 192, D =
    128 is a shape a plain causal call runs on them too), bit for bit in the forward."""
    S, D, H, Hkv = 192, 128, 4, 2
    qkv, do = gqa_inputs(B, S, H, Hkv, D, seed=4)
    o, dqkv = _run_op(qkv, do, H, Hkv, _bounds([S], S))
    x = qkv.clone().requires_grad_()
    o0 = ops.attention_gqa_packed(x, Hkv, causal=True)
    o0.backward(do)
    assert torch.equal(o, o0.detach())
    ref_o, ref_d = _doc_reference(qkv, do, H, Hkv, [S])
    _assert_parts_close(o, dqkv, ref_o, ref_d, H, Hkv, torch.bfloat16, "one document")


def test_documents_separate_tensors(k):
    """``ops.attention`` on separate ``[B, H, S, D]`` tensors."""
    S, D, H = 192, 64, 4
    lengths = PACK192[0]
    qkv, do = gqa_inputs(B, S, H, H, D, seed=5)
    leaves = [t.transpose(1, 2).contiguous().requires_grad_() for t in qkv.view(B, S, 3, H, D).unbind(2)]
    o = ops.attention(*leaves, causal=True, doc_bounds=_bounds(lengths, S))
    o.backward(do.transpose(1, 2))
    ref_o, ref_d = _doc_reference(qkv, do, H, H, lengths)
    dqkv = torch.cat([t.grad.transpose(1, 2) for t in leaves], dim=2)
    _assert_parts_close(o.detach().transpose(1, 2), dqkv, ref_o, ref_d, H, H, torch.bfloat16, "ops.attention")


# ------------------------------------------------------------------ 2. one-token documents
@pytest.mark.parametrize("H,Hkv", HEADS)
def test_one_token_documents_give_v_and_zero_dq_dk_exactly(k, H, Hkv):
    """Every document one token: a query sees itself only, p = 1 exactly and o is v bit for bit; dS = P (dP -
    delta) is 0 in exact arithmetic and dq == dk == 0 bit for bit on the kernels, because the backward takes
    delta from attn_delta_mfma_kernel -- the argument test_window_of_one_gives_zero_dq_dk_exactly makes."""
    S, D = 192, 64
    qkv, do = gqa_inputs(B, S, H, Hkv, D, seed=2)
    o, dqkv = _run_op(qkv, do, H, Hkv, _bounds([1] * S, S))
    assert torch.equal(o, qkv[:, :, H + Hkv:].repeat_interleave(H // Hkv, 2))
    print(f"one-token documents H{H}/{Hkv}: max|dq| {dqkv[:, :, :H].abs().max().item():.3e}, "
          f"max|dk| {dqkv[:, :, H:H + Hkv].abs().max().item():.3e}")
    assert torch.equal(dqkv[:, :, :H + Hkv], torch.zeros_like(dqkv[:, :, :H + Hkv]))


# ------------------------------------------------------------------ 3. locality, bit for bit
@pytest.mark.parametrize("D", [64, 128])
def test_document_locality_bit_exact(k, D):
    """Keys of another document and queries of another document do not reach a token at all: both loop bounds
    and both masks, to the row.  The overwritten rows keep randn scale (this tests skipping, not overflow)."""
    S, H, Hkv = 320, 4, 2
    lengths = [128, 70, 122]  # boundaries at 128 (a tile edge) and 198 (mid tile)
    bounds = _bounds(lengths, S)
    qkv, do = gqa_inputs(B, S, H, Hkv, D, seed=4)
    other, other_do = gqa_inputs(B, S, H, Hkv, D, seed=5)
    assert torch.isfinite(other.float()).all() and torch.isfinite(other_do.float()).all()
    o0, d0 = _run_op(qkv, do, H, Hkv, bounds)

    kv = qkv.clone()
    kv[:, :128, H:] = other[:, :128, H:]          # K and V rows [0, 128): the first document's
    o1, d1 = _run_op(kv, do, H, Hkv, bounds)
    assert torch.equal(o1[:, 128:], o0[:, 128:])
    assert torch.equal(d1[:, 128:, :H], d0[:, 128:, :H])
    assert not torch.equal(o1[:, 127], o0[:, 127])            # the row before the boundary does see them
    assert not torch.equal(d1[:, 127, :H], d0[:, 127, :H])

    qd = qkv.clone()
    qd[:, 198:, :H] = other[:, 198:, :H]          # Q and dO rows [198, 320): the last document's
    do2 = do.clone()
    do2[:, 198:] = other_do[:, 198:]
    o2, d2 = _run_op(qd, do2, H, Hkv, bounds)
    assert torch.equal(d2[:, :198, H:], d0[:, :198, H:])
    assert not torch.equal(d2[:, 198, H:H + Hkv], d0[:, 198, H:H + Hkv])  # key 198 is seen by those queries
    assert not torch.equal(d2[:, 198, H + Hkv:], d0[:, 198, H + Hkv:])


# ------------------------------------------------------------------ 4. dropout
@pytest.mark.parametrize("S,D", [(192, 64), (320, 64)])
def test_document_dropout_exact_mask(k, S, D):
    """p = 0.1: the mask is the generic kernels' Philox keying (bh, q / 4, key) at every S -- also where a call
    without bounds uses the long-sequence kernels' stored bits -- restricted to the visible keys."""
    H, p = 2, 0.1
    lengths = PACK192[0] if S == 192 else PACK[S]
    bounds = _bounds(lengths, S)
    qkv, do = gqa_inputs(B, S, H, H, D, seed=7)
    q, kk, v = qkv.view(B, S, 3, H, D).unbind(2)
    scale = 1.0 / math.sqrt(D)
    torch.manual_seed(11)
    _, _, seed, offset, bits = k.attention_fwd(q, kk, v, True, p, scale, doc_bounds=bounds)
    assert bits.numel() == 0
    keep = _attn_keep_mask(B, H, S, p, seed, offset)
    assert abs(keep.float().mean().item() - (1 - p)) < 0.02
    o, dqkv = _run_op(qkv, do, H, H, bounds, p=p, seed=11)  # the same draw
    ref_o, ref_d = _doc_reference(qkv, do, H, H, lengths, dtype=torch.float32, keep=keep, p=p)
    err = (o.float() - ref_o).abs().max().item()
    gerr = (dqkv.float() - ref_d).abs().max().item()
    gscale = ref_d.abs().max().item()
    print(f"S{S} p={p}: o err {err:.3e}, grad err {gerr:.3e} (scale {gscale:.3e})")
    assert err < 3e-2, err
    assert gerr < 3e-2 * max(1.0, gscale), (gerr, gscale)
    o2, _ = _run_op(qkv, do, H, H, bounds, p=p, seed=12)
    assert not torch.equal(o, o2)


# ------------------------------------------------------------------ 5. checkpoint recompute
def test_document_checkpoint_recompute_bit_exact(k):
    """S = 256, D = 64 is a long-sequence shape: without bounds the first forward would leave keep words for the
    recompute.  A call with bounds has none and regenerates the same mask from the restored draw; the recompute
    runs inside the same ``use_documents`` block."""
    A = sys.modules["mipipe.ops.attention"]
    S, E = 256, 256
    torch.manual_seed(0)
    core = AttentionCore(E, 4, 0.1, norm_first=True, causal=True, layer_norm_eps=1e-5,
                         n_kv_heads=2).to(DEV, torch.bfloat16).train()
    assert core.head_dim == 64 and k.attention_long_supported(S, core.head_dim)
    g = torch.Generator(device=DEV).manual_seed(8)
    base = torch.randn(B, S, E, device=DEV, generator=g).to(torch.bfloat16)
    do = torch.randn(B, S, E, device=DEV, generator=g).to(torch.bfloat16)
    bounds = _bounds(PACK[S], S)

    def run(ckpt, b=bounds):
        core.zero_grad()
        x = base.clone().requires_grad_()
        torch.manual_seed(7)
        with ops.use_documents(b):
            o = checkpoint(core, x) if ckpt else core(x)
            o.backward(do)
        torch.cuda.synchronize()
        return o.detach(), x.grad, core.in_proj_weight.grad.clone()

    A.clear_keep_words()
    before = dict(A.keep_stats)
    o1, g1, w1 = run(True)
    assert A.keep_stats == before and not A._keep_words
    o0, g0, w0 = run(False)
    assert torch.equal(o1, o0) and torch.equal(g1, g0) and torch.equal(w1, w0)
    assert not torch.equal(run(False, None)[0], o0)  # the bounds were really there
    core.eval()
    with torch.no_grad(), ops.use_documents(bounds):
        assert not torch.equal(core(base), o0)  # and so was the dropout


# ------------------------------------------------------------------ 6. padded shapes
@pytest.mark.parametrize("S,D,lengths", [(100, 64, [[30, 37, 33], [1, 99]]), (192, 80, [[100, 92], [17, 175]])])
def test_document_padded_shapes_run_native(k, S, D, lengths):
    """A causal length padded at the end (the pad tokens become one trailing document) and a head dim padded
    with zero features stay on the kernels."""
    A = sys.modules["mipipe.ops.attention"]
    H = 4
    assert not k.attention_supported(S, D)
    bounds = _bounds(lengths, S)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for Hkv in (4, 2):
            qkv, do = gqa_inputs(B, S, H, Hkv, D, seed=9)
            o, dqkv = _run_op(qkv, do, H, Hkv, bounds)
            ref_o, ref_d = _doc_reference(qkv, do, H, Hkv, lengths)
            _assert_parts_close(o, dqkv, ref_o, ref_d, H, Hkv, torch.bfloat16, f"padded S{S} D{D} H{H}/{Hkv}")
        qkv, do = gqa_inputs(B, S, H, H, D, seed=10)
        leaves = [t.transpose(1, 2).contiguous().requires_grad_() for t in qkv.view(B, S, 3, H, D).unbind(2)]
        o = ops.attention(*leaves, causal=True, doc_bounds=bounds)
        o.backward(do.transpose(1, 2))
    ref_o, ref_d = _doc_reference(qkv, do, H, H, lengths)
    dqkv = torch.cat([t.grad.transpose(1, 2) for t in leaves], dim=2)
    _assert_parts_close(o.detach().transpose(1, 2), dqkv, ref_o, ref_d, H, H, torch.bfloat16, f"padded attention S{S}")
    assert not [key for key in A._noted if key[:2] == (S, D)]  # no eager path was noted for this shape


# ------------------------------------------------------------------ 7. fp32 is not native
def test_document_fp32_uses_eager_reference_and_warns_once(k):
    A = sys.modules["mipipe.ops.attention"]
    S, D, H, Hkv = 64, 64, 4, 2
    lengths = PACK[S]
    bounds = _bounds(lengths, S)
    qkv, do = gqa_inputs(B, S, H, Hkv, D, seed=11)
    qkv, do = qkv.float(), do.float()
    A._noted.discard((S, D, torch.float32, "documents"))
    with pytest.warns(UserWarning, match="Document-masked attention is native in bf16 only"):
        o, dqkv = _run_op(qkv, do, H, Hkv, bounds)
    ref_o, ref_d = _doc_reference(qkv, do, H, Hkv, lengths)
    _assert_parts_close(o, dqkv, ref_o, ref_d, H, Hkv, torch.float32, "fp32")
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # once per shape
        o2, _ = _run_op(qkv, do, H, Hkv, bounds)
    assert torch.equal(o2, o)


# ------------------------------------------------------------------ 8. the binding's argument checks
def test_binding_refuses_bad_bounds(k):
    """Host-side argument errors: nothing is launched."""
    S = 64
    qkv, _ = gqa_inputs(B, S, 4, 4, 64)
    q, kk, v = qkv.view(B, S, 3, 4, 64).unbind(2)
    good = _bounds([S], S)
    with pytest.raises(RuntimeError, match="int32"):
        k.attention_fwd(q, kk, v, True, 0.0, 0.125, doc_bounds=good.long())
    with pytest.raises(RuntimeError, match=r"\[B, 2, S\]"):
        k.attention_fwd(q, kk, v, True, 0.0, 0.125, doc_bounds=good[:, :, :32].contiguous())
    with pytest.raises(RuntimeError, match=r"\[B, 2, S\]"):
        k.attention_fwd(q, kk, v, True, 0.0, 0.125, doc_bounds=good[:, 0])
    with pytest.raises(RuntimeError, match="contiguous"):
        k.attention_fwd(q, kk, v, True, 0.0, 0.125, doc_bounds=good.transpose(0, 1).contiguous().transpose(0, 1))
    with pytest.raises(RuntimeError, match="causal"):
        k.attention_fwd(q, kk, v, False, 0.0, 0.125, doc_bounds=good)
    with pytest.raises(RuntimeError, match="device"):
        k.attention_fwd(q, kk, v, True, 0.0, 0.125, doc_bounds=good.cpu())
    with pytest.raises(RuntimeError, match="bf16"):
        k.attention_fwd(q.float(), kk.float(), v.float(), True, 0.0, 0.125, doc_bounds=good)


# ------------------------------------------------------------------ 9. the model
def _packed_batch(cfg, n):
    """``_data``'s batch, its most frequent token id taken as EOS, and the bounds."""
    x, t = _data(cfg, n)
    eos = int(torch.bincount(x.reshape(-1), minlength=cfg.vocab).argmax())
    bounds = document_bounds(x, eos)
    ops.check_doc_bounds(bounds)
    # at least one row holds two or more documents: a plain causal path cannot pass
    assert int((bounds[:, 0].max(dim=1).values > 0).sum()) >= 1
    return x, t, bounds


@pytest.fixture(scope="module")
def mistral_documents_reference():
    """mistral_tiny's blocks (bf16-rounded weights) and, on the CPU in fp32 under ``use_documents`` -- where the
    attention is the eager fp32 reference with the document mask --, the loss and gradients of one step."""
    cfg = CONFIGS["mistral_tiny"]
    torch.manual_seed(0)
    blocks = build_lm_blocks(cfg, dtype=torch.bfloat16)
    ref = torch.nn.Sequential(*copy.deepcopy(blocks)).float().train()
    x, t, bounds = _packed_batch(cfg, 8)
    with ops.use_documents(bounds):
        loss = _loss_fn(cfg)(ref(x), t)
    loss.backward()
    with torch.no_grad():
        plain = _loss_fn(cfg)(ref(x), t)
    assert float(plain) != float(loss.detach())  # the mask changes the model's output
    return blocks, float(loss.detach()), {n: p.grad for n, p in ref.named_parameters()}


def test_mistral_tiny_documents_unpipelined(k, mistral_documents_reference):
    cfg = CONFIGS["mistral_tiny"]
    blocks, ref_loss, ref_grads = mistral_documents_reference
    model = torch.nn.Sequential(*copy.deepcopy(blocks)).to(DEV).train()
    x, t, bounds = _packed_batch(cfg, 8)
    with ops.use_documents(bounds.to(DEV)):
        loss, grads = _gpu_step(model, cfg, x, t)
    _assert_model_close(loss, grads, ref_loss, ref_grads)


def test_mistral_tiny_documents_engine_step_flat_adam(k, mistral_documents_reference):
    cfg = CONFIGS["mistral_tiny"]
    blocks, ref_loss, ref_grads = mistral_documents_reference
    model = torch.nn.Sequential(*copy.deepcopy(blocks)).to(DEV).train()
    opt = FlatAdam(model.parameters(), lr=1e-3)
    m, mb = 4, 2
    eng = PipelineEngine(model, chunks=m, checkpoint="except_last", act_shape=(mb, cfg.seq_len),
                         act_dtype=torch.bfloat16, loss_fn=_loss_fn(cfg), device=torch.device(DEV, 0))
    x, t, bounds = _packed_batch(cfg, m * mb)
    opt.zero_grad()
    st = eng.step([c.to(DEV) for c in x.split(mb)], [c.to(DEV) for c in t.split(mb)],
                  doc_bounds=[c.to(DEV).contiguous() for c in bounds.split(mb)])
    opt.fold_grads()
    torch.cuda.synchronize()
    _assert_model_close(float(st.loss), {n: p.main_grad.clone() for n, p in model.named_parameters()}, ref_loss,
                        ref_grads)
    assert ops.current_documents() is None  # the step leaves no context behind
