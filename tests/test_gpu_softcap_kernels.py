"""Logit soft-capping on the GPU: the generic attention kernels with ``s <- c * tanh(s / c)`` before the masks
(non-causal, causal, causal + window; grouped-query heads; dropout; checkpoint recompute), the dispatch that keeps
a capped call off the S = 128, wide and long-sequence kernels, the padded shapes and the eager fallbacks, the
binding's refusals, the stand-alone ``ops.softcap`` kernels, the decoder's final cap and the ``gemma2_tiny``
model.  Everything here but the stated fallbacks runs native code from mipipe/_C.so: the tests fail if the
extension is missing.

Random ``randn`` inputs have scores of about N(0, 1), so a cap of 50 is invisible at the bf16 bound; the kernel
tests use cap 2.0 (and 1.0), where the capped and the uncapped fp64 references differ beyond the bound in at
least a quarter of the elements of each of ``o``, ``dq``, ``dk`` and ``dv`` -- asserted before every comparison, so
a kernel that ignored the cap cannot pass.  S = 192 has three 64-key tiles (a query tile skips one on both sides
of a band); S = 128 and S = 256 / 320 at D = 64 are the shapes an uncapped call sends to other kernels."""
import copy
import dataclasses
import math
import sys
import warnings

import pytest
import torch

from helpers.gqa_cases import gqa_inputs
from helpers.rowwise_cases import assert_close
from test_gpu_kernels import _attn_keep_mask, _tol
from test_gpu_llama_kernels import _assert_model_close, _data, _gpu_step, _loss_fn

from mipipe import Pipe, checkpoint, ops
from mipipe.models import CONFIGS, build_lm_blocks
from mipipe.models.lm import Decoder
from mipipe.models.transformer import AttentionCore
from mipipe.optim import FlatAdam
from mipipe.parallel import PipelineEngine

pytestmark = pytest.mark.gpu

DEV = "cuda"
B = 2


@pytest.fixture(scope="module")
def k():
    from mipipe._native_loader import kernels

    return kernels()


def _reference(qkv, do, H, Hkv, cap, causal=True, W=None, keep=None, p=0.0, dtype=torch.float64):
    """Attention on ``qkv [B, S, H + 2 Hkv, D]`` with repeated K/V heads, every step in ``dtype``: the scaled
    scores capped with ``torch.tanh`` (``cap=None``: not), then masked from ``arange``, not the op's own code.
    (o [B, S, H, D], dqkv); autograd sums each group.  ``keep [B, H, S, S]``: a dropout mask."""
    x = qkv.to(dtype).requires_grad_()
    q, kk, v = (t.transpose(1, 2) for t in (x[:, :, :H], x[:, :, H:H + Hkv], x[:, :, H + Hkv:]))
    g = H // Hkv
    kk, v = kk.repeat_interleave(g, 1), v.repeat_interleave(g, 1)
    S = q.shape[-2]
    s = torch.matmul(q, kk.transpose(-1, -2)) / math.sqrt(q.shape[-1])
    if cap is not None:
        s = cap * torch.tanh(s / cap)
    i = torch.arange(S, device=s.device)[:, None]
    j = torch.arange(S, device=s.device)[None, :]
    if causal:
        s = s.masked_fill(j > i, float("-inf"))
    if W is not None:
        s = s.masked_fill(j <= i - W, float("-inf"))
    pr = torch.softmax(s, dim=-1)
    if keep is not None:
        pr = pr * keep.to(pr.device).to(dtype) / (1 - p)
    o = torch.matmul(pr, v)
    o.backward(do.to(dtype).transpose(1, 2))
    return o.detach().transpose(1, 2), x.grad


def _run_op(qkv, do, H, Hkv, cap, causal=True, W=None, p=0.0, seed=11):
    """(o, dqkv) of the capped op on ``qkv [B, S, H + 2 Hkv, D]``: attention_packed for Hkv == H (the same bytes
    viewed [B, S, 3, H, D]), attention_gqa_packed otherwise."""
    x = qkv.clone().requires_grad_()
    torch.manual_seed(seed)
    if Hkv == H:
        Bn, S, _, D = qkv.shape
        o = ops.attention_packed(x.view(Bn, S, 3, H, D), causal=causal, dropout_p=p, training=True, window=W,
                                 softcap=cap)
    else:
        o = ops.attention_gqa_packed(x, Hkv, causal=causal, dropout_p=p, training=True, window=W, softcap=cap)
    o.backward(do)
    torch.cuda.synchronize()
    return o.detach(), x.grad


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


def _assert_cap_bites(ref_o, ref_d, un_o, un_d, H, Hkv, tag):
    """On the references alone: the cap moves at least 25 % of the elements of each of o, dq, dk and dv beyond
    the bound the kernels are then held to."""
    atol, rtol = _tol(torch.bfloat16)
    for (name, r), (_, u) in zip(_parts(ref_o, ref_d, H, Hkv), _parts(un_o, un_d, H, Hkv)):
        moved = ((r - u).abs() > atol + rtol * r.abs()).double().mean().item()
        print(f"{tag} {name}: the cap moves {100 * moved:.1f} % of the elements beyond the bound")
        assert moved >= 0.25, f"{tag}: the cap moves only {100 * moved:.1f} % of {name}"


# ------------------------------------------------------------------ 1. against fp64
#        S,   D,  causal, W
GRID = [(192, 64, True, None), (192, 128, True, None), (192, 256, True, None), (64, 256, True, None),
        (128, 64, True, None), (128, 128, True, None),      # not the S = 128 one-pass kernels
        (256, 64, True, None), (320, 64, True, None),       # not the wide or the long-sequence kernels
        (192, 64, False, None), (128, 128, False, None),
        (192, 64, True, 65), (192, 64, True, 17), (192, 128, True, 48)]


@pytest.mark.parametrize("H,Hkv", [(4, 4), (6, 2), (4, 1)])
@pytest.mark.parametrize("S,D,causal,W", GRID)
def test_softcap_against_fp64(k, S, D, causal, W, H, Hkv):
    cap = 2.0
    assert k.attention_supported(S, D)
    qkv, do = gqa_inputs(B, S, H, Hkv, D, seed=2)
    ref_o, ref_d = _reference(qkv, do, H, Hkv, cap, causal, W)
    un_o, un_d = _reference(qkv, do, H, Hkv, None, causal, W)
    tag = f"S{S} D{D} {'causal' if causal else 'full'} W{W} H{H}/{Hkv} cap{cap}"
    _assert_cap_bites(ref_o, ref_d, un_o, un_d, H, Hkv, tag)
    o, dqkv = _run_op(qkv, do, H, Hkv, cap, causal, W)
    _assert_parts_close(o, dqkv, ref_o, ref_d, H, Hkv, torch.bfloat16, tag)


@pytest.mark.parametrize("H,Hkv", [(4, 4), (6, 2), (4, 1)])
def test_softcap_of_one_against_fp64(k, H, Hkv):
    S, D, cap = 192, 64, 1.0
    qkv, do = gqa_inputs(B, S, H, Hkv, D, seed=2)
    ref_o, ref_d = _reference(qkv, do, H, Hkv, cap)
    un_o, un_d = _reference(qkv, do, H, Hkv, None)
    _assert_cap_bites(ref_o, ref_d, un_o, un_d, H, Hkv, f"cap{cap} H{H}/{Hkv}")
    o, dqkv = _run_op(qkv, do, H, Hkv, cap)
    _assert_parts_close(o, dqkv, ref_o, ref_d, H, Hkv, torch.bfloat16, f"cap{cap} H{H}/{Hkv}")


@pytest.mark.parametrize("H,Hkv", [(4, 4), (6, 2), (4, 1)])
def test_large_softcap_loses_nothing(k, H, Hkv):
    """cap 50 on N(0, 1) scores: the capped fp64 reference is the uncapped one at the bound, and the capped
    kernels (the generic ones, not the wide ones an uncapped call runs here) meet it."""
    S, D, cap = 192, 64, 50.0
    atol, rtol = _tol(torch.bfloat16)
    qkv, do = gqa_inputs(B, S, H, Hkv, D, seed=2)
    ref_o, ref_d = _reference(qkv, do, H, Hkv, cap)
    un_o, un_d = _reference(qkv, do, H, Hkv, None)
    assert torch.allclose(ref_o, un_o, atol=atol, rtol=rtol) and torch.allclose(ref_d, un_d, atol=atol, rtol=rtol)
    o, dqkv = _run_op(qkv, do, H, Hkv, cap)
    _assert_parts_close(o, dqkv, ref_o, ref_d, H, Hkv, torch.bfloat16, f"cap{cap} H{H}/{Hkv}")


def test_softcap_separate_tensors(k):
    """``ops.attention`` on separate ``[B, H, S, D]`` tensors."""
    S, D, H, cap = 192, 64, 4, 2.0
    qkv, do = gqa_inputs(B, S, H, H, D, seed=3)
    leaves = [t.transpose(1, 2).contiguous().requires_grad_() for t in qkv.view(B, S, 3, H, D).unbind(2)]
    o = ops.attention(*leaves, causal=True, softcap=cap)
    o.backward(do.transpose(1, 2))
    ref_o, ref_d = _reference(qkv, do, H, H, cap)
    dqkv = torch.cat([t.grad.transpose(1, 2) for t in leaves], dim=2)
    _assert_parts_close(o.detach().transpose(1, 2), dqkv, ref_o, ref_d, H, H, torch.bfloat16, "ops.attention")


# ------------------------------------------------------------------ 2. dropout
@pytest.mark.parametrize("S,D,W", [(192, 64, None), (192, 128, 48)])
def test_softcap_dropout_exact_mask(k, S, D, W):
    """p = 0.2: a capped call returns no keep words and its mask is the uncapped generic kernels' Philox mask."""
    H, p, cap = 2, 0.2, 2.0
    qkv, do = gqa_inputs(B, S, H, H, D, seed=7)
    q, kk, v = qkv.view(B, S, 3, H, D).unbind(2)
    scale = 1.0 / math.sqrt(D)
    torch.manual_seed(11)
    _, _, seed, offset, bits = k.attention_fwd(q, kk, v, True, p, scale, window=W or 0, softcap=cap)
    assert bits.numel() == 0
    keep = _attn_keep_mask(B, H, S, p, seed, offset)
    assert abs(keep.float().mean().item() - (1 - p)) < 0.02
    o, dqkv = _run_op(qkv, do, H, H, cap, True, W, p=p, seed=11)  # the same draw
    ref_o, ref_d = _reference(qkv, do, H, H, cap, True, W, keep=keep, p=p)
    _assert_parts_close(o, dqkv, ref_o, ref_d, H, H, torch.bfloat16, f"dropout S{S} D{D} W{W}")
    o2, _ = _run_op(qkv, do, H, H, cap, True, W, p=p, seed=12)
    assert not torch.equal(o, o2)


# ------------------------------------------------------------------ 3. checkpoint recompute
def test_softcap_checkpoint_recompute_bit_exact(k):
    """S = 256, D = 64 is a long-sequence shape: uncapped, the first forward would leave keep words for the
    recompute.  A capped call has none and regenerates the same mask from the restored draw."""
    A = sys.modules["mipipe.ops.attention"]
    S, E = 256, 256
    torch.manual_seed(0)
    core = AttentionCore(E, 4, 0.1, norm_first=True, causal=True, layer_norm_eps=1e-5, n_kv_heads=2,
                         attn_softcap=2.0).to(DEV, torch.bfloat16).train()
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
        return o.detach(), x.grad, core.in_proj_weight.grad.clone()

    A.clear_keep_words()
    before = dict(A.keep_stats)
    o1, g1, w1 = run(True)
    assert A.keep_stats == before and not A._keep_words
    o0, g0, w0 = run(False)
    assert torch.equal(o1, o0) and torch.equal(g1, g0) and torch.equal(w1, w0)
    core.eval()
    with torch.no_grad():
        assert not torch.equal(core(base), o0)  # the dropout was really there


# ------------------------------------------------------------------ 4. padded shapes and fallbacks
def test_softcap_causal_padded_shape_runs_native(k):
    """Causal S = 100, D = 80: end padding and zero features (which add 0 to the raw score, before the cap)."""
    A = sys.modules["mipipe.ops.attention"]
    S, D, H, cap = 100, 80, 4, 2.0
    assert not k.attention_supported(S, D)
    noted = set(A._noted)
    A._noted.discard((S, D, torch.bfloat16, "softcap"))  # a note would warn, whatever ran before
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for Hkv in (4, 2):
            qkv, do = gqa_inputs(B, S, H, Hkv, D, seed=9)
            o, dqkv = _run_op(qkv, do, H, Hkv, cap)
            ref_o, ref_d = _reference(qkv, do, H, Hkv, cap)
            _assert_parts_close(o, dqkv, ref_o, ref_d, H, Hkv, torch.bfloat16, f"padded S{S} D{D} H{H}/{Hkv}")
    assert (S, D, torch.bfloat16, "softcap") not in A._noted  # no eager path was noted for this shape
    A._noted |= noted


def test_softcap_noncausal_padded_shape_uses_eager_reference_and_warns_once(k):
    """The spare-feature key mask does not survive the cap: this shape is not native."""
    A = sys.modules["mipipe.ops.attention"]
    S, D, H, cap = 100, 80, 4, 2.0
    qkv, do = gqa_inputs(B, S, H, H, D, seed=10)
    A._noted.discard((S, D, torch.bfloat16, "softcap"))
    with pytest.warns(UserWarning, match="Soft-capped attention is native in bf16 only"):
        o, dqkv = _run_op(qkv, do, H, H, cap, causal=False)
    x = qkv.clone().requires_grad_()
    q, kk, v = (t.transpose(1, 2) for t in x.view(B, S, 3, H, D).unbind(2))
    ref = ops.attention_reference(q, kk, v, False, 0.0, softcap=cap).transpose(1, 2)
    ref.backward(do)
    assert torch.equal(o, ref.detach()) and torch.equal(dqkv, x.grad)
    ref_o, ref_d = _reference(qkv, do, H, H, cap, causal=False)
    _assert_parts_close(o, dqkv, ref_o, ref_d, H, H, torch.bfloat16, "eager non-causal")
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # once per shape
        o2, _ = _run_op(qkv, do, H, H, cap, causal=False)
    assert torch.equal(o2, o)


def test_softcap_fp32_uses_eager_reference_and_warns_once(k):
    A = sys.modules["mipipe.ops.attention"]
    S, D, H, Hkv, cap = 64, 64, 4, 2, 2.0
    qkv, do = gqa_inputs(B, S, H, Hkv, D, seed=11)
    qkv, do = qkv.float(), do.float()
    A._noted.discard((S, D, torch.float32, "softcap"))
    with pytest.warns(UserWarning, match="Soft-capped attention is native in bf16 only"):
        o, dqkv = _run_op(qkv, do, H, Hkv, cap)
    ref_o, ref_d = _reference(qkv, do, H, Hkv, cap)
    _assert_parts_close(o, dqkv, ref_o, ref_d, H, Hkv, torch.float32, "fp32")
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # once per shape
        o2, _ = _run_op(qkv, do, H, Hkv, cap)
    assert torch.equal(o2, o)


# ------------------------------------------------------------------ 5. the binding
def test_binding_refuses_bad_softcaps(k):
    qkv, _ = gqa_inputs(B, 64, 4, 4, 64)
    q, kk, v = qkv.view(B, 64, 3, 4, 64).unbind(2)
    with pytest.raises(RuntimeError, match="softcap"):
        k.attention_fwd(q, kk, v, True, 0.0, 0.125, softcap=-1.0)
    with pytest.raises(RuntimeError, match="softcap"):
        k.attention_fwd(q, kk, v, True, 0.0, 0.125, softcap=float("nan"))
    with pytest.raises(RuntimeError, match="softcap"):
        k.attention_fwd(q, kk, v, True, 0.0, 0.125, softcap=float("inf"))
    with pytest.raises(RuntimeError, match="bf16"):
        k.attention_fwd(q.float(), kk.float(), v.float(), True, 0.0, 0.125, softcap=2.0)
    o, lse, _, _, _ = k.attention_fwd(q, kk, v, True, 0.0, 0.125)
    dq, dk, dv = (torch.empty_like(t) for t in (q, kk, v))
    with pytest.raises(RuntimeError, match="softcap"):
        k.attention_bwd(o, q, kk, v, o, lse, True, 0.0, 0.125, 0, 0, dq, dk, dv, softcap=-2.0)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("S,D", [(128, 64), (256, 64), (192, 128)])
def test_zero_softcap_is_todays_path_bit_exact(k, S, D, p):
    """``softcap=0.0`` through the binding is the call without the argument: the same kernels (the long-sequence
    ones return keep bits, whose words above the diagonal are never written, so only their shape is compared)."""
    H, Hkv = 4, 2
    qkv, do = gqa_inputs(B, S, H, Hkv, D, seed=6)
    q, kk, v = qkv[:, :, :H], qkv[:, :, H:H + Hkv], qkv[:, :, H + Hkv:]
    scale = 1.0 / math.sqrt(D)
    torch.manual_seed(11)
    a = k.attention_fwd(q, kk, v, True, p, scale)
    torch.manual_seed(11)
    b = k.attention_fwd(q, kk, v, True, p, scale, softcap=0.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2:4] == b[2:4] and a[4].shape == b[4].shape
    grads = []
    for fwd, kw in ((a, {}), (b, {"softcap": 0.0})):
        d = torch.empty_like(qkv)
        k.attention_bwd(do, q, kk, v, fwd[0], fwd[1], True, p, scale, fwd[2], fwd[3], d[:, :, :H],
                        d[:, :, H:H + Hkv], d[:, :, H + Hkv:], fwd[4] if fwd[4].numel() else None, 0, **kw)
        grads.append(d)
    assert torch.equal(grads[0], grads[1])


# ------------------------------------------------------------------ 6. ops.softcap
def _softcap_input(shape, dtype, seed):
    """std 3, so the tanh bites: ([37, 1000] is the [:, :1000] view of a [37, 1024] buffer: padded rows, a tail)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    if shape == (37, 1000):
        full = (3.0 * torch.randn(37, 1024, device=DEV, generator=g)).to(dtype)
        dfull = torch.randn(37, 1024, device=DEV, generator=g).to(dtype)
        return full[:, :1000], dfull[:, :1000]
    return (3.0 * torch.randn(*shape, device=DEV, generator=g)).to(dtype), \
        torch.randn(*shape, device=DEV, generator=g).to(dtype)


@pytest.mark.parametrize("cap", [1.0, 30.0])
@pytest.mark.parametrize("shape", [(37, 1000), (8191,), (3, 5, 256)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_ops_softcap_against_fp64(k, dtype, shape, cap):
    """Forward against ``cap * tanh(x / cap)`` in fp64.  The backward is defined on the saved output, ``dx = dy *
    (1 - (y / cap)^2)``: it is compared against that formula in fp64 on the stored ``y`` (whose own rounding the
    forward comparison bounds), and in fp32, where ``y`` carries no visible rounding, against the derivative
    ``dy * (1 - tanh(x / cap)^2)`` taken from ``x`` as well."""
    x, dy = _softcap_input(shape, dtype, seed=3 + len(shape))
    if shape == (37, 1000):
        assert not x.is_contiguous() and x.stride(0) == 1024
    leaf = x.detach().requires_grad_()
    y = ops.softcap(leaf, cap)
    y.backward(dy)
    torch.cuda.synchronize()
    assert y.shape == x.shape and leaf.grad.shape == x.shape and y.dtype == dtype
    ref = cap * torch.tanh(x.double() / cap)
    assert_close(y.detach(), ref, dtype, f"softcap {shape} {dtype} cap {cap}")
    assert (y.detach().abs() <= cap).all()
    ref_dx = dy.double() * (1 - (y.detach().double() / cap) ** 2)
    assert_close(leaf.grad, ref_dx, dtype, f"softcap backward {shape} {dtype} cap {cap}")
    if dtype == torch.float32:
        assert_close(leaf.grad, dy.double() * (1 - torch.tanh(x.double() / cap) ** 2), dtype,
                     f"softcap derivative {shape} cap {cap}")


def test_ops_softcap_in_place_and_pad_columns(k):
    """In place (also under autograd) the result is the out-of-place one bit for bit; an in-place call on a view
    of a padded buffer leaves the pad columns alone."""
    x, dy = _softcap_input((37, 1000), torch.bfloat16, seed=5)
    y0 = ops.softcap(x, 2.0)
    buf = torch.full((37, 1024), 7.0, device=DEV, dtype=torch.bfloat16)
    buf[:, :1000] = x
    ops.softcap(buf[:, :1000], 2.0, inplace=True)
    assert torch.equal(buf[:, :1000], y0) and (buf[:, 1000:] == 7.0).all()
    leaf = x.detach().clone().requires_grad_()
    y1 = ops.softcap(leaf * 1.0, 2.0, inplace=True)
    y1.backward(dy)
    leaf0 = x.detach().clone().requires_grad_()
    ops.softcap(leaf0, 2.0).backward(dy)
    assert torch.equal(y1.detach(), y0) and torch.equal(leaf.grad, leaf0.grad)


# ------------------------------------------------------------------ 7. the decoder's final cap
def test_decoder_final_softcap_keeps_pad_columns_zero(k, monkeypatch):
    V, E, cap = 1000, 256, 1.0
    torch.manual_seed(0)
    dec = Decoder(V, E, final_softcap=cap, dtype=torch.bfloat16)
    assert dec.padded == 1024
    ref = copy.deepcopy(dec).float()
    gen = torch.Generator().manual_seed(1)
    x = (4.0 * torch.randn(2, 48, E, generator=gen)).to(torch.bfloat16)  # logits of std ~ 3.7: the cap bites
    t = torch.randint(0, V, (2, 48), generator=gen)
    loss_fn = lambda y, tt: ops.cross_entropy(y.reshape(-1, V), tt.reshape(-1))  # noqa: E731
    xr = x.float().requires_grad_()
    ref_loss = loss_fn(ref(xr), t)
    ref_loss.backward()
    uncapped = copy.deepcopy(ref)
    uncapped.final_softcap = None
    ref_loss = ref_loss.detach()
    with torch.no_grad():
        assert abs(float(loss_fn(uncapped(x.float()), t)) - float(ref_loss)) > 2e-3 * abs(float(ref_loss))

    dec = dec.to(DEV).train()
    seen = {}
    L = sys.modules["mipipe.ops.linear"]
    real_bwd = L._Linear.backward

    def spy(ctx, dy, dres=None):
        seen["dy"] = dy.detach().clone()
        return real_bwd(ctx, dy, dres)

    monkeypatch.setattr(L._Linear, "backward", staticmethod(spy))
    xg = x.to(DEV).requires_grad_()
    y = dec(xg)
    assert y.shape[-1] == V and y.stride(-2) == dec.padded and y.storage_offset() == 0
    padded = torch.as_strided(y.detach(), (2, 48, dec.padded), (48 * dec.padded, dec.padded, 1))
    assert torch.equal(padded[..., V:], torch.zeros_like(padded[..., V:]))  # tanh(0) = 0 exactly
    assert (padded.abs() <= cap).all()
    logits = ops.linear(xg.detach(), dec.weight.detach(), dec.bias.detach())
    assert y.data_ptr() != logits.data_ptr() and torch.equal(padded, ops.softcap(logits, cap))  # the cap, once
    loss = loss_fn(y, t.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    assert seen["dy"].shape[-1] == dec.padded
    assert torch.equal(seen["dy"][..., V:], torch.zeros_like(seen["dy"][..., V:]))
    assert seen["dy"][..., :V].abs().max() > 0
    assert abs(float(loss) - float(ref_loss)) < 2e-3 * abs(float(ref_loss)), (float(loss), float(ref_loss))
    for name, g, r in (("weight", dec.weight.grad, ref.weight.grad), ("bias", dec.bias.grad, ref.bias.grad),
                       ("x", xg.grad, xr.grad)):
        err = (g.float().cpu() - r).abs().max().item()
        print(f"decoder {name}: max|err| {err:.3e} of max|ref| {r.abs().max().item():.3e}")
        assert err <= 2e-2 * (r.abs().max().item() + 1e-6), name


# ------------------------------------------------------------------ 8. the model
def _gemma_cfgs():
    cfg = CONFIGS["gemma2_tiny"]
    return {"config": cfg, "biting": dataclasses.replace(cfg, attn_softcap=0.5, final_softcap=1.0)}


@pytest.fixture(scope="module", params=["config", "biting"])
def gemma_reference(request):
    """gemma2_tiny's blocks (bf16-rounded weights) and, on the CPU in fp32 -- eager capped attention, eager capped
    logits --, the loss and gradients of one step: with the config's caps (50 / 30), and with caps of 0.5 / 1.0,
    which bite at initialisation (scores of std ~ 0.7, logits ~ 0.9): there the CPU reference's loss first has to
    differ from the uncapped model's by more than the comparison's tolerance."""
    cfg = _gemma_cfgs()[request.param]
    torch.manual_seed(0)
    blocks = build_lm_blocks(cfg, dtype=torch.bfloat16)
    assert all(b.core.attn_softcap == cfg.attn_softcap and b.core.window == 48 for b in blocks if hasattr(b, "core"))
    assert blocks[-1].final_softcap == cfg.final_softcap
    ref = torch.nn.Sequential(*copy.deepcopy(blocks)).float().train()
    x, t = _data(cfg, 8)
    loss = _loss_fn(cfg)(ref(x), t)
    loss.backward()
    if request.param == "biting":
        plain = copy.deepcopy(ref)
        for b in plain:
            if hasattr(b, "core"):
                b.core.attn_softcap = None
        plain[-1].final_softcap = None
        with torch.no_grad():
            plain_loss = float(_loss_fn(cfg)(plain(x), t))
        print(f"capped loss {float(loss.detach()):.5f}, uncapped {plain_loss:.5f}")
        assert abs(plain_loss - float(loss.detach())) > 2e-3 * abs(float(loss.detach()))
    return cfg, blocks, float(loss.detach()), {n: p.grad for n, p in ref.named_parameters()}


def test_gemma2_tiny_pipe_step(k, gemma_reference):
    cfg, blocks, ref_loss, ref_grads = gemma_reference
    model = torch.nn.Sequential(*copy.deepcopy(blocks)).to(DEV).train()
    x, t = _data(cfg, 8)
    loss, grads = _gpu_step(model, cfg, x, t)
    _assert_model_close(loss, grads, ref_loss, ref_grads)
    model = torch.nn.Sequential(*copy.deepcopy(blocks)).to(DEV).train()
    opt = FlatAdam(model.parameters(), lr=1e-3)
    pipe = Pipe(model, chunks=4, checkpoint="except_last", balance=[3, len(blocks) - 3], copy_same_device=True)
    try:
        assert len(pipe.partitions) == 2
        opt.zero_grad()
        loss = _loss_fn(cfg)(pipe(x.to(DEV)).local_value(), t.to(DEV))
        loss.backward()
        opt.fold_grads()
        torch.cuda.synchronize()
    finally:
        pipe.close()
    _assert_model_close(float(loss.detach()), {n: p.main_grad for n, p in model.named_parameters()}, ref_loss,
                        ref_grads)


def test_gemma2_tiny_engine_step_flat_adam(k, gemma_reference):
    cfg, blocks, ref_loss, ref_grads = gemma_reference
    model = torch.nn.Sequential(*copy.deepcopy(blocks)).to(DEV).train()
    opt = FlatAdam(model.parameters(), lr=1e-3)
    m, mb = 4, 2
    eng = PipelineEngine(model, chunks=m, checkpoint="except_last", act_shape=(mb, cfg.seq_len),
                         act_dtype=torch.bfloat16, loss_fn=_loss_fn(cfg), device=torch.device(DEV, 0))
    x, t = _data(cfg, m * mb)
    before = [p.detach().clone() for p in model.parameters()]
    opt.zero_grad()
    st = eng.step([c.to(DEV) for c in x.split(mb)], [c.to(DEV) for c in t.split(mb)])
    opt.fold_grads()
    torch.cuda.synchronize()
    _assert_model_close(float(st.loss), {n: p.main_grad.clone() for n, p in model.named_parameters()}, ref_loss,
                        ref_grads)
    opt.step()
    torch.cuda.synchronize()
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
    assert all(torch.isfinite(p.detach().float()).all() for p in model.parameters())
