"""Attention with separate QK and V head dims (csrc/kernels/attention_mla.hip) through ``ops.attention``: bf16
q, k 192 wide and v 128 wide against the same math in fp64 / fp32 on the same bf16-rounded values."""
import math
import warnings

import pytest
import torch

from test_gpu_kernels import _attn_keep_mask, _tol

from mipipe import ops

pytestmark = pytest.mark.gpu

DEV, BF = "cuda", torch.bfloat16
B, DQK, DV = 2, 192, 128


@pytest.fixture(scope="module")
def k():
    from mipipe._native_loader import kernels

    return kernels()


def _inputs(S, H, Hkv, views=False, seed=0, dqk=DQK, dv=DV):
    """q, k, v, do as [B, H, S, D].  ``views``: q and v are transposed views of [B, S, H, D] tensors and k a
    slice of a wider last axis, so all three reach the kernels with strides of their own and no copy."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g).to(BF)  # noqa: E731
    if views:
        q, kk, v = rn(B, S, H, dqk).transpose(1, 2), rn(B, Hkv, S, dqk + 64)[..., :dqk], rn(B, S, Hkv, dv).transpose(1, 2)
    else:
        q, kk, v = rn(B, H, S, dqk), rn(B, Hkv, S, dqk), rn(B, Hkv, S, dv)
    return q, kk, v, rn(B, H, S, dv)


def _run(q, kk, v, do, causal, p=0.0, seed=None):
    q, kk, v = (t.detach().requires_grad_() for t in (q, kk, v))
    if seed is not None:
        torch.manual_seed(seed)
    o = ops.attention(q, kk, v, causal, p, True)
    o.backward(do)
    return o.detach(), q.grad, kk.grad, v.grad


def _reference(q, kk, v, do, causal, dtype, keep=None, p=0.0):
    q, kk, v = (t.detach().to(dtype).requires_grad_() for t in (q, kk, v))
    g, S = q.shape[1] // kk.shape[1], q.shape[2]
    s = q @ kk.repeat_interleave(g, 1).transpose(-1, -2) / math.sqrt(q.shape[-1])
    if causal:
        s = s.masked_fill(torch.ones(S, S, dtype=torch.bool, device=DEV).triu(1), float("-inf"))
    pr = torch.softmax(s, -1)
    if keep is not None:
        pr = pr * keep.to(DEV, dtype) / (1 - p)
    o = pr @ v.repeat_interleave(g, 1)
    o.backward(do.to(dtype))
    return o.detach(), q.grad, kk.grad, v.grad


@pytest.mark.parametrize("S,causal,H,Hkv,views", [
    (64, False, 3, 3, False), (64, True, 3, 3, False),      # one tile
    (192, False, 3, 3, False), (192, True, 3, 3, False),    # a skipped tile, a full one, three in each loop
    (192, True, 3, 3, True),                                # independent strides, read in place
    (192, False, 4, 2, False),                              # 4 query heads over 2 K/V heads
    (100, True, 3, 3, False),                               # causal end padding to 128
])
def test_against_fp64(S, causal, H, Hkv, views):
    q, kk, v, do = _inputs(S, H, Hkv, views)
    if views:
        assert not any(t.is_contiguous() for t in (q, kk, v))
    got = _run(q, kk, v, do, causal)
    ref = _reference(q, kk, v, do, causal, torch.float64)
    rtol, atol = _tol(BF)
    for name, a, r in zip(("o", "dq", "dk", "dv"), got, ref):
        assert a.shape == r.shape and a.dtype == BF
        print(f"S{S} causal={causal} {name}: max err {(a.double() - r).abs().max().item():.3e} "
              f"(scale {r.abs().max().item():.3e})")
        torch.testing.assert_close(a.double(), r, rtol=rtol, atol=atol, msg=lambda m, n=name: f"{n}: {m}")


def test_dropout_exact_mask(k):
    """p = 0.25: the mask is the generic kernels' Philox keying (bh, q / 4, key), word q & 3, in all three kernels."""
    S, H, p = 192, 3, 0.25
    q, kk, v, do = _inputs(S, H, H, seed=7)
    torch.manual_seed(11)
    _, _, seed, offset = k.attention_mla_fwd(*(t.transpose(1, 2) for t in (q, kk, v)), True, p, 1 / math.sqrt(DQK))
    keep = _attn_keep_mask(B, H, S, p, seed, offset)
    assert abs(keep.float().mean().item() - (1 - p)) < 0.02
    got = _run(q, kk, v, do, True, p, seed=11)  # the same draw
    ref = _reference(q, kk, v, do, True, torch.float32, keep, p)
    for name, a, r in zip(("o", "dq", "dk", "dv"), got, ref):
        err, scale = (a.float() - r).abs().max().item(), r.abs().max().item()
        print(f"p={p} {name}: err {err:.3e} (scale {scale:.3e})")
        assert err < 3e-2 * (1.0 if name == "o" else max(1.0, scale)), (name, err, scale)
    assert not torch.equal(got[0], _run(q, kk, v, do, True, p, seed=12)[0])


def test_same_seed_same_bits():
    q, kk, v, do = _inputs(192, 3, 3, seed=3)
    a, b = (_run(q, kk, v, do, True, 0.25, seed=5) for _ in range(2))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_dims_supported(k):
    assert k.attention_dims_supported(64, 192, 128)
    assert not any(k.attention_dims_supported(*c) for c in ((96, 192, 128), (64, 192, 64), (64, 128, 128)))


@pytest.mark.parametrize("dqk,dv,window", [(DQK, DV, 32), (96, 64, None)])
def test_fallback_is_reference_with_one_warning(dqk, dv, window):
    q, kk, v, _ = _inputs(64, 3, 3, dqk=dqk, dv=dv)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        outs = [ops.attention(q, kk, v, True, window=window) for _ in range(2)]
    assert len([w for w in rec if "eager math path" in str(w.message)]) == 1
    ref = ops.attention_reference(q, kk, v, True, 0.0, window=window)
    assert all(torch.equal(o, ref) for o in outs)


def test_narrow_k_raises():
    q, kk, v, _ = _inputs(64, 3, 3)
    with pytest.raises(ValueError, match="head dim"):
        ops.attention(q, kk[..., :128], v, True)
