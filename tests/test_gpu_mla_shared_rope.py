"""``ops.attention(q, k_nope, v, k_rope=...)``: the shared rope key head read in place by attention_mla.hip's SHARED
kernels, against fp64 math on the concatenated K and, bit for bit, against the plain kernels on the same K."""
import warnings

import pytest
import torch

from test_gpu_kernels import _tol

from mipipe import ops

pytestmark = pytest.mark.gpu

DEV, BF = "cuda", torch.bfloat16
B, DN, R, DV = 2, 128, 64, 128
NAMES = ("o", "dq", "dk_nope", "dk_rope", "dv")


def _inputs(S, H, views=False, seed=0, dtype=BF):
    """q [B, H, S, 192], k_nope, v [B, H, S, 128], k_rope [B, S, 64], do.  ``views``: k_nope and v are the halves of
    one [B, S, H, 256] tensor and q a slice of a wider one, all read in place."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g).to(dtype)  # noqa: E731
    if views:
        kv = rn(B, S, H, DN + DV).transpose(1, 2)
        q, kn, v = rn(B, S, H, DN + R + 64)[..., :DN + R].transpose(1, 2), kv[..., :DN], kv[..., DN:]
    else:
        q, kn, v = rn(B, H, S, DN + R), rn(B, H, S, DN), rn(B, H, S, DV)
    return q, kn, v, rn(B, S, R), rn(B, H, S, DV)


def _shared(q, kn, v, kr, do, causal, p=0.0, seed=None):
    q, kn, v, kr = (t.detach().requires_grad_() for t in (q, kn, v, kr))
    if seed is not None:
        torch.manual_seed(seed)
    o = ops.attention(q, kn, v, causal, p, True, k_rope=kr)
    o.backward(do)
    return o.detach(), q.grad, kn.grad, kr.grad, v.grad


def _fp64(q, kn, v, kr, do, causal):
    """The reference on a K built by hand; autograd sums dk_rope over the heads."""
    q, kn, v, kr = (t.detach().double().requires_grad_() for t in (q, kn, v, kr))
    kk = torch.cat([kn, kr[:, None].expand(-1, kn.shape[1], -1, -1)], -1)
    o = ops.attention_reference(q, kk, v, causal, 0.0)
    o.backward(do.double())
    return o.detach(), q.grad, kn.grad, kr.grad, v.grad


def _concat(q, kn, v, kr, do, causal, p=0.0, seed=None):
    """Today's call on the hand-concatenated K; dk split back into (nope, rope summed over the heads by autograd)."""
    q, kn, v, kr = (t.detach().requires_grad_() for t in (q, kn, v, kr))
    kk = torch.cat([kn, kr[:, None].expand(-1, kn.shape[1], -1, -1)], -1).detach().requires_grad_()
    if seed is not None:
        torch.manual_seed(seed)
    o = ops.attention(q, kk, v, causal, p, True)
    o.backward(do)
    return o.detach(), q.grad, kk.grad[..., :DN], kk.grad[..., DN:], v.grad


@pytest.mark.parametrize("S,causal,H,views", [
    (64, True, 1, False),    # one tile, one head
    (128, True, 3, True),    # the diagonal and an off-diagonal tile, an odd head count, operands read in place
    (192, False, 2, False),  # non-causal
    (100, True, 2, False),   # causal end padding to 128
])
def test_against_fp64(S, causal, H, views):
    q, kn, v, kr, do = _inputs(S, H, views)
    if views:
        assert not any(t.is_contiguous() for t in (q, kn, v))
    got = _shared(q, kn, v, kr, do, causal)
    ref = _fp64(q, kn, v, kr, do, causal)
    rtol, atol = _tol(BF)
    for name, a, r in zip(NAMES, got, ref):
        assert a.shape == r.shape and a.dtype == BF
        print(f"S{S} causal={causal} H{H} {name}: max err {(a.double() - r).abs().max().item():.3e} "
              f"(scale {r.abs().max().item():.3e})")
        torch.testing.assert_close(a.double(), r, rtol=rtol, atol=atol, msg=lambda m, n=name: f"{n}: {m}")


@pytest.mark.parametrize("p", [0.0, 0.25])
def test_bits_of_the_concatenated_call(p):
    """Same data, same arithmetic: o, dq, dk_nope and dv are the plain kernels' bits, also under dropout (one seed:
    the mask keying did not move)."""
    q, kn, v, kr, do = _inputs(128, 3, seed=1)
    got = _shared(q, kn, v, kr, do, True, p, seed=5)
    ref = _concat(q, kn, v, kr, do, True, p, seed=5)
    for name, a, r in zip(NAMES, got, ref):
        if name != "dk_rope":
            assert torch.equal(a, r), name


def test_dk_rope_same_bits_every_run():
    q, kn, v, kr, do = _inputs(128, 3, seed=2)
    a, b = (_shared(q, kn, v, kr, do, True)[3] for _ in range(2))
    assert torch.equal(a, b)


def test_one_head_dk_rope_is_the_concatenated_bits():
    """A sum of one partial rounds once."""
    q, kn, v, kr, do = _inputs(128, 1, seed=3)
    assert torch.equal(_shared(q, kn, v, kr, do, True)[3], _concat(q, kn, v, kr, do, True)[3][:, 0])


@pytest.mark.parametrize("dtype,window", [(torch.float32, None), (BF, 32)])
def test_fallback_is_reference_with_one_warning(dtype, window):
    q, kn, v, kr, _ = _inputs(64, 3, dtype=dtype)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        outs = [ops.attention(q, kn, v, True, window=window, k_rope=kr) for _ in range(2)]
    assert len([w for w in rec if "eager math path" in str(w.message)]) == 1
    ref = ops.attention_reference(q, kn, v, True, 0.0, window=window, k_rope=kr)
    assert all(torch.equal(o, ref) for o in outs)


def test_wrong_width_raises():
    q, kn, v, kr, _ = _inputs(64, 3)
    with pytest.raises(ValueError, match="k_rope"):
        ops.attention(q, kn, v, True, k_rope=kr[..., :32])
