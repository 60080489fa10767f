"""``ops.mla_rope`` (llama.hip's mla_rope kernel): the decoupled RoPE of multi-head latent attention against the
eager reference in fp64."""
import pytest
import torch

from test_gpu_kernels import _tol

from mipipe import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(2, 5, 3, 128, 64, 64), (1, 64, 1, 128, 64, 512), (1, 7, 2, 16, 32, 8)]  # B, S, H, Dn, R, Lkv


def _inputs(B, S, H, Dn, R, Lkv, dtype):
    g = torch.Generator(device=DEV).manual_seed(0)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g).to(dtype)  # noqa: E731
    cos, sin = ops.rope_tables(S + 3, R, 10000.0, device=DEV)
    return rn(B, S, H, Dn + R), rn(B, S, Lkv + R), cos, sin, rn(B, S, H, Dn + R), rn(B, S, R)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shape", SHAPES)
def test_against_fp64(shape, dtype):
    q, ckv, cos, sin, gq, gk = _inputs(*shape, dtype)
    outs = []
    for fn, wide in ((ops.mla_rope, dtype), (ops.mla_rope_reference, torch.float64)):
        qq, cc = (t.detach().to(wide).requires_grad_() for t in (q, ckv))
        qo, kr = fn(qq, cc, cos, sin)
        torch.autograd.backward((qo, kr), (gq.to(wide), gk.to(wide)))
        outs.append((qo.detach(), kr.detach(), qq.grad, cc.grad))
    rtol, atol = _tol(dtype)
    for name, a, r in zip(("q", "k_rope", "dq", "dckv"), *outs):
        assert a.shape == r.shape and a.dtype == dtype and a.is_contiguous()
        torch.testing.assert_close(a.double(), r, rtol=rtol, atol=atol, msg=lambda m, n=name: f"{n}: {m}")
    Dn = shape[3]
    assert torch.equal(outs[0][0][..., :Dn], q[..., :Dn])  # the nope columns are the input's bits


@pytest.mark.parametrize("shape", SHAPES)
def test_in_place_gives_the_same_bits(shape):
    q, ckv, cos, sin, _, _ = _inputs(*shape, torch.bfloat16)
    q0 = q.clone()
    qo, kr = ops.mla_rope(q0.clone().requires_grad_(), ckv, cos, sin)  # under autograd: a new tensor
    with torch.no_grad():
        qi, ki = ops.mla_rope(q, ckv, cos, sin)
    assert qi.data_ptr() == q.data_ptr() and not torch.equal(q, q0)
    assert torch.equal(qi, qo) and torch.equal(ki, kr)
