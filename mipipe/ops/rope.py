"""Rotary position embeddings on the packed QKV projection (kernel: csrc/kernels/llama.hip).

Half-split convention: within a head of width ``D`` the pair is ``(i, i + D/2)``
and position ``t`` rotates it by the angle ``t * base^(-2i/D)``::

    q'_i       = q_i cos - q_{i+D/2} sin
    q'_{i+D/2} = q_{i+D/2} cos + q_i sin

Q and K of ``qkv [B, S, 3, H, D]`` are rotated, V passes through.  The tables
are built once on the host in fp64 and stored in fp32 (:func:`rope_tables`);
the kernel does no trigonometry.  A rotation is orthogonal, so the backward is
the inverse rotation (``sin`` negated) of the incoming gradient -- the same
kernel.

The kernel itself takes "rotate the first ``n_rot`` heads of a token, pass the
last ``n_copy`` through" on ``[B, S, n_rot + n_copy, D]``: the layout above is
``(2H, H)``, and a grouped-query projection ``[B, S, H + 2 Hkv, D]`` (Q heads,
then ``Hkv`` K heads, then ``Hkv`` V heads) is ``(H + Hkv, Hkv)``
(:func:`rope_heads`, ``rope_projection(..., n_kv_heads=Hkv)``).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from ._util import kernels_for

__all__ = ["rope_tables", "rope_packed", "rope_heads", "rope_projection", "rope_reference"]


def rope_tables(max_len: int, head_dim: int, base: float = 10000.0, device=None) -> Tuple[Tensor, Tensor]:
    """``(cos, sin)``, each fp32 ``[max_len, head_dim / 2]``: angles ``t * base^(-2i/D)`` computed in fp64."""
    if head_dim % 2 != 0:
        raise ValueError(f"rope_tables: head_dim must be even, got {head_dim}")
    i = torch.arange(head_dim // 2, dtype=torch.float64)
    theta = torch.pow(torch.tensor(float(base), dtype=torch.float64), -2.0 * i / head_dim)
    ang = torch.arange(max_len, dtype=torch.float64).unsqueeze(1) * theta
    return ang.cos().float().to(device), ang.sin().float().to(device)


def rope_reference(qkv: Tensor, cos: Tensor, sin: Tensor, pos0: int = 0, inverse: bool = False) -> Tensor:
    """Eager rotation of Q and K of ``qkv [B, S, 3, H, D]`` (CPU path and test
    oracle); the arithmetic runs in the wider of qkv's and the tables' dtypes."""
    B, S, three, H, D = qkv.shape
    assert three == 3
    half = D // 2
    wide = torch.promote_types(qkv.dtype, cos.dtype)
    c = cos[pos0:pos0 + S].to(wide).view(1, S, 1, 1, half)
    s = sin[pos0:pos0 + S].to(wide).view(1, S, 1, 1, half)
    if inverse:
        s = -s
    qk = qkv[:, :, :2].to(wide)
    a, b = qk[..., :half], qk[..., half:]
    rot = torch.cat((a * c - b * s, b * c + a * s), dim=-1).to(qkv.dtype)
    return torch.cat((rot, qkv[:, :, 2:]), dim=2)


def rope_heads_reference(x: Tensor, cos: Tensor, sin: Tensor, n_rot: int, pos0: int = 0,
                         inverse: bool = False) -> Tensor:
    """Eager rotation of the first ``n_rot`` heads of ``x [B, S, heads, D]`` (CPU path and test oracle);
    the arithmetic runs in the wider of x's and the tables' dtypes."""
    B, S, heads, D = x.shape
    half = D // 2
    wide = torch.promote_types(x.dtype, cos.dtype)
    c = cos[pos0:pos0 + S].to(wide).view(1, S, 1, half)
    s = sin[pos0:pos0 + S].to(wide).view(1, S, 1, half)
    if inverse:
        s = -s
    r = x[:, :, :n_rot].to(wide)
    a, b = r[..., :half], r[..., half:]
    rot = torch.cat((a * c - b * s, b * c + a * s), dim=-1).to(x.dtype)
    return torch.cat((rot, x[:, :, n_rot:]), dim=2)


class _RopeHeads(torch.autograd.Function):
    """:class:`_RopePacked` on ``[B, S, heads, D]`` = shape4 with the first ``n_rot`` heads rotated."""

    @staticmethod
    def forward(ctx, x, cos, sin, pos0, inplace, shape4, n_rot):  # type: ignore[override]
        k = kernels_for(x)
        ctx.save_for_backward(cos, sin)
        ctx.pos0, ctx.shape4, ctx.n_rot = pos0, shape4, n_rot
        x4 = x.view(shape4)
        if inplace:
            ctx.mark_dirty(x)
            k.rope_heads(x4, cos, sin, x4, n_rot, pos0, False)
            return x
        return k.rope_heads(x4, cos, sin, None, n_rot, pos0, False).view(x.shape)

    @staticmethod
    def backward(ctx, dout):  # type: ignore[override]
        cos, sin = ctx.saved_tensors
        d4 = dout.contiguous().view(ctx.shape4)  # out of place: the incoming gradient belongs to autograd
        dx = kernels_for(dout).rope_heads(d4, cos, sin, None, ctx.n_rot, ctx.pos0, True)
        return dx.view(dout.shape), None, None, None, None, None, None


class _RopePacked(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, cos, sin, pos0, inplace, shape5):  # type: ignore[override]
        # qkv: contiguous, [B, S, 3, H, D] = shape5 or any view of it (the
        # projection output [B, S, 3 H D] as it is: an in-place rotation of an
        # autograd VIEW of it would add a copy-slices node to the graph)
        k = kernels_for(qkv)
        ctx.save_for_backward(cos, sin)
        ctx.pos0, ctx.shape5 = pos0, shape5
        q5 = qkv.view(shape5)
        if inplace:
            ctx.mark_dirty(qkv)
            k.rope_packed(q5, cos, sin, q5, pos0, False)
            return qkv
        return k.rope_packed(q5, cos, sin, None, pos0, False).view(qkv.shape)

    @staticmethod
    def backward(ctx, dout):  # type: ignore[override]
        cos, sin = ctx.saved_tensors
        # out of place: the incoming gradient belongs to autograd (it may be
        # shared with another consumer or be the caller's own tensor)
        d5 = dout.contiguous().view(ctx.shape5)
        dqkv = kernels_for(dout).rope_packed(d5, cos, sin, None, ctx.pos0, True)
        return dqkv.view(dout.shape), None, None, None, None, None


def rope_packed(qkv: Tensor, cos: Tensor, sin: Tensor, pos0: int = 0, *, inplace: bool = False) -> Tensor:
    """Rotates Q and K of ``qkv [B, S, 3, H, D]`` for positions ``pos0 .. pos0 + S - 1``.

    Out of place by default: a fresh tensor holds the rotated Q and K and a
    copy of V, and the argument is left as it was -- a public op must not
    change a tensor its caller may still read.  ``inplace=True`` rotates
    ``qkv`` itself (V is not touched: a third less traffic, no allocation) and
    returns it; autograd permits that exactly when no backward needs the
    unrotated values, which it checks itself (the tensor is marked dirty, so a
    saved copy of it raises instead of giving wrong gradients); a leaf that
    requires grad is rotated out of place.  The backward is always out of
    place.  Both variants give the same bits.  CPU tensors take
    :func:`rope_reference` (out of place)."""
    if qkv.dim() != 5 or qkv.shape[2] != 3:
        raise ValueError(f"rope_packed: qkv must be [B, S, 3, H, D], got {tuple(qkv.shape)}")
    if not qkv.is_cuda:
        return rope_reference(qkv, cos, sin, pos0)
    if not qkv.is_contiguous():
        qkv, inplace = qkv.contiguous(), False
    if inplace and qkv.is_leaf and qkv.requires_grad:
        inplace = False  # autograd forbids writing into a leaf that requires grad
    return _RopePacked.apply(qkv, cos, sin, int(pos0), bool(inplace), tuple(qkv.shape))


def rope_heads(x: Tensor, cos: Tensor, sin: Tensor, n_rot: int, pos0: int = 0, *, inplace: bool = False) -> Tensor:
    """Rotates the first ``n_rot`` heads of ``x [B, S, heads, D]`` for positions ``pos0 .. pos0 + S - 1``; the
    other heads pass through.  The in-place / out-of-place rules are :func:`rope_packed`'s."""
    if x.dim() != 4 or not 0 <= n_rot <= x.shape[2]:
        raise ValueError(f"rope_heads: x must be [B, S, heads, D] with 0 <= n_rot <= heads, got {tuple(x.shape)}, "
                         f"n_rot={n_rot}")
    if not x.is_cuda:
        return rope_heads_reference(x, cos, sin, n_rot, pos0)
    if not x.is_contiguous():
        x, inplace = x.contiguous(), False
    if inplace and x.is_leaf and x.requires_grad:
        inplace = False  # autograd forbids writing into a leaf that requires grad
    return _RopeHeads.apply(x, cos, sin, int(pos0), bool(inplace), tuple(x.shape), int(n_rot))


def rope_projection(proj: Tensor, cos: Tensor, sin: Tensor, nhead: int, pos0: int = 0,
                    n_kv_heads: Optional[int] = None) -> Tensor:
    """:func:`rope_packed` for the models: ``proj [B, S, 3 E]`` is the QKV
    projection's own output (fresh, read by nothing else), returned rotated
    and viewed as ``[B, S, 3, H, D]``.

    In place when no graph is being recorded (a checkpointed stage's first
    forward, evaluation): the projection output is then a plain tensor.  Out of
    place under autograd: the output of the linear op's autograd Function is a
    view made inside it, and autograd forbids modifying such a view in place
    (its own view + in-place logic would replace the Function's backward).
    The two give the same bits, so a checkpoint's recompute matches its first
    forward.

    ``n_kv_heads`` (``None`` or ``nhead``: the above) selects the grouped-query
    projection: ``proj [B, S, (H + 2 Hkv) D]``, returned as ``[B, S, H + 2 Hkv,
    D]`` with the ``H`` Q heads and the ``Hkv`` K heads rotated."""
    if n_kv_heads is not None and n_kv_heads != nhead:
        B, S, W = proj.shape
        heads = nhead + 2 * n_kv_heads
        shape4 = (B, S, heads, W // heads)
        n_rot = nhead + n_kv_heads
        if not proj.is_cuda:
            return rope_heads_reference(proj.view(shape4), cos, sin, n_rot, pos0)
        inplace = proj.is_contiguous() and not (torch.is_grad_enabled() and proj.requires_grad)
        return _RopeHeads.apply(proj.contiguous(), cos, sin, int(pos0), inplace, shape4, n_rot).view(shape4)
    B, S, E3 = proj.shape
    shape5 = (B, S, 3, nhead, E3 // (3 * nhead))
    if not proj.is_cuda:
        return rope_reference(proj.view(shape5), cos, sin, pos0)
    inplace = proj.is_contiguous() and not (torch.is_grad_enabled() and proj.requires_grad)
    return _RopePacked.apply(proj.contiguous(), cos, sin, int(pos0), inplace, shape5).view(shape5)
