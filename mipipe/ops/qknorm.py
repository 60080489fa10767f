"""QK-norm: per-head RMSNorm on Q and K fused with RoPE (kernel: csrc/kernels/qknorm.hip).

Qwen3, OLMo-2 and Gemma-3 normalise every query head and every key head over
its ``D`` features, with a learned ``[D]`` weight per kind, after the QKV
projection and before the rotary rotation::

    n  = x * rsqrt(mean(x^2) + eps) * w        w = wq for Q heads, wk for K heads
    y  = rotate(n)                             (:mod:`mipipe.ops.rope`'s half-split pairs and tables)

The layout is :func:`~mipipe.ops.rope.rope_heads`': ``x [B, S, heads, D]`` with
the first ``n_q`` heads Q, the next ``n_k`` K and the rest (V) passed through;
``[B, S, 3, H, D]`` is the case ``(H, H)`` byte for byte and the grouped-query
projection ``[B, S, H + 2 Hkv, D]`` the case ``(H, Hkv)``.  ``cos = sin = None``
drops the rotation (the norm alone).  One kernel reads and writes every element
once, in fp32 with a single rounding at the store; the backward needs the
un-normalised ``x`` and the rows' ``rstd``, so those are what autograd saves.

GPU tensors go to the HIP kernels (a missing extension raises) for head dims
16, 32, 64, 128 and 256; another head dim takes the eager reference and says so
once per shape.  CPU tensors use the reference.
"""
from __future__ import annotations

import warnings
from typing import Optional

import torch
from torch import Tensor

from ._util import kernels_for
from .linear import accumulable

__all__ = ["qk_norm_rope_heads", "qk_norm_rope_projection", "qk_norm_rope_reference"]

_noted = set()


def qk_norm_rope_reference(x: Tensor, wq: Tensor, wk: Tensor, eps: float, cos: Optional[Tensor],
                           sin: Optional[Tensor], n_q: int, n_k: int, pos0: int = 0) -> Tensor:
    """Eager QK-norm + rotation of ``x [B, S, heads, D]`` (CPU path and test oracle): the arithmetic runs in the
    wider of x's and the tables' dtypes and in fp32 at least, like ``rms_norm_reference``."""
    B, S, heads, D = x.shape
    half = D // 2
    wide = torch.promote_types(x.dtype, torch.float32)
    if cos is not None:
        wide = torch.promote_types(wide, cos.dtype)
    qk = x[:, :, :n_q + n_k].to(wide)
    w = torch.cat((wq.to(wide).view(1, D).expand(n_q, D), wk.to(wide).view(1, D).expand(n_k, D)), dim=0)
    n = qk * torch.rsqrt(qk.pow(2).mean(-1, keepdim=True) + eps) * w
    if cos is not None:
        c = cos[pos0:pos0 + S].to(wide).view(1, S, 1, half)
        s = sin[pos0:pos0 + S].to(wide).view(1, S, 1, half)
        a, b = n[..., :half], n[..., half:]
        n = torch.cat((a * c - b * s, b * c + a * s), dim=-1)
    return torch.cat((n.to(x.dtype), x[:, :, n_q + n_k:]), dim=2)


class _QkNormRope(torch.autograd.Function):
    """``x``: contiguous, ``[B, S, heads, D]`` = shape4 or any view of it (the projection's own output)."""

    @staticmethod
    def forward(ctx, x, wq, wk, eps, cos, sin, pos0, inplace, shape4, n_q, n_k, save):  # type: ignore[override]
        ctx.set_materialize_grads(False)
        k = kernels_for(x)
        x4 = x.view(shape4)
        ctx.pos0, ctx.shape4, ctx.n_q, ctx.n_k, ctx.has_tables = pos0, shape4, n_q, n_k, cos is not None
        if inplace:
            # only where no graph is recorded: the backward needs the un-normalised x
            ctx.mark_dirty(x)
            k.qk_norm_rope_fwd(x4, wq, wk, eps, cos, sin, x4, n_q, n_k, pos0, False)
            return x
        y, rstd = k.qk_norm_rope_fwd(x4, wq, wk, eps, cos, sin, None, n_q, n_k, pos0, save)
        if save:
            ctx.save_for_backward(x, rstd, wq, wk, *((cos, sin) if cos is not None else ()))
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dout):  # type: ignore[override]
        if dout is None:
            return (None,) * 12
        x, rstd, wq, wk = ctx.saved_tensors[:4]
        cos, sin = ctx.saved_tensors[4:] if ctx.has_tables else (None, None)
        # the weight gradients accumulate straight into the fp32 main_grad buffers where there are any
        mq = accumulable(wq) if ctx.needs_input_grad[1] else None
        mk = accumulable(wk) if ctx.needs_input_grad[2] else None
        d4 = dout.contiguous().view(ctx.shape4)
        dx, dwq, dwk = kernels_for(dout).qk_norm_rope_bwd(d4, x.view(ctx.shape4), rstd, wq, wk, cos, sin, ctx.n_q,
                                                          ctx.n_k, ctx.pos0, mq, mk)
        return (dx.view(dout.shape), dwq if ctx.needs_input_grad[1] else None,
                dwk if ctx.needs_input_grad[2] else None) + (None,) * 9


def _check(x: Tensor, wq: Tensor, wk: Tensor, cos, sin, n_q: int, n_k: int) -> None:
    if x.dim() != 4 or n_q < 0 or n_k < 0 or n_q + n_k > x.shape[2]:
        raise ValueError(f"qk_norm_rope: x must be [B, S, heads, D] with n_q + n_k <= heads, got {tuple(x.shape)}, "
                         f"n_q={n_q}, n_k={n_k}")
    if wq.numel() != x.shape[3] or wk.numel() != x.shape[3]:
        raise ValueError(f"qk_norm_rope: wq and wk must hold D = {x.shape[3]} values, got {wq.numel()} and "
                         f"{wk.numel()}")
    if (cos is None) != (sin is None):
        raise ValueError("qk_norm_rope: give both cos and sin, or neither")


def _native(x: Tensor) -> bool:
    """Whether the HIP kernels take this GPU tensor; a head dim they do not is noted once per shape."""
    D = x.shape[-1]
    if kernels_for(x).qk_norm_rope_supported(D):
        return True
    key = (tuple(x.shape), x.dtype)
    if key not in _noted:
        _noted.add(key)
        warnings.warn(f"qk_norm_rope: head dim {D} is not native (16, 32, 64, 128, 256 are); "
                      f"{tuple(x.shape)} {x.dtype} runs the eager reference", stacklevel=3)
    return False


def _grad_recorded(x: Tensor, wq: Tensor, wk: Tensor) -> bool:
    return torch.is_grad_enabled() and (x.requires_grad or wq.requires_grad or wk.requires_grad)


def qk_norm_rope_heads(x: Tensor, wq: Tensor, wk: Tensor, eps: float, cos: Optional[Tensor], sin: Optional[Tensor],
                       n_q: int, n_k: int, pos0: int = 0, *, inplace: bool = False) -> Tensor:
    """Per-head RMSNorm of the first ``n_q`` (weight ``wq``) and the next ``n_k`` (``wk``) heads of
    ``x [B, S, heads, D]``, rotated for positions ``pos0 .. pos0 + S - 1``; the other heads pass through.
    ``cos = sin = None``: no rotation.

    Out of place by default, like :func:`~mipipe.ops.rope.rope_heads`.  ``inplace=True`` writes into ``x`` itself
    (V is not touched) and returns it, but only where no graph is recorded: the backward needs the un-normalised
    ``x``, so under autograd the call is out of place whatever ``inplace`` says.  Both variants give the same bits.
    For a backward ``x``, the rows' ``rstd`` (fp32 ``[B S, n_q + n_k]``) and the weights are saved; the weight
    gradients are summed in fp32 without atomics and go straight into ``w.main_grad`` where there is one."""
    _check(x, wq, wk, cos, sin, n_q, n_k)
    if not x.is_cuda or not _native(x):
        return qk_norm_rope_reference(x, wq, wk, eps, cos, sin, n_q, n_k, pos0)
    recorded = _grad_recorded(x, wq, wk)
    if not x.is_contiguous():
        x, inplace = x.contiguous(), False
    if recorded:
        inplace = False
    return _QkNormRope.apply(x, wq, wk, float(eps), cos, sin, int(pos0), bool(inplace), tuple(x.shape), int(n_q),
                             int(n_k), recorded)


def qk_norm_rope_projection(proj: Tensor, wq: Tensor, wk: Tensor, eps: float, cos: Optional[Tensor],
                            sin: Optional[Tensor], nhead: int, n_kv_heads: Optional[int] = None,
                            pos0: int = 0) -> Tensor:
    """:func:`qk_norm_rope_heads` for the models, mirroring :func:`~mipipe.ops.rope.rope_projection`: ``proj
    [B, S, (H + 2 Hkv) D]`` is the QKV projection's own output (fresh, read by nothing else).

    In place when no graph is being recorded (a checkpointed stage's first forward, evaluation), out of place under
    autograd; the two give the same bits, so a checkpoint's recompute matches its first forward.  Returns the
    ``[B, S, H + 2 Hkv, D]`` view for grouped-query attention (``n_kv_heads != nhead``) and ``[B, S, 3, H, D]``
    otherwise."""
    hkv = nhead if n_kv_heads is None else int(n_kv_heads)
    B, S, W = proj.shape
    heads = nhead + 2 * hkv
    shape4 = (B, S, heads, W // heads)
    out_shape = shape4 if hkv != nhead else (B, S, 3, nhead, W // heads)
    p4 = proj.reshape(shape4)  # a view of a contiguous projection
    _check(p4, wq, wk, cos, sin, nhead, hkv)
    if not proj.is_cuda or not _native(p4):
        return qk_norm_rope_reference(p4, wq, wk, eps, cos, sin, nhead, hkv, pos0).view(out_shape)
    recorded = _grad_recorded(proj, wq, wk)
    inplace = proj.is_contiguous() and not recorded
    return _QkNormRope.apply(proj.contiguous(), wq, wk, float(eps), cos, sin, int(pos0), inplace, shape4, nhead, hkv,
                             recorded).view(out_shape)
