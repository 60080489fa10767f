"""Logit soft-capping ``y = cap * tanh(x / cap)`` (kernels: csrc/kernels/elementwise.hip).

Gemma-2's ``final_logit_softcapping``: the values stay inside ``(-cap, cap)`` and
near 0 the map is the identity.  bf16 and fp32; the arithmetic is fp32 with one
rounding at the store.  The backward is ``dx = dy * (1 - (y / cap)^2)``, computed
from the saved **output**, so the input is not kept: with ``inplace=True`` the
output overwrites the input and the op holds no tensor of its own.

The kernels read rows of the last dim: any tensor with unit stride there whose
leading dims collapse to one row stride -- a contiguous tensor, or the
``[..., :V]`` view of a padded buffer -- is read where it lies; anything else is
made contiguous first.  CPU tensors use eager math.
"""
from __future__ import annotations

import math

import torch
from torch import Tensor

from ._util import kernels_for

__all__ = ["softcap", "softcap_owned", "softcap_reference"]


def _check_cap(cap) -> float:
    if isinstance(cap, bool) or not isinstance(cap, (int, float)):
        raise ValueError(f"softcap: cap must be a finite number > 0, got {cap!r}")
    if not math.isfinite(cap) or cap <= 0:
        raise ValueError(f"softcap: cap must be finite and > 0, got {cap!r}")
    return float(cap)


def softcap_reference(x: Tensor, cap: float) -> Tensor:
    """Eager math in fp32 (CPU path and test oracle)."""
    cap = _check_cap(cap)
    return (cap * torch.tanh(x.float() / cap)).to(x.dtype)


def _rows_ok(t: Tensor) -> bool:
    """True if the kernels can read ``t`` in place: unit stride on the last dim, one row stride."""
    if t.dim() == 0:
        return True
    if t.shape[-1] > 1 and t.stride(-1) != 1:
        return False
    if t.dim() == 1:
        return True
    if t.shape[-2] > 1 and t.stride(-2) < t.shape[-1]:
        return False
    expect = t.stride(-2) * t.shape[-2]
    for size, st in zip(reversed(t.shape[:-2]), reversed(t.stride()[:-2])):
        if size > 1 and st != expect:
            return False
        expect = st * size
    return True


class _Softcap(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cap, inplace):  # type: ignore[override]
        k = kernels_for(x)
        if inplace:
            k.softcap_fwd(x, cap, x)
            ctx.mark_dirty(x)
            y = x
        else:
            y = k.softcap_fwd(x, cap)
        ctx.save_for_backward(y)
        ctx.cap = cap
        return y

    @staticmethod
    def backward(ctx, dy):  # type: ignore[override]
        (y,) = ctx.saved_tensors
        k = kernels_for(dy)
        if not _rows_ok(dy):
            dy = dy.contiguous()
        return k.softcap_bwd(dy, y, ctx.cap), None, None


class _SoftcapOwned(torch.autograd.Function):
    """The cap written over ``x``'s values for a caller that owns ``x`` (:func:`softcap_owned`).  Autograd's own
    in-place route (``mark_dirty``) refuses the output of another custom Function that is a view -- which
    ``ops.linear``'s is -- so the overwrite is not declared: the result is a new alias of the same storage."""

    @staticmethod
    def forward(ctx, x, cap):  # type: ignore[override]
        kernels_for(x).softcap_fwd(x, cap, x)
        y = x.view_as(x)
        ctx.save_for_backward(y)
        ctx.cap = cap
        return y

    @staticmethod
    def backward(ctx, dy):  # type: ignore[override]
        (y,) = ctx.saved_tensors
        if not _rows_ok(dy):
            dy = dy.contiguous()
        return kernels_for(dy).softcap_bwd(dy, y, ctx.cap), None


def softcap_owned(x: Tensor, cap: float) -> Tensor:
    """:func:`softcap` over the values of a tensor the caller owns, under autograd too, at no memory of its own:
    the capped values replace ``x``'s and are what the backward reads.  The caller guarantees that ``x`` is not
    used again -- not by itself, not by the backward of the op that made it (``ops.linear`` without an
    activation saves nothing of its output) -- because autograd is not told of the overwrite.  The models'
    decoder caps its logits GEMM's output this way; CPU tensors get the eager result in a new tensor."""
    cap = _check_cap(cap)
    if not x.is_cuda:
        return softcap_reference(x, cap)
    if not _rows_ok(x):
        raise ValueError("softcap_owned: needs unit stride on the last dim and one row stride")
    if not (torch.is_grad_enabled() and x.requires_grad):
        kernels_for(x).softcap_fwd(x, cap, x)
        return x
    return _SoftcapOwned.apply(x, cap)


def softcap(x: Tensor, cap: float, *, inplace: bool = False) -> Tensor:
    """``cap * tanh(x / cap)``.  ``inplace=True`` overwrites ``x`` (under autograd too: the backward needs the
    output only; autograd itself refuses where ``x``'s producer saved ``x``, and where ``x`` is a view made inside
    another custom Function -- see :func:`softcap_owned` for that case)."""
    cap = _check_cap(cap)
    if not x.is_cuda:
        y = softcap_reference(x, cap)
        return x.copy_(y) if inplace and not (torch.is_grad_enabled() and x.requires_grad) else y
    if not _rows_ok(x):
        if inplace:
            raise ValueError("softcap: inplace=True needs unit stride on the last dim and one row stride")
        x = x.contiguous()
    return _Softcap.apply(x, cap, bool(inplace))
