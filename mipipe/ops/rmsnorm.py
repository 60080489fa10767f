"""Fused ``RMSNorm(residual + dropout(x))`` (kernel: csrc/kernels/rmsnorm.hip).

``y = z * rsqrt(mean(z^2) + eps) * weight`` with ``z = residual + dropout(x)``:
the LLaMA-style block's norm, with the contract of :mod:`mipipe.ops.layernorm`
(no mean, no bias).  GPU tensors always go to the HIP kernel (a missing
extension raises); CPU tensors use the eager reference so CPU-only tests
exercise the same module code.

``rms_norm_residual`` is the sandwich norm of the Gemma-2 block, the norm on
the branch instead of on the sum: ``y = residual + x * rsqrt(mean(x^2) + eps) *
weight`` -- a variant of the same forward kernels (one pass: ``x``, ``residual``
and ``weight`` read, ``y`` and ``rstd`` written) and, for ``x`` and ``weight``,
the same backward kernels on the saved ``x``; the residual's gradient is the
output's, the same tensor.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F
from torch import Tensor

from ._util import kernels_for
from .linear import accumulable

__all__ = ["add_dropout_rms_norm", "rms_norm_fanout", "rms_norm_reference", "rms_norm_residual",
           "rms_norm_residual_reference"]


def rms_norm_reference(x: Tensor, residual: Optional[Tensor], weight: Tensor, eps: float, p: float,
                       training: bool) -> Tensor:
    h = F.dropout(x, p, training) if p > 0 else x
    if residual is not None:
        h = residual + h
    # statistics in fp32 at least, as in the kernel
    hf = h.float() if h.dtype in (torch.bfloat16, torch.float16) else h
    y = hf * torch.rsqrt(hf.pow(2).mean(-1, keepdim=True) + eps) * weight.to(hf.dtype)
    return y.to(h.dtype)


class _AddDropoutRmsNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, weight, eps, p, fanout=False, save=True):  # type: ignore[override]
        ctx.set_materialize_grads(False)
        k = kernels_for(x)
        xc = x.contiguous()
        rc = residual.contiguous() if residual is not None else None
        # z (the normalised sum) is written only for a backward, and only when it
        # is not the input itself: a pre-norm RMSNorm (no residual, no dropout)
        # saves x, and a forward under no_grad (a checkpointed stage) saves nothing
        z_is_x = residual is None and p == 0.0
        y, z, rstd, seed, offset = k.rmsnorm_fwd(xc, rc, weight, eps, p, save and not z_is_x)
        if save and z_is_x:
            z = xc
        ctx.save_for_backward(z, rstd, weight)
        ctx.p = p
        ctx.seed = seed
        ctx.offset = offset
        ctx.has_residual = residual is not None
        if fanout:
            # x again for its other consumer (pre-norm residual); its gradient
            # is added to dx inside the RMSNorm backward kernel
            return y, x.view_as(x)
        return y

    @staticmethod
    def backward(ctx, dy, dfan=None):  # type: ignore[override]
        z, rstd, weight = ctx.saved_tensors
        if dy is None:  # only the fan-out branch carries a gradient
            return dfan, None, None, None, None, None, None
        k = kernels_for(dy)
        # dgamma accumulates straight into the fp32 main_grad buffer when there is one
        mg = accumulable(weight)
        add = dfan.contiguous() if dfan is not None and dfan.dtype == dy.dtype else None
        dz, dx, dgamma = k.rmsnorm_bwd(dy.contiguous(), z, rstd, weight, ctx.p, ctx.seed, ctx.offset, mg, add)
        if dx is None:
            dx = dz
        if dfan is not None and add is None:
            dx = dx + dfan
        dres = dz if ctx.has_residual else None
        return dx, dres, dgamma, None, None, None, None


def add_dropout_rms_norm(
    x: Tensor,
    residual: Optional[Tensor],
    weight: Tensor,
    eps: float = 1e-5,
    p: float = 0.0,
    training: bool = True,
) -> Tensor:
    """``RMSNorm(residual + dropout(x, p))`` with the affine ``weight``."""
    p = float(p) if training else 0.0
    if not x.is_cuda:
        return rms_norm_reference(x, residual, weight, eps, p, True)
    return _AddDropoutRmsNorm.apply(x, residual, weight, float(eps), p, False, torch.is_grad_enabled())


def rms_norm_fanout(x: Tensor, weight: Tensor, eps: float = 1e-5):
    """``(RMSNorm(x), x')``: ``x'`` is ``x`` for its other consumer (the
    pre-norm residual ``x' + f(RMSNorm(x))``); the gradient reaching ``x'`` is
    added inside the RMSNorm backward kernel instead of by an autograd add kernel."""
    if not x.is_cuda or not torch.is_grad_enabled() or not x.requires_grad:
        return add_dropout_rms_norm(x, None, weight, eps, 0.0, True), x
    return _AddDropoutRmsNorm.apply(x, None, weight, float(eps), 0.0, True)


def rms_norm_residual_reference(x: Tensor, residual: Tensor, weight: Tensor, eps: float) -> Tensor:
    """Eager ``residual + RMSNorm(x) * weight``: fp32 at least, one rounding at the end."""
    xf = x.float() if x.dtype in (torch.bfloat16, torch.float16) else x
    y = residual.to(xf.dtype) + xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * weight.to(xf.dtype)
    return y.to(x.dtype)


class _RmsNormResidual(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, weight, eps, save=True):  # type: ignore[override]
        ctx.set_materialize_grads(False)
        xc = x.contiguous()
        # rstd is written only for a backward; x (the GEMM's output) is saved as it is
        y, rstd = kernels_for(x).rmsnorm_residual_fwd(xc, residual.contiguous(), weight, eps, save)
        if save:
            ctx.save_for_backward(xc, rstd, weight)
        return y

    @staticmethod
    def backward(ctx, dy):  # type: ignore[override]
        if dy is None:
            return None, None, None, None, None
        x, rstd, weight = ctx.saved_tensors
        dx = dgamma = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[2]:
            # dgamma accumulates straight into the fp32 main_grad buffer when there is one
            dx, _, dgamma = kernels_for(dy).rmsnorm_bwd(dy.contiguous(), x, rstd, weight, 0.0, 0, 0,
                                                        accumulable(weight), None)
        return dx, dy, dgamma, None, None


def rms_norm_residual(x: Tensor, residual: Tensor, weight: Tensor, eps: float = 1e-5) -> Tensor:
    """``residual + RMSNorm(x) * weight``, the statistics from ``x`` alone (no dropout)."""
    if x.shape != residual.shape:
        raise ValueError(f"rms_norm_residual: x {tuple(x.shape)} and residual {tuple(residual.shape)} differ")
    if not x.is_cuda:
        return rms_norm_residual_reference(x, residual, weight, eps)
    return _RmsNormResidual.apply(x, residual, weight, float(eps), torch.is_grad_enabled())
