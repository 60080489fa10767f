"""Gated tanh-GELU of the Gemma-2 MLP (kernel: csrc/kernels/llama.hip).

:mod:`mipipe.ops.swiglu` with another gate: ``gu [..., 2F]`` is the first
linear's output with the gate projection in columns ``[0, F)`` and the up
projection in ``[F, 2F)``; the op returns ``h [..., F] = gelu_tanh(gate) * up``.
The backward writes ONE ``dgu [..., 2F]`` (``[dgate | dup]``) from the saved
``gu``.  No dropout inside.

The GELU is the tanh approximation (``F.gelu(..., approximate="tanh")``, Hugging
Face's ``gelu_pytorch_tanh``), not the erf GELU of ``ops.linear``'s epilogue.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import Tensor

from ._util import kernels_for

__all__ = ["geglu", "geglu_reference"]


def geglu_reference(gu: Tensor) -> Tensor:
    """Eager ``gelu_tanh(g) * u``.  A gate of ``-inf`` takes the GELU's limit
    there, 0 with a zero gradient (``F.gelu(-inf, approximate="tanh")`` itself is
    ``-inf * 0 = nan``)."""
    g, u = gu.chunk(2, dim=-1)
    dead = torch.isneginf(g)
    gelu = F.gelu(torch.where(dead, torch.zeros_like(g), g), approximate="tanh")
    return torch.where(dead, torch.zeros_like(g), gelu) * u


class _GeGLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gu):  # type: ignore[override]
        k = kernels_for(gu)
        guc = gu.contiguous()
        ctx.save_for_backward(guc)
        return k.geglu_fwd(guc)

    @staticmethod
    def backward(ctx, dh):  # type: ignore[override]
        (gu,) = ctx.saved_tensors
        return kernels_for(dh).geglu_bwd(dh.contiguous(), gu)


def geglu(gu: Tensor) -> Tensor:
    """``gelu_tanh(gu[..., :F]) * gu[..., F:]`` for ``gu [..., 2F]``, ``F % 8 == 0`` on the GPU."""
    if gu.shape[-1] % 2 != 0:
        raise ValueError(f"geglu: the last dimension holds gate and up halves, got {gu.shape[-1]}")
    if not gu.is_cuda:
        return geglu_reference(gu)
    return _GeGLU.apply(gu)
