"""Gated SiLU of the LLaMA-style MLP (kernel: csrc/kernels/llama.hip).

``gu [..., 2F]`` is the first linear's output with the gate projection in
columns ``[0, F)`` and the up projection in ``[F, 2F)``; the op returns
``h [..., F] = silu(gate) * up``.  The backward writes ONE ``dgu [..., 2F]``
(``[dgate | dup]``), which feeds that linear's dgrad and wgrad GEMMs without a
concatenation.  No dropout inside.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import Tensor

from ._util import kernels_for

__all__ = ["swiglu", "swiglu_reference"]


def swiglu_reference(gu: Tensor) -> Tensor:
    """Eager ``silu(g) * u``.  A gate of ``-inf`` takes silu's limit there, 0
    with a zero gradient (``F.silu(-inf)`` itself is ``-inf * 0 = nan``)."""
    g, u = gu.chunk(2, dim=-1)
    dead = torch.isneginf(g)
    silu = F.silu(torch.where(dead, torch.zeros_like(g), g))
    return torch.where(dead, torch.zeros_like(g), silu) * u


class _SwiGLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gu):  # type: ignore[override]
        k = kernels_for(gu)
        guc = gu.contiguous()
        ctx.save_for_backward(guc)
        return k.swiglu_fwd(guc)

    @staticmethod
    def backward(ctx, dh):  # type: ignore[override]
        (gu,) = ctx.saved_tensors
        return kernels_for(dh).swiglu_bwd(dh.contiguous(), gu)


def swiglu(gu: Tensor) -> Tensor:
    """``silu(gu[..., :F]) * gu[..., F:]`` for ``gu [..., 2F]``, ``F % 8 == 0`` on the GPU."""
    if gu.shape[-1] % 2 != 0:
        raise ValueError(f"swiglu: the last dimension holds gate and up halves, got {gu.shape[-1]}")
    if not gu.is_cuda:
        return swiglu_reference(gu)
    return _SwiGLU.apply(gu)
