"""Grouped expert linear over expert-sorted rows (kernels: csrc/kernels/gemm_grouped.hip).

``ops.moe_assign_sorted`` lays the token choices of all experts into one ``[R, E]`` buffer, every expert's segment
padded to whole 128-row tiles.  ``grouped_linear`` multiplies the rows of tile ``i`` by ``weights[tile_expert[i]]^T``::

    slot, src, counts, offsets, tile_expert = moe_assign_sorted(idx, Ne)
    xe = moe_dispatch(x, slot, src)                                  # [R, K], zeros in the padding rows
    ye = grouped_linear(xe, weights, tile_expert, offsets)           # [R, N]

* ``x [R, K]`` with ``R % 128 == 0``; ``weights`` a sequence of ``Ne`` tensors ``[N, K]`` of one shape and dtype.
* A tile whose expert is ``-1`` (the tiles past ``offsets[Ne]``) gives zeros.
* Forward, input gradient and weight gradient are ONE launch each, whatever ``Ne``: the kernels read the tile's
  expert, the expert's row range and the expert's weight pointer from device memory.  The pointer tables are device
  ``int64 [Ne]`` tensors cached on the tuple of pointers, so a steady-state step (the weights are stable views of the
  flat optimizer's buffers) copies nothing to the device.
* Weight gradients go straight into ``main_grad`` (fp32) where every expert has one: a store when the buffers are
  fresh, an accumulation otherwise (:func:`mipipe.ops.linear._claim`), and an expert without rows gets zeros or is
  left alone accordingly.  Without ``main_grad`` they are returned per expert in the weight dtype.  They are NOT
  queued by ``deferred_wgrad()``: they run in the backward, one ``main_grad`` read-modify-write per micro-batch.
  The padding rows of ``x`` must be zeros (dispatch writes them so, and a gated activation keeps them so): then they
  add nothing to a weight gradient whatever ``dy`` holds there.

Native on the GPU for bf16 with ``K % 128 == 0`` and ``N % 128 == 0``; anything else (and the CPU) runs
:func:`grouped_linear_reference`, ``Ne`` masked matmuls without a host synchronisation, and on the GPU says so once per
shape.
"""
from __future__ import annotations

import warnings
from typing import Dict, Sequence, Tuple

import torch
from torch import Tensor

from ._util import kernels_for
from .linear import _aligned, _claim

__all__ = ["grouped_linear", "grouped_linear_reference"]

TILE = 128

_noted = set()
_TABLES: Dict[Tuple, Tensor] = {}
_MAX_TABLES = 1024


def _ptr_table(tensors: Sequence[Tensor]) -> Tensor:
    """Device ``int64 [Ne]`` of the tensors' addresses.  Cached on the addresses: a table stays right for as long as
    it is found, whoever owns the memory by then."""
    dev = tensors[0].device
    key = (dev.index, tuple(t.data_ptr() for t in tensors))
    tab = _TABLES.get(key)
    if tab is None:
        if len(_TABLES) >= _MAX_TABLES:
            _TABLES.clear()
        tab = torch.tensor(key[1], dtype=torch.int64).to(dev)
        _TABLES[key] = tab
    return tab


def grouped_linear_reference(x: Tensor, weights: Sequence[Tensor], tile_expert: Tensor, offsets: Tensor) -> Tensor:
    """Eager oracle and fallback: per expert, the rows of its tiles (the others masked to zero) times ``W_e^T``,
    summed.  ``Ne`` times the work, no host synchronisation.  ``offsets`` is not needed."""
    row_expert = tile_expert.repeat_interleave(TILE)
    y = None
    for e, w in enumerate(weights):
        mine = (row_expert == e)[:, None]
        term = torch.where(mine, x, torch.zeros_like(x)) @ w.t()
        term = torch.where(mine, term, torch.zeros_like(term))
        y = term if y is None else y + term
    return y


class _GroupedLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, tile_expert, offsets, *weights):  # type: ignore[override]
        k = kernels_for(x)
        ctx.save_for_backward(x, tile_expert, offsets, *weights)
        return k.grouped_gemm_rows(x, _ptr_table(weights), tile_expert, weights[0].shape[0], True)

    @staticmethod
    def backward(ctx, dy):  # type: ignore[override]
        x, tile_expert, offsets, *weights = ctx.saved_tensors
        k = kernels_for(x)
        dy = dy.contiguous()
        if not _aligned(dy):
            dy = dy.clone()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = k.grouped_gemm_rows(dy, _ptr_table(weights), tile_expert, x.shape[1], False)
        dws = [None] * len(weights)
        if any(ctx.needs_input_grad[3:]):
            mains = [getattr(w, "main_grad", None) for w in weights]
            if all(m is not None and m.dtype == torch.float32 and m.is_contiguous() and _aligned(m)
                   and m.shape == w.shape and m.device == x.device for m, w in zip(mains, weights)):
                accumulate = [_claim(w) for w in weights]
                if any(accumulate) and not all(accumulate):
                    for m, acc in zip(mains, accumulate):
                        if not acc:
                            m.zero_()
                k.grouped_gemm_wgrad(dy, x, offsets, _ptr_table(mains), any(accumulate))
            else:
                dw = k.grouped_gemm_wgrad(dy, x, offsets, None, False)
                dws = [dw[e].to(w.dtype) if need else None
                       for e, (w, need) in enumerate(zip(weights, ctx.needs_input_grad[3:]))]
        return (dx, None, None, *dws)


def _note(why: str, x: Tensor, w: Tensor) -> None:
    key = (tuple(x.shape), tuple(w.shape), x.dtype)
    if key not in _noted:
        _noted.add(key)
        warnings.warn(f"grouped_linear: {why}; x {tuple(x.shape)} {x.dtype} with weights {tuple(w.shape)} runs the "
                      f"eager reference", stacklevel=3)


def grouped_linear(x: Tensor, weights: Sequence[Tensor], tile_expert: Tensor, offsets: Tensor) -> Tensor:
    """``y [R, N]`` with the rows of 128-row tile ``i`` equal to ``x[tile] @ weights[tile_expert[i]].T`` (zeros for a
    ``-1``); see the module docstring.  ``tile_expert [R / 128]`` and ``offsets [Ne + 1]`` are
    ``ops.moe_assign_sorted``'s."""
    weights = tuple(weights)
    if x.dim() != 2 or x.shape[0] % TILE != 0 or x.shape[0] == 0:
        raise ValueError(f"grouped_linear: x must be [R, K] with R a positive multiple of {TILE}, got {tuple(x.shape)}")
    if not weights:
        raise ValueError("grouped_linear: needs at least one weight")
    w0 = weights[0]
    for w in weights:
        if w.dim() != 2 or w.shape != w0.shape or w.dtype != w0.dtype or w.device != w0.device:
            raise ValueError("grouped_linear: the weights must be [N, K] tensors of one shape, dtype and device")
    if w0.shape[1] != x.shape[1] or w0.dtype != x.dtype or w0.device != x.device:
        raise ValueError(f"grouped_linear: weights {tuple(w0.shape)} {w0.dtype} on {w0.device} do not fit x "
                         f"{tuple(x.shape)} {x.dtype} on {x.device}")
    for name, t, n in (("tile_expert", tile_expert, x.shape[0] // TILE), ("offsets", offsets, len(weights) + 1)):
        if t.dtype != torch.int32 or t.shape != (n,) or t.device != x.device:
            raise ValueError(f"grouped_linear: {name} must be int32 [{n}] on {x.device}, got {t.dtype} "
                             f"{tuple(t.shape)} on {t.device}")
    if not x.is_cuda:
        return grouped_linear_reference(x, weights, tile_expert, offsets)
    n, kk = w0.shape
    if x.dtype != torch.bfloat16:
        _note("only bf16 is native", x, w0)
        return grouped_linear_reference(x, weights, tile_expert, offsets)
    if n % TILE != 0 or kk % TILE != 0:
        _note(f"widths N={n}, K={kk} are not multiples of {TILE}", x, w0)
        return grouped_linear_reference(x, weights, tile_expert, offsets)
    if not all(w.is_contiguous() and _aligned(w) for w in weights):
        _note("the weights are not contiguous and 16-byte aligned", x, w0)
        return grouped_linear_reference(x, weights, tile_expert, offsets)
    x = x.contiguous()
    if not _aligned(x):
        x = x.clone()
    return _GroupedLinear.apply(x, tile_expert.contiguous(), offsets.contiguous(), *weights)
