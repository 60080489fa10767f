"""Mixture-of-experts routing ops (kernels: csrc/kernels/moe.hip).

``T`` tokens choose ``k`` of ``Ne`` experts; every expert has ``C`` slots, so
every tensor has a static shape.  ``a = t * k + j`` is token ``t``'s ``j``-th
choice.  Four ops, in the order a block calls them::

    idx, gate, probs_sum = moe_route(logits, k)          # top-k + softmax over the k
    slot, src, counts    = moe_assign(idx, Ne, C)        # (t, j) -> e * C + pos, or -1 (dropped)
    xe = moe_dispatch(x, slot, src)                      # [Ne * C, E]: expert e's rows are xe[e * C : (e + 1) * C]
    y  = moe_combine(ye, gate, slot, src, residual=x)    # y[t] = x[t] + sum_j gate[t, j] ye[slot[t, j]]

* ``idx [T, k]`` (int32): the ``k`` largest logits of a row in descending order,
  the lower expert first among equal logits.  ``gate [T, k]`` (fp32): the softmax
  over those ``k`` (Mixtral's, Qwen3-MoE's ``norm_topk_prob=True`` and gpt-oss's
  gate); a selected ``-inf`` gets exactly 0.  ``probs_sum [Ne]`` (fp32): the
  full-row softmax summed over the tokens, for the load-balancing loss.
* ``pos`` counts the entries of the same expert that come earlier in choice-major
  order (``j`` first, then ``t``): a token's first choice never loses its place
  to another token's second choice.  ``(t, j)`` is dropped iff ``pos >= C``.
  ``src [Ne * C]`` is the ``a`` that owns a slot, ``-1`` for an empty one;
  ``counts [Ne]`` the choices per expert before the capacity.
* Empty slots of ``xe`` hold zeros.  The combine sums in fp32 in ``j`` order,
  adds the residual in fp32 and rounds once.

GPU tensors go to the HIP kernels (a missing extension raises): no sort, no
float atomics, no host synchronisation, the same bits on every run.  A width
that does not fill 16-byte vectors, a single expert or another dtype than bf16 /
fp32 takes the eager reference and says so once per shape.  CPU tensors use the
references.

The dropless variant of the second step, for ``ops.grouped_linear``::

    slot, src, counts, offsets, tile_expert = moe_assign_sorted(idx, Ne)

sorts the choices by expert into ``R = moe_sorted_rows(T, Ne, k)`` rows, every expert's segment padded to whole
128-row tiles (see :func:`moe_assign_sorted`); dispatch and combine take its tables unchanged.
"""
from __future__ import annotations

import math
import warnings
from typing import Optional, Tuple

import torch
from torch import Tensor

from ._util import kernels_for

__all__ = ["moe_route", "moe_assign", "moe_dispatch", "moe_combine", "moe_capacity", "moe_route_reference",
           "moe_assign_reference", "moe_dispatch_reference", "moe_combine_reference", "moe_attach_aux",
           "moe_assign_sorted", "moe_assign_sorted_reference", "moe_sorted_rows", "MAX_EXPERTS", "MAX_TOP_K"]

MAX_EXPERTS = 256
MAX_TOP_K = 8

_noted = set()


def _ceil64(n: int) -> int:
    return (n + 63) // 64 * 64


def moe_capacity(tokens: int, n_experts: int, k: int, capacity_factor: Optional[float]) -> int:
    """Slots per expert: ``ceil(capacity_factor * tokens * k / n_experts)`` rounded up to a multiple of 64 (the
    experts' weight-gradient GEMM has ``K = C`` and runs whole 64-deep K tiles) and clamped to ``ceil64(tokens)``
    (top-k picks distinct experts: no expert can receive more than ``tokens``).  ``capacity_factor=None`` gives
    ``ceil64(tokens)``: nothing is dropped, at ``n_experts / k`` times the GEMM work."""
    if tokens < 1 or n_experts < 1 or k < 1:
        raise ValueError(f"moe_capacity: tokens, n_experts and k must be >= 1, got {tokens}, {n_experts}, {k}")
    top = _ceil64(tokens)
    if capacity_factor is None:
        return top
    if not math.isfinite(capacity_factor) or capacity_factor <= 0:
        raise ValueError(f"moe_capacity: capacity_factor must be a finite number > 0 or None, got {capacity_factor!r}")
    return min(_ceil64(max(1, math.ceil(capacity_factor * tokens * k / n_experts))), top)


# ------------------------------------------------------------------ references
def moe_route_reference(logits: Tensor, k: int) -> Tuple[Tensor, Tensor, Tensor]:
    """Eager route (CPU path and test oracle): a stable descending sort of the fp32 values (fp64 stays fp64)."""
    wide = torch.promote_types(logits.dtype, torch.float32)
    lf = logits.to(wide)
    vals, order = torch.sort(lf, dim=-1, descending=True, stable=True)
    idx = order[:, :k].to(torch.int32)
    gate = torch.softmax(vals[:, :k], dim=-1)
    probs_sum = torch.softmax(lf, dim=-1).sum(0)
    return idx, gate, probs_sum


def moe_assign_reference(idx: Tensor, n_experts: int, capacity: int) -> Tuple[Tensor, Tensor, Tensor]:
    """Eager assignment: a cumulative sum of one-hots in choice-major order."""
    T, k = idx.shape
    flat = idx.t().reshape(-1).long()  # entry q = j * T + t
    onehot = torch.nn.functional.one_hot(flat, n_experts)
    pos = (onehot.cumsum(0) - onehot).gather(1, flat[:, None]).squeeze(1)
    counts = onehot.sum(0).to(torch.int32)
    keep = pos < capacity
    slot_cm = torch.where(keep, flat * capacity + pos, torch.full_like(pos, -1))
    q = torch.arange(T * k, device=idx.device)
    a = (q % max(T, 1)) * k + q // max(T, 1)
    # masked_scatter-free and sync-free: the dropped entries write to a spare last element
    src = torch.full((n_experts * capacity + 1,), -1, dtype=torch.int64, device=idx.device)
    src.scatter_(0, torch.where(keep, slot_cm, torch.full_like(pos, n_experts * capacity)),
                 torch.where(keep, a, torch.full_like(a, -1)))
    slot = slot_cm.view(k, T).t().contiguous().to(torch.int32)
    return slot, src[:-1].to(torch.int32), counts


def moe_dispatch_reference(x: Tensor, slot: Tensor, src: Tensor) -> Tensor:
    k = slot.shape[1]
    rows = x.index_select(0, torch.div(src.clamp(min=0), k, rounding_mode="floor").long())
    return torch.where((src >= 0)[:, None], rows, torch.zeros_like(rows))


def moe_combine_reference(ye: Tensor, gate: Tensor, slot: Tensor, src: Tensor,
                          residual: Optional[Tensor] = None) -> Tensor:
    wide = torch.promote_types(ye.dtype, torch.float32)
    rows = ye.to(wide)[slot.clamp(min=0).long()]  # [T, k, E]
    terms = torch.where((slot >= 0)[..., None], rows * gate.to(wide)[..., None], torch.zeros_like(rows))
    y = terms.sum(1)
    if residual is not None:
        y = y + residual.to(wide)
    return y.to(ye.dtype)


# ------------------------------------------------------------------ checks
def _check_k(name: str, n_experts: int, k: int) -> None:
    if n_experts < 1:
        raise ValueError(f"{name}: needs at least one expert, got {n_experts}")
    if n_experts > MAX_EXPERTS:
        raise ValueError(f"{name}: at most {MAX_EXPERTS} experts are supported, got {n_experts}")
    if k < 1:
        raise ValueError(f"{name}: k must be >= 1, got {k}")
    if k > MAX_TOP_K:
        raise ValueError(f"{name}: at most {MAX_TOP_K} experts per token are supported, got k={k}")
    if k > n_experts:
        raise ValueError(f"{name}: k={k} experts per token out of {n_experts}")


def _check_index(name: str, what: str, t: Tensor, like: Tensor) -> None:
    if t.dtype != torch.int32:
        raise ValueError(f"{name}: {what} must be int32, got {t.dtype}")
    if t.device != like.device:
        raise ValueError(f"{name}: {what} is on {t.device}, the values on {like.device}")


def _note(name: str, why: str, t: Tensor) -> None:
    key = (name, tuple(t.shape), t.dtype)
    if key not in _noted:
        _noted.add(key)
        warnings.warn(f"{name}: {why}; {tuple(t.shape)} {t.dtype} runs the eager reference", stacklevel=4)


def _native_rows(name: str, t: Tensor) -> bool:
    """Whether the row kernels take ``t [rows, E]`` on the GPU."""
    if t.dtype not in (torch.bfloat16, torch.float32):
        _note(name, "only bf16 and fp32 are native", t)
        return False
    if (t.shape[-1] * t.element_size()) % 16 != 0:
        _note(name, f"width {t.shape[-1]} does not fill 16-byte vectors", t)
        return False
    return True


# ------------------------------------------------------------------ route
class _MoeRoute(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, k):  # type: ignore[override]
        ctx.set_materialize_grads(False)
        idx, gate, probs_sum = kernels_for(logits).moe_route_fwd(logits, k)
        ctx.save_for_backward(logits, idx, gate)
        ctx.mark_non_differentiable(idx)
        return idx, gate, probs_sum

    @staticmethod
    def backward(ctx, _didx, dgate, dprobs):  # type: ignore[override]
        logits, idx, gate = ctx.saved_tensors
        if dgate is None and dprobs is None:
            return None, None
        dgate = torch.zeros_like(gate) if dgate is None else dgate.contiguous().float()
        if dprobs is not None:
            dprobs = dprobs.contiguous().float()
        return kernels_for(logits).moe_route_bwd(logits, idx, gate, dgate, dprobs), None


def moe_route(logits: Tensor, k: int) -> Tuple[Tensor, Tensor, Tensor]:
    """``(idx, gate, probs_sum)`` of ``logits [T, Ne]`` (see the module docstring).  The logits are finite or
    ``-inf`` with at least one finite value per row.  Differentiable in ``gate`` and ``probs_sum``."""
    if logits.dim() != 2:
        raise ValueError(f"moe_route: logits must be [T, Ne], got {tuple(logits.shape)}")
    if not logits.dtype.is_floating_point:
        raise ValueError(f"moe_route: logits must be floating point, got {logits.dtype}")
    k = int(k)
    _check_k("moe_route", logits.shape[1], k)
    if not logits.is_cuda:
        return moe_route_reference(logits, k)
    if logits.dtype not in (torch.bfloat16, torch.float32):
        _note("moe_route", "only bf16 and fp32 are native", logits)
        return moe_route_reference(logits, k)
    if logits.shape[1] < 2:
        _note("moe_route", "a single expert is not native", logits)
        return moe_route_reference(logits, k)
    return _MoeRoute.apply(logits.contiguous(), k)


class _AttachAux(torch.autograd.Function):
    """``gate`` unchanged; the backward hands ``dprobs`` to ``probs_sum``."""

    @staticmethod
    def forward(ctx, gate, probs_sum, dprobs):  # type: ignore[override]
        ctx.save_for_backward(dprobs)
        return gate.view_as(gate)

    @staticmethod
    def backward(ctx, dgate):  # type: ignore[override]
        (dprobs,) = ctx.saved_tensors
        return dgate, dprobs, None


def moe_attach_aux(gate: Tensor, probs_sum: Tensor, dprobs: Tensor) -> Tensor:
    """Returns ``gate``; in the backward ``probs_sum`` receives the constant gradient ``dprobs [Ne]``, together with
    the gate's own gradient, so the router's backward runs once.  This is how a block's load-balancing loss reaches
    the router without being part of the loss tensor."""
    if dprobs.shape != probs_sum.shape:
        raise ValueError(f"moe_attach_aux: dprobs {tuple(dprobs.shape)} must match probs_sum {tuple(probs_sum.shape)}")
    return _AttachAux.apply(gate, probs_sum, dprobs.to(probs_sum.dtype))


# ------------------------------------------------------------------ assign
def moe_assign(idx: Tensor, n_experts: int, capacity: int) -> Tuple[Tensor, Tensor, Tensor]:
    """``(slot [T, k], src [Ne * C], counts [Ne])``, all int32, of ``idx [T, k]`` (see the module docstring)."""
    if idx.dim() != 2:
        raise ValueError(f"moe_assign: idx must be [T, k], got {tuple(idx.shape)}")
    _check_index("moe_assign", "idx", idx, idx)
    n_experts, capacity = int(n_experts), int(capacity)
    _check_k("moe_assign", n_experts, idx.shape[1])
    if capacity < 1:
        raise ValueError(f"moe_assign: capacity must be >= 1, got {capacity}")
    if n_experts * capacity >= 2 ** 31:
        raise ValueError(f"moe_assign: n_experts * capacity must be below 2^31, got {n_experts} * {capacity}")
    if not idx.is_cuda:
        return moe_assign_reference(idx, n_experts, capacity)
    if n_experts < 2:
        _note("moe_assign", "a single expert is not native", idx)
        return moe_assign_reference(idx, n_experts, capacity)
    return kernels_for(idx).moe_assign(idx.contiguous(), n_experts, capacity)


def moe_sorted_rows(tokens: int, n_experts: int, k: int) -> int:
    """Rows of the sorted layout: the largest ``sum_e ceil128(c_e)`` over every count vector with ``sum_e c_e =
    tokens * k``.  With ``n = min(n_experts, tokens * k)`` the worst vector gives ``n`` experts one entry each (a
    whole tile for one row) and every further 128 entries fill one more tile: ``128 * (n + (tokens * k - n) //
    128)``.  Static: it depends on no routing decision."""
    if tokens < 1 or n_experts < 1 or k < 1:
        raise ValueError(f"moe_sorted_rows: tokens, n_experts and k must be >= 1, got {tokens}, {n_experts}, {k}")
    n = min(n_experts, tokens * k)
    return 128 * (n + (tokens * k - n) // 128)


def moe_assign_sorted_reference(idx: Tensor, n_experts: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """Eager sorted assignment: :func:`moe_assign_reference`'s cumulative sums, the experts' segments padded to whole
    128-row tiles and laid end to end.  No host synchronisation."""
    T, k = idx.shape
    rows = moe_sorted_rows(T, n_experts, k)
    raw = idx.t().reshape(-1).long()  # entry q = j * T + t
    valid = (raw >= 0) & (raw < n_experts)
    flat = raw.clamp(0, n_experts - 1)
    onehot = torch.nn.functional.one_hot(flat, n_experts) * valid[:, None]
    pos = (onehot.cumsum(0) - onehot).gather(1, flat[:, None]).squeeze(1)
    counts = onehot.sum(0)
    ends = ((counts + 127) // 128 * 128).cumsum(0)
    offsets = torch.cat([torch.zeros_like(ends[:1]), ends])
    slot_cm = torch.where(valid, offsets[flat] + pos, torch.full_like(pos, -1))
    q = torch.arange(T * k, device=idx.device)
    a = (q % T) * k + q // T
    # the invalid entries write to a spare last element
    src = torch.full((rows + 1,), -1, dtype=torch.int64, device=idx.device)
    src.scatter_(0, torch.where(valid, slot_cm, torch.full_like(pos, rows)),
                 torch.where(valid, a, torch.full_like(a, -1)))
    # a tile's expert: the number of segment ends at or before its first row (empty experts end where they start)
    starts = torch.arange(rows // 128, device=idx.device) * 128
    te = torch.searchsorted(ends, starts, right=True)
    te = torch.where(te < n_experts, te, torch.full_like(te, -1))
    slot = slot_cm.view(k, T).t().contiguous().to(torch.int32)
    return (slot, src[:-1].to(torch.int32), counts.to(torch.int32), offsets.to(torch.int32), te.to(torch.int32))


def moe_assign_sorted(idx: Tensor, n_experts: int) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """The dropless layout: ``(slot [T, k], src [R], counts [Ne], offsets [Ne + 1], tile_expert [R / 128])``, all
    int32, with ``R = moe_sorted_rows(T, Ne, k)``.  Expert ``e`` owns rows ``[offsets[e], offsets[e + 1])``,
    ``offsets[e + 1] = offsets[e] + ceil128(counts[e])``; ``slot = offsets[e] + pos`` with :func:`moe_assign`'s ``pos``
    (``-1`` only for an ``idx`` outside ``[0, Ne)``); ``src`` is the owning ``a`` or ``-1`` for a padding row;
    ``tile_expert`` the expert of each 128-row tile, ``-1`` past ``offsets[Ne]``.  :func:`moe_dispatch` and
    :func:`moe_combine` take ``slot`` and ``src`` as they are; ``ops.grouped_linear`` takes the other two."""
    if idx.dim() != 2:
        raise ValueError(f"moe_assign_sorted: idx must be [T, k], got {tuple(idx.shape)}")
    _check_index("moe_assign_sorted", "idx", idx, idx)
    n_experts = int(n_experts)
    _check_k("moe_assign_sorted", n_experts, idx.shape[1])
    if idx.shape[0] < 1:
        raise ValueError("moe_assign_sorted: needs at least one token")
    rows = moe_sorted_rows(idx.shape[0], n_experts, idx.shape[1])
    if rows >= 2 ** 31:
        raise ValueError(f"moe_assign_sorted: the sorted layout must stay below 2^31 rows, got {rows}")
    if not idx.is_cuda:
        return moe_assign_sorted_reference(idx, n_experts)
    if n_experts < 2:
        _note("moe_assign_sorted", "a single expert is not native", idx)
        return moe_assign_sorted_reference(idx, n_experts)
    return kernels_for(idx).moe_assign_sorted(idx.contiguous(), n_experts, rows)


# ------------------------------------------------------------------ dispatch / combine
def _check_tables(name: str, rows: Tensor, slot: Tensor, src: Tensor) -> None:
    if slot.dim() != 2 or src.dim() != 1:
        raise ValueError(f"{name}: slot must be [T, k] and src [Ne * C], got {tuple(slot.shape)} and "
                         f"{tuple(src.shape)}")
    if not 1 <= slot.shape[1] <= MAX_TOP_K:
        raise ValueError(f"{name}: at most {MAX_TOP_K} experts per token are supported, got k={slot.shape[1]}")
    _check_index(name, "slot", slot, rows)
    _check_index(name, "src", src, rows)


class _MoeDispatch(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, slot, src):  # type: ignore[override]
        ctx.save_for_backward(slot)
        return kernels_for(x).moe_gather_slots(x, src, slot.shape[1])

    @staticmethod
    def backward(ctx, dxe):  # type: ignore[override]
        (slot,) = ctx.saved_tensors
        return kernels_for(dxe).moe_gather_tokens(dxe.contiguous(), slot), None, None


def moe_dispatch(x: Tensor, slot: Tensor, src: Tensor) -> Tensor:
    """``xe [Ne * C, E]`` with ``xe[s] = x[src[s] // k]`` and zeros in the empty slots, for ``x [T, E]``: a bit-exact
    copy.  Backward: ``dx[t] = sum_j dxe[slot[t, j]]`` over the kept choices, summed in fp32 and rounded once."""
    if x.dim() != 2:
        raise ValueError(f"moe_dispatch: x must be [T, E], got {tuple(x.shape)}")
    _check_tables("moe_dispatch", x, slot, src)
    if slot.shape[0] != x.shape[0]:
        raise ValueError(f"moe_dispatch: slot has {slot.shape[0]} tokens, x {x.shape[0]}")
    if not x.is_cuda or not _native_rows("moe_dispatch", x):
        return moe_dispatch_reference(x, slot, src)
    return _MoeDispatch.apply(x.contiguous(), slot.contiguous(), src.contiguous())


class _MoeCombine(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ye, gate, slot, src, residual):  # type: ignore[override]
        ctx.save_for_backward(ye, gate, src)
        ctx.has_residual = residual is not None
        return kernels_for(ye).moe_gather_tokens(ye, slot, gate, residual)

    @staticmethod
    def backward(ctx, dy):  # type: ignore[override]
        ye, gate, src = ctx.saved_tensors
        dy = dy.contiguous()
        dye, dgate = kernels_for(dy).moe_combine_bwd(dy, ye, gate, src)
        return dye, dgate, None, None, (dy if ctx.has_residual else None)


def moe_combine(ye: Tensor, gate: Tensor, slot: Tensor, src: Tensor, residual: Optional[Tensor] = None) -> Tensor:
    """``y [T, E]`` with ``y[t] = (residual[t]) + sum_j gate[t, j] ye[slot[t, j]]`` over the kept choices, for the
    experts' outputs ``ye [Ne * C, E]``: fp32 in ``j`` order, the residual added in fp32, one rounding.  Backward:
    one pass over the slots gives ``dye[s] = gate[a] dy[t]`` (zeros in the empty slots) and ``dgate[a] = <dy[t],
    ye[s]>`` (0 for a dropped choice); the residual's gradient is ``dy`` itself."""
    if ye.dim() != 2:
        raise ValueError(f"moe_combine: ye must be [Ne * C, E], got {tuple(ye.shape)}")
    _check_tables("moe_combine", ye, slot, src)
    if src.shape[0] != ye.shape[0]:
        raise ValueError(f"moe_combine: src has {src.shape[0]} slots, ye {ye.shape[0]} rows")
    if gate.shape != slot.shape:
        raise ValueError(f"moe_combine: gate {tuple(gate.shape)} must match slot {tuple(slot.shape)}")
    want = torch.promote_types(ye.dtype, torch.float32)
    if gate.dtype != want:
        raise ValueError(f"moe_combine: gate must be {want} for {ye.dtype} values, got {gate.dtype}")
    if gate.device != ye.device:
        raise ValueError(f"moe_combine: gate is on {gate.device}, ye on {ye.device}")
    if residual is not None:
        if residual.shape != (slot.shape[0], ye.shape[1]):
            raise ValueError(f"moe_combine: residual must be [T, E] = [{slot.shape[0]}, {ye.shape[1]}], got "
                             f"{tuple(residual.shape)}")
        if residual.dtype != ye.dtype or residual.device != ye.device:
            raise ValueError(f"moe_combine: residual ({residual.dtype}, {residual.device}) must match ye "
                             f"({ye.dtype}, {ye.device})")
    if not ye.is_cuda or not _native_rows("moe_combine", ye):
        return moe_combine_reference(ye, gate, slot, src, residual)
    return _MoeCombine.apply(ye.contiguous(), gate.contiguous(), slot.contiguous(), src.contiguous(),
                             None if residual is None else residual.contiguous())
