"""Scaled dot-product attention on the HIP flash-attention kernels
(csrc/kernels/attention.hip).

Three entry points:

* :func:`attention_packed` -- ``qkv [B, S, 3, H, D]`` (the QKV projection output
  viewed in place) -> ``o [B, S, H, D]``.  No transposes: the kernels read Q, K
  and V with strides and the backward writes one packed ``dqkv`` gradient.
* :func:`attention_gqa_packed` -- grouped-query attention on ``qkv [B, S, H +
  2 Hkv, D]``: heads ``[0, H)`` are Q, ``[H, H + Hkv)`` K and ``[H + Hkv, H + 2
  Hkv)`` V; query head ``h`` attends with K/V head ``h // (H / Hkv)``.  With
  ``Hkv == H`` this is ``attention_packed``'s layout byte for byte.  On the
  bf16 kernels the K/V heads are read in place (no repeated copy) and the
  backward sums each group's dK / dV partials in one extra kernel; everything
  else (fp32, the CPU, the padded shapes of ``_plan``) repeats the K/V heads
  into ``[B, S, 3, H, D]`` and runs as :func:`attention_packed`, autograd
  summing the group.
* :func:`attention` -- the usual ``q, k, v [B, H, S, D]`` API (views are
  permuted, not copied); ``k`` and ``v`` may have ``Hkv | H`` heads (repeated).

Causal masking and attention dropout are supported; the dropout mask is
regenerated from Philox (seed, offset) in backward, so checkpoint recompute
replays it exactly.  The kernels tile bf16 with ``S % 64 == 0`` and ``D in {64,
128, 256}`` (attention.hip) and fp32 with ``S % 32 == 0`` and ``D in {64, 128}``
(attention_f32.hip, the reference's own precision).  The CPU is the eager math
of :func:`attention_reference`.  On the GPU one function, :func:`_plan`, says
for every entry point and every option at which shape a call runs on the
kernels, or that it has no native form and runs the eager math as well (noted
once per shape); its docstring is the table.  It chooses among three ways to
fit a shape the kernels do not tile:

* Feature padding.  Any smaller head dim (e.g. 32, 80, 96, 160) is zero-padded
  to the next supported one: the padded features add 0 to every raw score (the
  scale stays that of the real head dim) and the padded columns are sliced off.
* Causal end padding.  A CAUSAL sequence of any other length (the reference's
  ``get_batch`` tail window) is zero-padded at the end to the next supported
  length: under the causal mask no real query sees a padded key, so the real
  rows are exact; the padded rows are sliced off (and get no gradient).
* A key mask or key bound.  A non-causal sequence of an unsupported length runs
  padded too: in bf16 when its head dim leaves a spare padded feature to mask
  the padded keys with (1 in every query, 0 in every real key, -32768 in every
  padded key, which then scores ``-32768 * scale`` and gets weight 0), in fp32
  with the kernels' own key bound (``kv_len``, so the reference's fp32 D=64 tail
  window runs on the kernels).

A window ``< S``, a soft cap, document bounds or sinks make a call generic: in
bf16 on the GPU it runs attention.hip's generic 64-row kernels, whatever S and D
(the S = 128, wide D = 64 and long-sequence kernels know none of the options);
grouped-query heads are read in place as without an option and the dropout mask
is the plain call's, restricted to the visible keys.  Feature padding and causal
end padding stay native (padded keys lie after every real query and padded
features add 0 to the raw score, before a cap); fp32, the CPU and the shapes
``_plan`` rejects use :func:`attention_reference` with the same options.  Every
entry point takes the options keyword-only, ``None`` being the code path it
always was:

Sliding-window attention, ``window=W`` (an int >= 1, with ``causal=True``): query
``i`` attends the ``W`` keys ``i - W < j <= i``, its own included -- the Hugging
Face / Mistral ``sliding_window`` convention (flash-attn's ``window_size=(W - 1,
0)``).  ``W >= S`` is plain causal attention, on the code path it always took.
The kernels skip the 64-key tiles wholly below the band as well as those above
the diagonal (about ``S * W`` work instead of ``S^2 / 2``).

Logit soft-capping, ``softcap=c`` (a finite number > 0): the scaled scores become
``c * tanh(s / c)`` before the masks and the softmax -- flash-attn's ``softcap``,
Gemma-2's ``attn_logit_softcapping`` -- non-causal, causal, or causal with a
window.  A non-causal sequence of an unsupported length is not native: the
spare-feature key mask scores a padded key at ``-32768 * scale`` and the cap
would bring that back to ``-c``.  The kernels take ``tanh`` as ``1 - 2 / (1 +
exp2(.))`` in fp32: its absolute error of about 2e-7 is an error of about ``c *
2e-7`` in the capped score, so it grows with ``c`` (nothing at 30 or 50; 1e-3 in
the exponent at 5000).

Document masks (packed sequences), ``doc_bounds`` -- int32 ``[B, 2, S]``, ``[b, 0,
i]`` the index of the first token of token ``i``'s document and ``[b, 1, i]`` one
past its last (``utils.data.document_bounds``), with ``causal=True``: query ``i``
attends key ``j`` iff ``start[i] <= j <= i`` (and ``j > i - W`` under a window,
which the kernels merge at run time).  They skip the key tiles before a query
tile's first document and the query tiles after a key tile's last one.  Under
causal end padding the pad tokens become one trailing document.  The contract on
the values (``start[i] <= i < end[i]``, both rows non-decreasing) is the caller's:
:func:`check_doc_bounds` validates it on the host, with a sync, and is never
called on the hot path; the kernels clamp the loop bounds they take from the
tensor.  :func:`use_documents` sets the bounds for the calling thread
(``AttentionCore`` reads them).

Attention sinks, ``sinks`` -- a ``[H]`` tensor, one learned logit per query head
(also under grouped-query attention), fp32 or the activations' dtype; ``-inf`` is
"no sink for this head".  The sink joins the softmax's normalisation after the
cap and the masks, neither scaled nor capped, and has no value vector: ``p_ij =
exp(s_ij - m) / (exp(sink_h - m) + sum_j exp(s_ij - m))`` -- Hugging Face
gpt-oss's ``softmax(cat([scores, sinks], -1))[..., :-1]``.  It works with
``causal=False`` too, and dropout acts on the real keys' ``p_ij`` only, with the
sinkless call's mask.  The sink is folded in once after the forward's key loop,
the three backward kernels are the sinkless ones reading the forward's ``lse``,
and ``dsinks[h] = -sum exp(sink_h - lse) * delta`` comes from one small
fixed-order reduction (the same bits on every run; it goes straight into the
parameter's fp32 ``main_grad`` where there is one).  Every padded shape stays
native, the non-causal key mask included (a padded key still underflows against
a running max the sink can only raise), unless there is a cap as well.
"""
from __future__ import annotations

import math
import os
import threading
from collections import OrderedDict
from contextlib import contextmanager
from typing import Optional, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor

from ..checkpoint import is_recomputing, recompute_expected
from ._util import kernels_for
from .linear import accumulable

__all__ = ["attention", "attention_packed", "attention_gqa_packed", "attention_reference", "clear_keep_words",
           "check_doc_bounds", "use_documents", "current_documents"]


def _check_window(window: Optional[int], causal: bool, S: int) -> Optional[int]:
    """``window`` validated (an int >= 1, causal only) and clamped: one that covers the sequence is ``None``."""
    if window is None:
        return None
    if isinstance(window, bool) or not isinstance(window, int):
        raise ValueError(f"attention: window must be an int >= 1 or None, got {window!r}")
    if window < 1:
        raise ValueError(f"attention: window must be >= 1 (None: no window), got {window}")
    if not causal:
        raise ValueError("attention: a sliding window needs causal=True (two-sided windows are not supported)")
    return None if window >= S else window


def _check_softcap(softcap: Optional[float]) -> Optional[float]:
    """``softcap`` validated: ``None`` (no cap) or a finite number > 0, returned as a float."""
    if softcap is None:
        return None
    if isinstance(softcap, bool) or not isinstance(softcap, (int, float)):
        raise ValueError(f"attention: softcap must be a finite number > 0 or None, got {softcap!r}")
    if not math.isfinite(softcap) or softcap <= 0:
        raise ValueError(f"attention: softcap must be finite and > 0 (None: no cap), got {softcap!r}")
    return float(softcap)


def _check_docs(doc_bounds: Optional[Tensor], causal: bool, B: int, S: int) -> Optional[Tensor]:
    """``doc_bounds`` validated by what the host knows without a sync: causal only, int32, ``[B, 2, S]``."""
    if doc_bounds is None:
        return None
    if not causal:
        raise ValueError("attention: doc_bounds needs causal=True (bidirectional document masks are not supported)")
    if not isinstance(doc_bounds, Tensor) or doc_bounds.dtype != torch.int32:
        raise ValueError("attention: doc_bounds must be an int32 tensor, got "
                         f"{getattr(doc_bounds, 'dtype', doc_bounds)!r}")
    if tuple(doc_bounds.shape) != (B, 2, S):
        raise ValueError(f"attention: doc_bounds must be [B, 2, S] = [{B}, 2, {S}], got {tuple(doc_bounds.shape)}")
    return doc_bounds


def _check_sinks(sinks: Optional[Tensor], H: int, dtype: torch.dtype) -> Optional[Tensor]:
    """``sinks`` validated: ``None`` (no sinks) or a ``[H]`` tensor, one logit per query head, in fp32 or the
    activations' dtype.  The values are free (``-inf``: no sink for that head)."""
    if sinks is None:
        return None
    if not isinstance(sinks, Tensor) or sinks.dim() != 1 or sinks.shape[0] != H:
        raise ValueError(f"attention: sinks must be a [H] = [{H}] tensor, one per query head, got "
                         f"{tuple(sinks.shape) if isinstance(sinks, Tensor) else sinks!r}")
    if sinks.dtype not in (torch.float32, dtype):
        raise ValueError(f"attention: sinks must be float32 or the activations' dtype ({dtype}), got {sinks.dtype}")
    return sinks


def check_doc_bounds(bounds: Tensor) -> None:
    """Validates a ``doc_bounds`` tensor's contract on the host: int32 ``[B, 2, S]``, ``start[i] <= i < end[i]
    <= S``, ``start >= 0`` and both rows non-decreasing.  It reads the values (a device sync): an explicit call
    for data pipelines and tests, never made by the ops."""
    if not isinstance(bounds, Tensor) or bounds.dtype != torch.int32 or bounds.dim() != 3 or bounds.shape[1] != 2:
        raise ValueError("check_doc_bounds: bounds must be an int32 tensor [B, 2, S]")
    S = bounds.shape[2]
    start, end = bounds[:, 0].long(), bounds[:, 1].long()
    idx = torch.arange(S, device=bounds.device)
    ok = (start >= 0) & (start <= idx) & (idx < end) & (end <= S)
    if not bool(ok.all()):
        raise ValueError("check_doc_bounds: need 0 <= start[i] <= i < end[i] <= S for every token")
    if S > 1 and not bool(((start[:, 1:] >= start[:, :-1]) & (end[:, 1:] >= end[:, :-1])).all()):
        raise ValueError("check_doc_bounds: start and end must be non-decreasing along a row")
    # constant on a document: every token of [start[i], end[i]) carries the same pair
    if not bool(((start.gather(1, end - 1) == start) & (end.gather(1, start) == end)).all()):
        raise ValueError("check_doc_bounds: start and end must be constant on a document")


_documents = threading.local()


def current_documents() -> Optional[Tensor]:
    """The ``doc_bounds`` :func:`use_documents` set for the calling thread, or None."""
    return getattr(_documents, "bounds", None)


@contextmanager
def use_documents(bounds: Optional[Tensor]):
    """Sets ``bounds`` (int32 ``[B, 2, S]``, or None) as the calling thread's document bounds for the block:
    every causal ``AttentionCore`` that runs inside passes them to its attention op.  Thread-local, so worker
    threads started inside do not see it."""
    prev = current_documents()
    _documents.bounds = bounds
    try:
        yield bounds
    finally:
        _documents.bounds = prev


def attention_reference(q: Tensor, k: Tensor, v: Tensor, causal: bool, p: float, scale: Optional[float] = None,
                        *, window: Optional[int] = None, softcap: Optional[float] = None,
                        doc_bounds: Optional[Tensor] = None, sinks: Optional[Tensor] = None) -> Tensor:
    """Eager fp32 math on ``[B, H, S, D]`` (CPU path and test oracle).  ``window``: query ``i`` sees the keys
    ``i - window < j <= i`` only.  ``softcap``: the scaled scores become ``softcap * tanh(s / softcap)`` before
    the masks.  ``doc_bounds`` (int32 ``[B, 2, S]``): query ``i`` sees the keys ``j >= doc_bounds[b, 0, i]``
    only.  ``sinks`` (``[H]``): one more logit per query head in the softmax's denominator, with no value (the
    module doc); the math then runs in fp64 for fp64 inputs."""
    d = q.shape[-1]
    scale = scale if scale is not None else 1.0 / math.sqrt(d)
    window = _check_window(window, bool(causal), q.shape[-2])
    softcap = _check_softcap(softcap)
    docs = _check_docs(doc_bounds, bool(causal), q.shape[0], q.shape[-2])
    sinks = _check_sinks(sinks, q.shape[1], q.dtype)
    wide = torch.float32 if sinks is None else torch.promote_types(q.dtype, torch.float32)
    s = torch.matmul(q.to(wide), k.to(wide).transpose(-1, -2)) * scale
    if softcap is not None:
        s = softcap * torch.tanh(s / softcap)
    if causal:
        n, m = s.shape[-2], s.shape[-1]
        mask = torch.ones(n, m, dtype=torch.bool, device=s.device).triu(1 + m - n)
        if window is not None:  # keys at or below the band's lower edge: j <= i - window
            mask |= torch.ones(n, m, dtype=torch.bool, device=s.device).tril(m - n - window)
        s = s.masked_fill(mask, float("-inf"))
        if docs is not None:  # keys before the query's document: j < start[b, i]
            start = docs[:, 0].to(s.device)
            keys = torch.arange(m, device=s.device)
            s = s.masked_fill((keys[None, None, :] < start[:, :, None])[:, None], float("-inf"))
    pr = torch.softmax(s, dim=-1)
    if sinks is not None:
        # softmax(cat(s, sink))[..., :-1] = softmax(s) * den / (den + exp(sink)), den = sum_j exp(s_j): the factor
        # is sigmoid(lse(s) - sink), exactly 1 at sink = -inf (the sinkless bits) and finite for any sink
        sk = sinks.to(device=s.device, dtype=wide).view(1, -1, 1, 1)
        pr = pr * torch.sigmoid(torch.logsumexp(s, dim=-1, keepdim=True) - sk)
    if p > 0:
        pr = F.dropout(pr, p, True)
    return torch.matmul(pr, v.to(wide)).to(q.dtype)


# Keep words across a checkpoint: the long-sequence forward (attention_long.hip) makes its dropout keep words
# inside the kernel (Philox in the loop: ~1.6x the forward's VALU work) and returns them for the backward.  A
# checkpoint's first, no-grad forward throws them away and its recompute makes the same words again from the
# same restored Philox draw.  Instead the first forward leaves them here, keyed by (device, seed, offset), and
# the recompute -- whose draw is that key again -- reads them (the kernel variant that loads the words).  The
# words are bit-identical either way (tests/test_gpu_kernels.py::test_attention_keep_words_reused_bit_exact).
# Bounded: at most MIPIPE_ATTN_KEEP_REUSE_GB (default 16) are held, oldest dropped first (a dropped entry is just
# made again), and only when that recompute will run (checkpoint.recompute_expected(): not for a training-mode
# forward under no_grad); MIPIPE_ATTN_KEEP_REUSE=0 turns it off.
_KEEP_REUSE = os.environ.get("MIPIPE_ATTN_KEEP_REUSE", "1") != "0"
_KEEP_LIMIT = int(float(os.environ.get("MIPIPE_ATTN_KEEP_REUSE_GB", "16")) * (1 << 30))
_keep_words: "OrderedDict[tuple, Tensor]" = OrderedDict()
_keep_bytes = 0
_keep_lock = threading.Lock()
keep_stats = {"stored": 0, "reused": 0}  # counters, for the tests


def _i64(x: int) -> int:
    return x - (1 << 64) if x >= (1 << 63) else x


def _next_draw(device: torch.device) -> tuple:
    """(device, seed, offset) the next Philox draw on ``device`` will return (the binding's int64 view)."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    g = torch.cuda.default_generators[idx]
    return (idx, _i64(g.initial_seed()), g.get_offset())


def clear_keep_words() -> None:
    """Drops every held keep-word set (the engine calls it at the end of a step)."""
    global _keep_bytes
    with _keep_lock:
        _keep_words.clear()
        _keep_bytes = 0


def _attention_fwd(kern, q, k, v, causal, p, scale, kv_len, window=0, softcap=0.0, docs=None, sinks=None):
    global _keep_bytes
    if window or softcap or docs is not None or sinks is not None:
        # the generic kernels: the mask is regenerated from Philox, there are no keep words
        return kern.attention_fwd(q, k, v, causal, p, scale, kv_len, window=window, softcap=softcap, doc_bounds=docs,
                                  sinks=sinks)
    reuse = _KEEP_REUSE and p > 0 and q.is_cuda and q.dtype == torch.bfloat16 and kv_len == 0
    words = key = None
    if reuse and is_recomputing():
        key = _next_draw(q.device)
        with _keep_lock:
            words = _keep_words.pop(key, None)
            if words is not None:
                _keep_bytes -= words.numel() * 4
                keep_stats["reused"] += 1
    if words is not None:
        out = kern.attention_fwd(q, k, v, causal, p, scale, kv_len, words, key[1], key[2])
    else:
        out = kern.attention_fwd(q, k, v, causal, p, scale, kv_len)
    bits = out[4]
    if reuse and bits.numel() and recompute_expected() and not torch.is_grad_enabled():
        idx = q.device.index if q.device.index is not None else torch.cuda.current_device()
        with _keep_lock:
            _keep_words[(idx, out[2], out[3])] = bits
            _keep_bytes += bits.numel() * 4
            keep_stats["stored"] += 1
            while _keep_bytes > _KEEP_LIMIT and _keep_words:
                _, old = _keep_words.popitem(last=False)
                _keep_bytes -= old.numel() * 4
    return out


def _kernel_sinks(sinks: Optional[Tensor]) -> Optional[Tensor]:
    """``sinks`` as the kernels read them: fp32, contiguous, detached (the same tensor where it already is)."""
    return None if sinks is None else sinks.detach().float().contiguous()


def _dsinks_out(sinks: Optional[Tensor], sk: Optional[Tensor], needed: bool):
    """``(dsinks, accumulate)`` for ``attention_bwd``: the parameter's fp32 ``main_grad`` to add into where it has
    one, a fresh fp32 ``[H]`` to store into otherwise, ``(None, False)`` where no gradient is asked for."""
    if sinks is None or not needed:
        return None, False
    main = getattr(sinks, "main_grad", None)
    if main is not None and main.dtype == torch.float32 and main.is_contiguous() and main.device == sk.device:
        return accumulable(sinks), True  # claimed (and zero-filled if it was lazily zeroed) only once it is usable
    return torch.empty_like(sk), False


def _dsinks_grad(sinks: Optional[Tensor], ds: Optional[Tensor], accumulated: bool) -> Optional[Tensor]:
    return None if ds is None or accumulated else ds.to(sinks.dtype)


def _forward(ctx, inputs, q, k, v, causal, p, scale, kv_len, window, softcap, docs, sinks):
    """The Functions' forward: runs the kernel on the views ``q, k, v`` of ``inputs``, saves ``inputs`` with the
    results and stashes the scalars."""
    sk = _kernel_sinks(sinks)
    o, lse, seed, offset, bits = _attention_fwd(kernels_for(q), q, k, v, causal, p, scale, kv_len, window, softcap,
                                                docs, sk)
    ctx.save_for_backward(*inputs, o, lse, bits, docs, sinks, sk)
    ctx.scalars = (causal, p, scale, seed, offset, kv_len, window, softcap)
    return o


def _backward(ctx, do, views):
    """The Functions' backward: one gradient buffer per saved input, of which ``views`` gives the q, k, v views as
    it does of the inputs.  Returns the buffers and the sinks' gradient (``sinks`` is each forward's last
    argument)."""
    *inputs, o, lse, bits, docs, sinks, sk = ctx.saved_tensors
    causal, p, scale, seed, offset, kv_len, window, softcap = ctx.scalars
    if do.stride() != o.stride():
        do = do.contiguous()
    grads = [torch.empty_like(t) for t in inputs]
    ds, acc = _dsinks_out(sinks, sk, sinks is not None and ctx.needs_input_grad[-1])
    kernels_for(do).attention_bwd(do, *views(*inputs), o, lse, causal, p, scale, seed, offset, *views(*grads),
                                  bits if bits.numel() else None, kv_len, window, softcap, docs, sk, ds, acc)
    return grads, _dsinks_grad(sinks, ds, acc)


def _heads(qkv: Tensor, n_kv: int) -> Tuple[Tensor, Tensor, Tensor]:
    """The Q, K and V head slices of a packed ``[B, S, H + 2 Hkv, D]``."""
    H = qkv.shape[2] - 2 * n_kv
    return qkv.narrow(2, 0, H), qkv.narrow(2, H, n_kv), qkv.narrow(2, H + n_kv, n_kv)


class _AttentionPacked(torch.autograd.Function):
    """``qkv [B, S, H + 2 Hkv, D]`` (contiguous) in, ``o [B, S, H, D]`` out.  Q, K and V are head slices of the
    one buffer (same strides, fewer K/V heads when ``n_kv < H``: bf16 only); ``[B, S, 3, H, D]`` is the same bytes
    with ``n_kv = H``.  The backward writes dQ and the group-summed dK / dV into one packed ``dqkv`` of the same
    layout (the binding owns the per-query-head scratch)."""

    @staticmethod
    def forward(ctx, qkv, n_kv, causal, p, scale, kv_len=0, window=0, softcap=0.0,  # type: ignore[override]
                docs=None, sinks=None):
        ctx.n_kv = n_kv
        return _forward(ctx, (qkv,), *_heads(qkv, n_kv), causal, p, scale, kv_len, window, softcap, docs, sinks)

    @staticmethod
    def backward(ctx, do):  # type: ignore[override]
        (dqkv,), dsinks = _backward(ctx, do, lambda t: _heads(t, ctx.n_kv))
        return dqkv, None, None, None, None, None, None, None, None, dsinks


class _Attention(torch.autograd.Function):
    """Separate q, k, v as [B, S, H, D] views sharing one layout."""

    @staticmethod
    def forward(ctx, q, k, v, causal, p, scale, kv_len=0, window=0, softcap=0.0, docs=None,  # type: ignore[override]
                sinks=None):
        return _forward(ctx, (q, k, v), q, k, v, causal, p, scale, kv_len, window, softcap, docs, sinks)

    @staticmethod
    def backward(ctx, do):  # type: ignore[override]
        (dq, dk, dv), dsinks = _backward(ctx, do, lambda q, k, v: (q, k, v))
        return dq, dk, dv, None, None, None, None, None, None, None, dsinks


_noted = set()


def _note_math_path(S: int, D: int, dtype, window: Optional[int] = None, softcap: Optional[float] = None,
                    docs: bool = False, sinks: bool = False, stacklevel: int = 3) -> None:
    """Shapes outside the kernels' tiling use the eager math path; say so once per shape."""
    # (set, key tag, the call's words, the warning's tail) per option, in the key's order
    notes = [
        (window is not None, "window", f" window={window}",
         ".  fp32 sliding-window attention is not native: the window runs on the bf16 kernels only"),
        (softcap is not None, "softcap", f" softcap={softcap}",
         ".  Soft-capped attention is native in bf16 only, and not for a non-causal sequence of an unsupported "
         "length"),
        (docs, "documents", " doc_bounds", ".  Document-masked attention is native in bf16 only"),
        (sinks, "sinks", " sinks", ".  Attention with sinks is native in bf16 only"),
    ]
    notes = [n for n in notes if n[0]]
    key = (S, D, dtype) + tuple(n[1] for n in notes)
    if key not in _noted:
        _noted.add(key)
        import warnings

        extra, tail = "".join(n[2] for n in notes), "".join(n[3] for n in notes)
        warnings.warn(f"mipipe attention: S={S} D={D} {dtype}{extra} runs the eager math path (HIP kernels: bf16 "
                      "with S % 64 == 0, D in {64, 128, 256}; fp32 with S % 32 == 0, D in {64, 128})" + tail,
                      stacklevel=stacklevel)


def _gpu_ok(dtype: torch.dtype, S: int, D: int) -> bool:
    """The kernels tile (S, D) in ``dtype`` as it is: the one place the plan asks the extension."""
    if dtype == torch.bfloat16:
        return kernels_for().attention_supported(S, D)
    if dtype == torch.float32:
        return kernels_for().attention_f32_supported(S, D)
    return False


def _causal_pad(dtype: torch.dtype, S: int, D: int) -> Optional[int]:
    """The padded length a causal sequence of S runs at on the kernels (None: none fits)."""
    step = 64 if dtype == torch.bfloat16 else 32
    for sp in (-(-S // step) * step, max(128, -(-S // step) * step)):
        if sp != S and _gpu_ok(dtype, sp, D):
            return sp
    return None


_KEY_MASK = -32768.0  # exact in bf16; times the query's 1 and any scale >= 2^-8: exp underflows to 0


def _plan(dtype: torch.dtype, S: int, D: int, causal: bool, scale: float, *, generic: bool,
          softcap: Optional[float], sinks: bool) -> Optional[Tuple[int, int, int, bool]]:
    """``(sp, dp, kv_len, key_mask)`` a GPU call of (S, D) runs at on the kernels, or None (the eager path).
    ``generic``: the call has a window ``< S``, a cap, document bounds or sinks.  ``sp`` / ``dp`` are the padded
    sequence length and head dim, ``kv_len`` (0 = none) the key bound the fp32 kernels mask past themselves, and
    ``key_mask`` says that the caller masks the padded keys through the spare feature ``D`` (the module doc).

    ====================  ===========================================================================
    call                  runs at
    ====================  ===========================================================================
    any, (S, D) tiled     ``(S, D)`` as it is (generic: bf16 only)
    plain                 the first ``dp`` in ``D`` and the supported head dims above it with: ``S``
                          tiled -> ``(S, dp)``; fp32 non-causal -> end padding with ``kv_len = S``;
                          causal -> end padding; bf16 non-causal with ``dp > D`` and ``scale >= 2^-8``
                          (``exp(-32768 * scale)`` must underflow to 0) -> end padding with the key
                          mask.  End padding is to the next multiple of 64 (fp32: 32), or 128.
    generic               bf16 only; the plain answer unless it needs the key mask (a cap would bring
                          a masked key's score back to ``-softcap``; a window and document bounds are
                          causal anyway)
    generic with sinks    bf16 only; the plain answer, the key mask included unless there is a cap
                          (the sink only raises the row's running max, so a masked key underflows as
                          it does without one)
    ====================  ===========================================================================
    """
    bf16 = dtype == torch.bfloat16
    if generic and not bf16:
        return None
    if _gpu_ok(dtype, S, D):
        return S, D, 0, False
    for dp in [D] + [d for d in ((64, 128, 256) if bf16 else (64, 128)) if d > D]:
        if _gpu_ok(dtype, S, dp):
            return S, dp, 0, False
        if dtype == torch.float32 and not causal:  # key bound inside the kernel
            sp = _causal_pad(dtype, S, dp)
            if sp is not None:
                return sp, dp, S, False
        elif causal or (dp > D and scale >= 2.0 ** -8):
            sp = _causal_pad(dtype, S, dp)
            if sp is not None:
                if not causal and generic and not (sinks and softcap is None):
                    return None
                return sp, dp, 0, not causal
    return None


def _pad_docs(docs: Tensor, S: int, sp: int) -> Tensor:
    """``docs [B, 2, S]`` for a sequence end-padded to ``sp``: the pad tokens ``[S, sp)`` are one trailing
    document (no real query sees them under the causal mask anyway).  Tensor ops only, no sync."""
    if sp == S:
        return docs.contiguous()
    out = docs.new_empty(docs.shape[0], 2, sp)
    out[:, :, :S] = docs
    out[:, 0, S:] = S
    out[:, 1, S:] = sp
    return out


def _run_padded(run, ts, seq: int, heads: int, S: int, D: int, sp: int, dp: int, key_mask) -> Tensor:
    """``run(*ts)`` with every tensor of ``ts`` zero-padded to ``sp`` along axis ``seq`` and to ``dp`` along the
    last, and the result (same axes) sliced back to ``S`` and ``D``.  ``key_mask``, where the plan asks for one:
    ``((i, h), (j, g))`` -- the queries are the heads ``h`` (a slice of axis ``heads``) of ``ts[i]``, the keys the
    heads ``g`` of ``ts[j]`` -- sets the spare feature ``D`` to 1 in every query and to -32768 in every padded key."""
    if (sp, dp) == (S, D):
        return run(*ts)
    ts = [F.pad(t, (0, dp - D) + (0, 0) * (t.dim() - 2 - seq) + (0, sp - S)) for t in ts]
    if key_mask:
        (qi, qh), (ki, kh) = key_mask
        marks = {i: torch.zeros_like(ts[i]) for i in (qi, ki)}
        at = [slice(None)] * ts[qi].dim()
        at[heads], at[-1] = qh, D
        marks[qi][tuple(at)] = 1.0
        at[heads], at[seq] = kh, slice(S, None)
        marks[ki][tuple(at)] = _KEY_MASK
        for i, c in marks.items():
            ts[i] = ts[i] + c
    cut = [slice(None)] * 4
    cut[seq], cut[-1] = slice(0, S), slice(0, D)
    return run(*ts)[tuple(cut)]


def _is_generic(window, softcap, docs, sinks) -> bool:
    return window is not None or softcap is not None or docs is not None or sinks is not None


def _packed(qkv: Tensor, n_kv: int, causal: bool, p: float, scale: float, window: Optional[int],
            softcap: Optional[float], docs: Optional[Tensor], sinks: Optional[Tensor]) -> Tensor:
    """The packed entry points after validation: ``qkv [B, S, H + 2 n_kv, D]`` -> ``o [B, S, H, D]``.  With
    ``n_kv < H`` the caller has made sure the shape runs as it is."""
    B, S, heads, D = qkv.shape
    H = heads - 2 * n_kv
    plan = _plan(qkv.dtype, S, D, causal, scale, generic=_is_generic(window, softcap, docs, sinks), softcap=softcap,
                 sinks=sinks is not None) if qkv.is_cuda else None
    if plan is None:
        if qkv.is_cuda:
            _note_math_path(S, D, qkv.dtype, window, softcap, docs is not None, sinks is not None, stacklevel=4)
        q, k, v = (t.transpose(1, 2) for t in _heads(qkv, n_kv))
        o = attention_reference(q, k, v, causal, p, scale, window=window, softcap=softcap, doc_bounds=docs,
                                sinks=sinks)
        return o.transpose(1, 2)
    sp, dp, kv_len, key_mask = plan
    if docs is not None:
        docs = _pad_docs(docs.to(qkv.device), S, sp)
    return _run_padded(lambda t: _AttentionPacked.apply(t.contiguous(), n_kv, causal, p, scale, kv_len, window or 0,
                                                        softcap or 0.0, docs, sinks),
                       (qkv,), 1, 2, S, D, sp, dp, ((0, slice(0, H)), (0, slice(H, H + n_kv))) if key_mask else None)


def attention_packed(qkv: Tensor, causal: bool = False, dropout_p: float = 0.0, training: bool = True,
                     scale: Optional[float] = None, *, window: Optional[int] = None,
                     softcap: Optional[float] = None, doc_bounds: Optional[Tensor] = None,
                     sinks: Optional[Tensor] = None) -> Tensor:
    """``qkv [B, S, 3, H, D]`` -> ``o [B, S, H, D]``.  ``window``: sliding-window attention, ``softcap``: logit
    soft-capping, ``doc_bounds``: document masks, ``sinks``: attention sinks (module doc)."""
    B, S, three, H, D = qkv.shape
    assert three == 3
    causal = bool(causal)
    p = float(dropout_p) if training else 0.0
    scale = float(scale) if scale is not None else 1.0 / math.sqrt(D)
    window = _check_window(window, causal, S)
    softcap = _check_softcap(softcap)
    docs = _check_docs(doc_bounds, causal, B, S)
    sinks = _check_sinks(sinks, H, qkv.dtype)
    return _packed(qkv.reshape(B, S, 3 * H, D), H, causal, p, scale, window, softcap, docs, sinks)


def _expand_kv(qkv: Tensor, n_kv: int) -> Tensor:
    """``[B, S, H + 2 Hkv, D]`` -> ``[B, S, 3 H, D]`` with every K/V head repeated over its group
    (differentiable: the backward sums the group)."""
    q, k, v = _heads(qkv, n_kv)
    g = q.shape[2] // n_kv
    return torch.cat((q, k.repeat_interleave(g, dim=2), v.repeat_interleave(g, dim=2)), dim=2)


def attention_gqa_packed(qkv: Tensor, n_kv_heads: int, causal: bool = False, dropout_p: float = 0.0,
                         training: bool = True, scale: Optional[float] = None, *,
                         window: Optional[int] = None, softcap: Optional[float] = None,
                         doc_bounds: Optional[Tensor] = None, sinks: Optional[Tensor] = None) -> Tensor:
    """``qkv [B, S, H + 2 Hkv, D]`` -> ``o [B, S, H, D]`` (grouped-query attention, ``Hkv = n_kv_heads``).
    ``window``: sliding-window attention, ``softcap``: logit soft-capping, ``doc_bounds``: document masks,
    ``sinks``: attention sinks, one per QUERY head (module doc)."""
    if qkv.dim() != 4:
        raise ValueError(f"attention_gqa_packed: qkv must be [B, S, H + 2 Hkv, D], got {tuple(qkv.shape)}")
    B, S, heads, D = qkv.shape
    n_kv = int(n_kv_heads)
    H = heads - 2 * n_kv
    if n_kv <= 0 or H <= 0 or H % n_kv != 0:
        raise ValueError(f"attention_gqa_packed: {heads} packed heads do not split into H + 2 * {n_kv} with "
                         f"{n_kv} dividing H")
    causal = bool(causal)
    p = float(dropout_p) if training else 0.0
    scale = float(scale) if scale is not None else 1.0 / math.sqrt(D)
    window = _check_window(window, causal, S)
    softcap = _check_softcap(softcap)
    docs = _check_docs(doc_bounds, causal, B, S)
    sinks = _check_sinks(sinks, H, qkv.dtype)
    # Hkv == H is plain multi-head attention, the same bytes as [B, S, 3, H, D]; fewer K/V heads are read in place
    # by the bf16 kernels at a shape they tile as it is, and repeated otherwise (sinks are per query head already)
    if n_kv != H and not (qkv.is_cuda and qkv.dtype == torch.bfloat16 and _gpu_ok(qkv.dtype, S, D)):
        qkv, n_kv = _expand_kv(qkv, n_kv), H
    return _packed(qkv, n_kv, causal, p, scale, window, softcap, docs, sinks)


def attention(
    q: Tensor, k: Tensor, v: Tensor, causal: bool = False, dropout_p: float = 0.0, training: bool = True,
    scale: Optional[float] = None, *, window: Optional[int] = None, softcap: Optional[float] = None,
    doc_bounds: Optional[Tensor] = None, sinks: Optional[Tensor] = None,
) -> Tensor:
    """``q, k, v [B, H, S, D]`` -> ``[B, H, S, D]``.  ``k`` and ``v`` may have fewer heads, ``Hkv | H``
    (grouped-query attention): separate tensors do not share q's strides, so their heads are repeated
    (autograd sums each group's gradient).  ``window``: sliding-window attention, ``softcap``: logit
    soft-capping, ``doc_bounds``: document masks, ``sinks``: attention sinks (module doc)."""
    if k.shape[1] != q.shape[1]:
        if k.shape[1] != v.shape[1] or k.shape[1] <= 0 or q.shape[1] % k.shape[1] != 0:
            raise ValueError(f"attention: {k.shape[1]} / {v.shape[1]} K/V heads do not divide {q.shape[1]} query heads")
        g = q.shape[1] // k.shape[1]
        k, v = k.repeat_interleave(g, dim=1), v.repeat_interleave(g, dim=1)
    B, _, S, D = q.shape
    causal = bool(causal)
    p = float(dropout_p) if training else 0.0
    scale = float(scale) if scale is not None else 1.0 / math.sqrt(D)
    window = _check_window(window, causal, S)
    softcap = _check_softcap(softcap)
    docs = _check_docs(doc_bounds, causal, B, S)
    sinks = _check_sinks(sinks, q.shape[1], q.dtype)
    plan = _plan(q.dtype, S, D, causal, scale, generic=_is_generic(window, softcap, docs, sinks), softcap=softcap,
                 sinks=sinks is not None) if q.is_cuda else None
    if plan is None:
        if q.is_cuda:
            _note_math_path(S, D, q.dtype, window, softcap, docs is not None, sinks is not None)
        return attention_reference(q, k, v, causal, p, scale, window=window, softcap=softcap, doc_bounds=docs,
                                   sinks=sinks)
    sp, dp, kv_len, key_mask = plan
    if docs is not None:
        docs = _pad_docs(docs.to(q.device), S, sp)

    def run(q, k, v):
        qs, ks, vs = (t.transpose(1, 2) for t in (q, k, v))
        # (the fp32 key-bound path has always run on contiguous copies)
        if kv_len or not (qs.stride() == ks.stride() == vs.stride()) or qs.stride(3) != 1:
            qs, ks, vs = (t.contiguous() for t in (qs, ks, vs))
        o = _Attention.apply(qs, ks, vs, causal, p, scale, kv_len, window or 0, softcap or 0.0, docs, sinks)
        return o.transpose(1, 2)

    return _run_padded(run, (q, k, v), 2, 1, S, D, sp, dp, ((0, slice(None)), (1, slice(None))) if key_mask else None)
