"""Transformer blocks on the mipipe HIP ops (SURVEY §7.1 'Models').

A :class:`TransformerEncoderLayer` is the drop-in equivalent of
``nn.TransformerEncoderLayer`` as the reference driver uses it
(``/root/reference/main.py:115-120,139-157``: post-norm, ReLU, dropout, no
mask), but batch-first ``[B, S, E]`` and built from two *pipeline-splittable*
halves, each a single-tensor module:

* :class:`SelfAttentionBlock` -- ``LN1(x + drop(out_proj(attn(qkv(x)))))``
  (pre-norm: ``x + drop(out_proj(attn(qkv(LN1(x)))))``);
* :class:`FeedForwardBlock`   -- ``LN2(x + drop(W2 drop(act(W1 x))))``.

Splitting at sub-layer granularity lets the balancer put stage boundaries
between the attention and MLP halves, which matters when 12 layers are spread
over 8 MI355X stages.

Hot path per block: MFMA GEMMs with fused bias/activation/dropout epilogues,
flash attention, fused dropout+residual+LayerNorm -- see ``mipipe.ops``.
``from_torch`` copies weights from an ``nn.TransformerEncoderLayer`` so the
blocks can be checked against PyTorch.

Keyword options turn the same halves into a LLaMA-style block (all default to
the behaviour above): ``norm="rms"`` (RMSNorm, no norm bias), ``bias=False`` (no
bias parameters; the linears get ``None``), ``rope=True`` (rotary positions on
Q and K) and ``activation="swiglu"`` (``linear1_weight`` is ``[2F, E]``: rows
``[0, F)`` the gate projection, rows ``[F, 2F)`` the up projection; the halves
still exchange an ``F``-wide ``h``).  ``n_kv_heads=Hkv`` (a divisor of ``nhead``;
``None`` means ``nhead``) is grouped-query attention: ``in_proj_weight`` is
``[(H + 2 Hkv) D, E]`` -- rows of the ``H`` Q heads, then of the ``Hkv`` K heads,
then of the ``Hkv`` V heads -- and query head ``h`` attends with K/V head
``h // (H / Hkv)`` (``ops.attention_gqa_packed``).  ``window=W`` (causal blocks
only; ``None`` means none) is sliding-window attention: a query attends the
last ``W`` keys, its own included (Mistral's ``sliding_window``).
``attn_softcap=c`` (``None`` means none) caps the attention scores at ``c *
tanh(s / c)`` before the softmax (Gemma-2's ``attn_logit_softcapping``).
``qk_norm=True`` (Qwen3) RMS-normalises every Q head and every K head over its
``D`` features before the rotation, with the learned ``[D]`` weights
``q_norm_weight`` and ``k_norm_weight`` of the attention core and the block's
``layer_norm_eps`` (``ops.qk_norm_rope_projection``: one kernel with the
rotation, or the norm alone with ``rope=False``).  ``attn_sinks=True`` (gpt-oss)
gives the attention core ``sinks``, a learned ``[nhead]`` parameter (zeros at
initialisation): one logit per query head that joins the softmax's denominator
and has no value (``ops.attention``'s ``sinks=``).

Four more options make the halves a Gemma-2 block.  ``activation="geglu"`` is
``"swiglu"`` with the tanh-GELU as the gate (``ops.geglu``; the same ``[2F, E]``
weight, gate rows first).  ``sandwich_norm=True`` (pre-norm RMSNorm blocks
without residual dropout only) normalises each branch again before the residual
add: the output halves compute ``x + RMSNorm(W o + b) * post_norm_weight``
(``ops.rms_norm_residual``) with a ``[E]`` weight of their own, so their GEMM
runs as a plain ``ops.linear`` instead of with the add in its epilogue.
``head_dim=D`` (``None`` means ``d_model // nhead``) gives the heads a width of
their own: with ``A = nhead * D`` the QKV projection is ``[(H + 2 Hkv) D, E]``,
the core returns ``o [B, S, A]`` and ``out_proj_weight`` is ``[E, A]``; a packed
core whose ``A != E`` hands ``x`` and ``o`` on block-concatenated as ``[.., E +
A]``.  ``attn_scale`` (``None`` means ``1 / sqrt(D)``) is the score scale
(Gemma-2's ``query_pre_attn_scalar ** -0.5``).  ``transformer_blocks`` also takes
``global_every=n``: layer ``i`` with ``(i + 1) % n == 0`` is a global layer, built
without the window.

``transformer_blocks(..., n_experts=Ne)`` replaces every layer's MLP with a
:class:`MoEFeedForwardBlock` (Mixtral, Qwen3-MoE): ``Ne`` gated experts, a top-k
softmax router with a fixed capacity per expert (``ops.moe_route`` /
``moe_assign`` / ``moe_dispatch`` / ``moe_combine``) and a load-balancing term
that reaches the router through its backward.
"""
from __future__ import annotations

import math
import os
from typing import List, Optional

import torch
from torch import Tensor, nn

from .. import ops
from ..ops.linear import ActFold, mark_gemm_weight

# Fan-out fusion of the residual-branch gradient (see AttentionCore.forward_fanout);
# MIPIPE_FANOUT=0 turns it off (A/B measurements).
FANOUT = os.environ.get("MIPIPE_FANOUT", "1") != "0"
# MLP activation backward in fc_out's dgrad epilogue (ops.linear.ActFold), for
# the activations in FOLD_ACTS.  ReLU's backward is a sign test on the saved
# output, nearly free in the epilogue (enc12 FFN dgrad + act backward 240 -> 222
# us).  GELU's is one multiply as well when its forward saves GELU'(pre)
# (ops.linear MIPIPE_GELU_SAVE_GRAD=1, not the default); with pre saved, the
# erf/exp per element made the epilogue slower than the separate memory-bound
# kernel (GPT-2-XL fc2 dgrad 244 -> 251 us; tools/gemm_dact_probe.py), so GELU
# is then not folded.  MIPIPE_FOLD_ACT=0: off, =relu: ReLU only, =all: both.
_FOLD_ENV = os.environ.get("MIPIPE_FOLD_ACT", "auto")
if _FOLD_ENV == "auto":
    _FOLD_ENV = "all" if os.environ.get("MIPIPE_GELU_SAVE_GRAD", "0") == "1" else "relu"
FOLD_ACTS = () if _FOLD_ENV == "0" else (("relu", "gelu") if _FOLD_ENV == "all" else ("relu",))


def _folds(fc_in, training: bool) -> bool:
    """Fold fc_in's activation backward into fc_out's dgrad?  GELU only without
    dropout after it: the GEMM epilogue would regenerate the mask with Philox per
    element, which cost more than the separate pass saves (GPT-2-XL PP=1, p =
    0.1: 62.3k vs 62.9k tok/s) -- ReLU's saved output carries its mask."""
    act = fc_in.activation
    if act not in FOLD_ACTS:
        return False
    return act != "gelu" or not (training and fc_in.dropout > 0.0)


NORMS = ("layer", "rms")
GATED_ACTS = ("swiglu", "geglu")  # linear1 is [2F, E], gate rows first; the gate is a kernel of its own


def _check_sandwich(sandwich_norm: bool, norm_first: bool, norm: str, dropout: float) -> bool:
    if sandwich_norm and not (norm_first and norm == "rms" and dropout == 0.0):
        raise ValueError("sandwich_norm needs norm_first=True, norm='rms' and a residual dropout of 0, got "
                         f"norm_first={norm_first}, norm={norm!r}, dropout={dropout}")
    return bool(sandwich_norm)


def _init_norm(mod: nn.Module, d_model: int, norm: str, fk: dict) -> None:
    """``mod.norm_weight`` (and ``mod.norm_bias`` for LayerNorm: RMSNorm has none)."""
    if norm not in NORMS:
        raise ValueError(f"norm must be one of {NORMS}, got {norm!r}")
    mod.norm_weight = nn.Parameter(torch.empty(d_model, **fk))
    if norm == "layer":
        mod.norm_bias = nn.Parameter(torch.empty(d_model, **fk))


def _reset_norm(mod: nn.Module) -> None:
    nn.init.ones_(mod.norm_weight)
    if mod.norm == "layer":
        nn.init.zeros_(mod.norm_bias)


def _norm(mod: nn.Module, x: Tensor, residual: Optional[Tensor], p: float) -> Tensor:
    """``norm(residual + dropout(x, p))`` with ``mod``'s norm kind and parameters."""
    if mod.norm == "rms":
        return ops.add_dropout_rms_norm(x, residual, mod.norm_weight, mod.eps, p, mod.training)
    return ops.add_dropout_layer_norm(x, residual, mod.norm_weight, mod.norm_bias, mod.eps, p, mod.training)


def _norm_fanout(mod: nn.Module, x: Tensor):
    if mod.norm == "rms":
        return ops.rms_norm_fanout(x, mod.norm_weight, mod.eps)
    return ops.layer_norm_fanout(x, mod.norm_weight, mod.norm_bias, mod.eps)


__all__ = [
    "AttentionCore",
    "AttentionOutput",
    "PackedAttentionCore",
    "PackedAttentionOutput",
    "SelfAttentionBlock",
    "FeedForwardBlock",
    "MoEFeedForwardBlock",
    "FeedForwardIn",
    "FeedForwardOut",
    "PackedFeedForwardIn",
    "PackedFeedForwardOut",
    "TransformerEncoderLayer",
    "transformer_blocks",
    "layer_window",
    "block_flops",
]


class AttentionCore(nn.Module):
    """QKV projection + scaled-dot-product attention (pre-norm: LN first).

    ``x [B, S, E] -> o [B, S, A]`` (attention output before ``out_proj``), ``A = nhead * head_dim``
    (``E`` unless ``head_dim`` is given).
    """

    def __init__(self, d_model: int, nhead: int, dropout: float, *, norm_first: bool, causal: bool,
                 layer_norm_eps: float, norm: str = "layer", bias: bool = True, rope: bool = False,
                 rope_base: float = 10000.0, n_kv_heads: Optional[int] = None, window: Optional[int] = None,
                 qk_norm: bool = False, attn_softcap: Optional[float] = None, head_dim: Optional[int] = None,
                 attn_scale: Optional[float] = None, attn_sinks: bool = False, device=None, dtype=None) -> None:
        super().__init__()
        fk = {"device": device, "dtype": dtype}
        if head_dim is None:
            head_dim = d_model // nhead
        elif isinstance(head_dim, bool) or not isinstance(head_dim, int) or head_dim < 1:
            raise ValueError(f"head_dim must be an int >= 1 or None, got {head_dim!r}")
        self.d_model, self.nhead, self.head_dim = d_model, nhead, head_dim
        self.attn_dim = nhead * head_dim  # width of o: d_model unless head_dim is given
        if attn_scale is not None:
            if (isinstance(attn_scale, bool) or not isinstance(attn_scale, (int, float))
                    or not math.isfinite(attn_scale) or attn_scale <= 0):
                raise ValueError(f"attn_scale must be a finite number > 0 or None, got {attn_scale!r}")
            attn_scale = float(attn_scale)
        self.attn_scale = attn_scale  # None: the ops' own 1 / sqrt(head_dim)
        if attn_softcap is not None:
            if (isinstance(attn_softcap, bool) or not isinstance(attn_softcap, (int, float))
                    or not math.isfinite(attn_softcap) or attn_softcap <= 0):
                raise ValueError(f"attn_softcap must be a finite number > 0 or None, got {attn_softcap!r}")
            attn_softcap = float(attn_softcap)
        self.attn_softcap = attn_softcap
        if window is not None:
            if isinstance(window, bool) or not isinstance(window, int) or window < 1:
                raise ValueError(f"window must be an int >= 1 or None, got {window!r}")
            if not causal:
                raise ValueError("window (sliding-window attention) needs causal=True")
        self.window = window
        self.n_kv_heads = nhead if n_kv_heads is None else int(n_kv_heads)
        if self.n_kv_heads <= 0 or nhead % self.n_kv_heads != 0:
            raise ValueError(f"n_kv_heads must divide nhead, got nhead={nhead}, n_kv_heads={n_kv_heads}")
        # width of the QKV projection: H Q heads, then Hkv K heads, then Hkv V heads (3 * d_model for Hkv == H)
        self.qkv_dim = (nhead + 2 * self.n_kv_heads) * self.head_dim
        self.dropout, self.norm_first, self.causal, self.eps = dropout, norm_first, causal, layer_norm_eps
        self.norm, self.rope, self.rope_base = norm, rope, rope_base
        if rope and self.head_dim % 2 != 0:  # (the HIP kernel wants a multiple of 16 and says so itself)
            raise ValueError(f"rope needs an even head dim, got {self.head_dim}")
        self.in_proj_weight = mark_gemm_weight(nn.Parameter(torch.empty(self.qkv_dim, d_model, **fk)))
        self.in_proj_bias = nn.Parameter(torch.empty(self.qkv_dim, **fk)) if bias else None
        if norm_first:
            _init_norm(self, d_model, norm, fk)
        if rope:
            # cos / sin tables [positions, head_dim / 2], fp32: sized to the sequence, grown on demand
            empty = torch.empty(0, self.head_dim // 2, device=device, dtype=torch.float32)
            self.register_buffer("rope_cos", empty, persistent=False)
            self.register_buffer("rope_sin", empty.clone(), persistent=False)
        self.qk_norm = bool(qk_norm)
        if self.qk_norm:
            # per-head RMSNorm weights of the Q and of the K heads (not GEMM weights: the norm's backward writes
            # their gradients)
            self.q_norm_weight = nn.Parameter(torch.empty(self.head_dim, **fk))
            self.k_norm_weight = nn.Parameter(torch.empty(self.head_dim, **fk))
        self.attn_sinks = bool(attn_sinks)
        if self.attn_sinks:
            # one learned logit per query head in the softmax's denominator (not a GEMM weight: the attention
            # backward writes its gradient)
            self.sinks = nn.Parameter(torch.empty(nhead, **fk))
        self.reset_parameters()

    def reset_parameters(self) -> None:
        # nn.MultiheadAttention's init: xavier on in_proj, zero biases.
        nn.init.xavier_uniform_(self.in_proj_weight)
        if self.in_proj_bias is not None:
            nn.init.zeros_(self.in_proj_bias)
        if self.norm_first:
            _reset_norm(self)
        if self.qk_norm:
            nn.init.ones_(self.q_norm_weight)
            nn.init.ones_(self.k_norm_weight)
        if self.attn_sinks:
            nn.init.zeros_(self.sinks)

    def _rope_tables(self, seq_len: int, device):
        # rebuilt when too short, on another device, or cast by a module-wide .to(dtype): the kernel reads fp32
        if (self.rope_cos.shape[0] < seq_len or self.rope_cos.device != device
                or self.rope_cos.dtype != torch.float32):
            cos, sin = ops.rope_tables(seq_len, self.head_dim, self.rope_base, device=device)
            self.rope_cos, self.rope_sin = cos, sin
        return self.rope_cos, self.rope_sin

    def forward(self, x: Tensor) -> Tensor:
        return self.forward_fanout(x, fanout=False)[0]

    def _documents(self, B: int, S: int) -> Optional[Tensor]:
        """The calling thread's document bounds (``ops.use_documents``) for a ``[B, S, E]`` input, or None: a
        packed batch's tokens attend inside their own document only.  No parameter or config field: without a
        context nothing changes."""
        docs = ops.current_documents()
        if docs is None:
            return None
        if not self.causal:
            raise ValueError("AttentionCore: document bounds are set (ops.use_documents) but this core is not "
                             "causal; bidirectional document masks are not supported")
        if tuple(docs.shape) != (B, 2, S):
            raise ValueError(f"AttentionCore: document bounds {tuple(docs.shape)} do not match the input's "
                             f"[B, 2, S] = [{B}, 2, {S}]")
        return docs

    def forward_fanout(self, x: Tensor, fanout: bool = True):
        """``(o, x')``: ``x'`` is the block input for the residual branch.  With
        ``fanout`` the first consumer of ``x`` (LN1 for pre-norm, the QKV
        projection for post-norm) also returns it, so the residual gradient is
        added inside that op's backward kernel (no autograd add pass)."""
        B, S, _ = x.shape
        H, D, E = self.nhead, self.head_dim, self.attn_dim  # E: the width of o
        docs = self._documents(B, S)
        sinks = self.sinks if self.attn_sinks else None
        xr = x
        if self.norm_first:
            if fanout:
                x, xr = _norm_fanout(self, x)
            else:
                x = _norm(self, x, None, 0.0)
            qkv = ops.linear(x, self.in_proj_weight, self.in_proj_bias)
        elif fanout:
            qkv, xr = ops.linear_fanout(x, self.in_proj_weight, self.in_proj_bias)
        else:
            qkv = ops.linear(x, self.in_proj_weight, self.in_proj_bias)
        # The projection output viewed as [B, S, 3, H, D] feeds the kernel in
        # place; its output [B, S, H, D] is already [B, S, E] -- no transposes.
        Hkv = self.n_kv_heads
        if self.qk_norm:
            # Q and K heads normalised (and rotated, with rope) in one pass: where rope_projection runs otherwise
            cos, sin = self._rope_tables(S, qkv.device) if self.rope else (None, None)
            qkv_n = ops.qk_norm_rope_projection(qkv, self.q_norm_weight, self.k_norm_weight, self.eps, cos, sin, H,
                                                n_kv_heads=Hkv)
            if Hkv != H:
                o = ops.attention_gqa_packed(qkv_n, Hkv, causal=self.causal, dropout_p=self.dropout,
                                             training=self.training, scale=self.attn_scale, window=self.window,
                                             softcap=self.attn_softcap, doc_bounds=docs, sinks=sinks)
            else:
                o = ops.attention_packed(qkv_n, causal=self.causal, dropout_p=self.dropout, training=self.training,
                                         scale=self.attn_scale, window=self.window, softcap=self.attn_softcap,
                                         doc_bounds=docs, sinks=sinks)
            return o.reshape(B, S, E), xr
        if Hkv != H:
            # grouped-query attention: [B, S, H + 2 Hkv, D], the K/V heads read in place by every query head
            # of their group
            if self.rope:
                cos, sin = self._rope_tables(S, qkv.device)
                qkv4 = ops.rope_projection(qkv, cos, sin, H, n_kv_heads=Hkv)
            else:
                qkv4 = qkv.view(B, S, H + 2 * Hkv, D)
            o = ops.attention_gqa_packed(qkv4, Hkv, causal=self.causal, dropout_p=self.dropout,
                                         training=self.training, scale=self.attn_scale, window=self.window,
                                         softcap=self.attn_softcap, doc_bounds=docs, sinks=sinks)
            return o.reshape(B, S, E), xr
        if self.rope:
            # Q and K rotated: in the projection's own output where no graph is recorded, else into a new tensor
            cos, sin = self._rope_tables(S, qkv.device)
            qkv5 = ops.rope_projection(qkv, cos, sin, H)
        else:
            qkv5 = qkv.view(B, S, 3, H, D)
        o = ops.attention_packed(qkv5, causal=self.causal, dropout_p=self.dropout, training=self.training,
                                 scale=self.attn_scale, window=self.window, softcap=self.attn_softcap,
                                 doc_bounds=docs, sinks=sinks)
        return o.reshape(B, S, E), xr

    def flops_per_token(self, seq_len: int) -> float:
        """Document bounds (``ops.use_documents``) are per batch and not known here: a packed row is priced as
        causal, an upper bound on what the kernels run (so is ``block_costs``, which sums these)."""
        e = self.d_model
        # mean number of keys a query sees: all, half of them under the causal mask (the kernels skip the tiles
        # above the diagonal), and under a window w < seq_len the first w rows' 1 .. w and w for every later row
        w = self.window
        if w is not None and w < seq_len:
            keys = (w * (w + 1) / 2 + (seq_len - w) * w) / seq_len
        else:
            keys = seq_len * (0.5 if self.causal else 1.0)
        return 2 * self.qkv_dim * e + 4 * keys * self.attn_dim


class AttentionOutput(nn.Module):
    """``out_proj`` + dropout + residual (+ LayerNorm for post-norm): ``(x, o) -> y``.

    ``attn_dim``: the width of ``o`` (``d_model`` unless the core has a head dim of its own).
    ``sandwich_norm``: ``y = x + RMSNorm(out_proj(o)) * post_norm_weight``."""

    def __init__(self, d_model: int, dropout: float, *, norm_first: bool, layer_norm_eps: float,
                 norm: str = "layer", bias: bool = True, attn_dim: Optional[int] = None, sandwich_norm: bool = False,
                 device=None, dtype=None) -> None:
        super().__init__()
        fk = {"device": device, "dtype": dtype}
        self.d_model, self.dropout, self.norm_first, self.eps = d_model, dropout, norm_first, layer_norm_eps
        self.norm = norm
        self.attn_dim = d_model if attn_dim is None else int(attn_dim)
        self.sandwich_norm = _check_sandwich(sandwich_norm, norm_first, norm, dropout)
        self.out_proj_weight = mark_gemm_weight(nn.Parameter(torch.empty(d_model, self.attn_dim, **fk)))
        self.out_proj_bias = nn.Parameter(torch.empty(d_model, **fk)) if bias else None
        if not norm_first:
            _init_norm(self, d_model, norm, fk)
        if self.sandwich_norm:  # not a GEMM weight: the norm's backward writes its gradient
            self.post_norm_weight = nn.Parameter(torch.empty(d_model, **fk))
        self.reset_parameters()

    def reset_parameters(self) -> None:
        bound = 1.0 / math.sqrt(self.attn_dim)
        nn.init.uniform_(self.out_proj_weight, -bound, bound)
        if self.out_proj_bias is not None:
            nn.init.zeros_(self.out_proj_bias)
        if not self.norm_first:
            _reset_norm(self)
        if self.sandwich_norm:
            nn.init.ones_(self.post_norm_weight)

    def forward(self, x: Tensor, o: Tensor) -> Tensor:
        p = self.dropout if self.training else 0.0
        if self.sandwich_norm:
            a = ops.linear(o, self.out_proj_weight, self.out_proj_bias)
            return ops.rms_norm_residual(a, x, self.post_norm_weight, self.eps)
        if self.norm_first:
            return ops.linear_residual(o, self.out_proj_weight, self.out_proj_bias, x, p, self.training)
        a = ops.linear(o, self.out_proj_weight, self.out_proj_bias)
        return _norm(self, a, x, p)

    def flops_per_token(self, seq_len: int) -> float:
        return 2 * self.d_model * self.attn_dim


class SelfAttentionBlock(nn.Module):
    """Attention half of a Transformer layer: ``y = out(x, core(x))``.

    Post-norm: ``LN1(x + drop(out_proj(attn(qkv(x)))))``; pre-norm:
    ``x + drop(out_proj(attn(qkv(LN1(x)))))``.
    """

    def __init__(self, d_model: int, nhead: int, dropout: float = 0.1, *, norm_first: bool = False,
                 causal: bool = False, layer_norm_eps: float = 1e-5, norm: str = "layer", bias: bool = True,
                 rope: bool = False, rope_base: float = 10000.0, n_kv_heads: Optional[int] = None,
                 window: Optional[int] = None, qk_norm: bool = False, attn_softcap: Optional[float] = None,
                 sandwich_norm: bool = False, head_dim: Optional[int] = None, attn_scale: Optional[float] = None,
                 attn_sinks: bool = False, device=None, dtype=None) -> None:
        super().__init__()
        if head_dim is None and d_model % nhead != 0:
            raise ValueError("d_model must be divisible by nhead")
        _check_sandwich(sandwich_norm, norm_first, norm, dropout)
        self.core = AttentionCore(d_model, nhead, dropout, norm_first=norm_first, causal=causal,
                                  layer_norm_eps=layer_norm_eps, norm=norm, bias=bias, rope=rope,
                                  rope_base=rope_base, n_kv_heads=n_kv_heads, window=window, qk_norm=qk_norm,
                                  attn_softcap=attn_softcap, head_dim=head_dim, attn_scale=attn_scale,
                                  attn_sinks=attn_sinks, device=device, dtype=dtype)
        self.out = AttentionOutput(d_model, dropout, norm_first=norm_first, layer_norm_eps=layer_norm_eps,
                                   norm=norm, bias=bias, attn_dim=self.core.attn_dim, sandwich_norm=sandwich_norm,
                                   device=device, dtype=dtype)

    def reset_parameters(self) -> None:
        self.core.reset_parameters()
        self.out.reset_parameters()

    def forward(self, x: Tensor) -> Tensor:
        o, xr = self.core.forward_fanout(x, FANOUT)
        return self.out(xr, o)

    def flops_per_token(self, seq_len: int) -> float:
        return self.core.flops_per_token(seq_len) + self.out.flops_per_token(seq_len)


class _Unpack(torch.autograd.Function):
    """A packed stage-boundary activation -> its parts, as contiguous views.

    The packs are block-concatenated (part after part in memory, not
    interleaved per row), so every part is a contiguous view -- the consumer
    needs no ``.contiguous()`` copies -- and the backward writes the parts'
    gradients into one packed gradient with a single concatenation (autograd's
    own slice/select backward would zero-fill a packed-size tensor per part
    and add them)."""

    @staticmethod
    def forward(ctx, packed: Tensor, lead, widths):  # type: ignore[override]
        flat = packed.reshape(-1)
        n = math.prod(lead)
        outs, o = [], 0
        for w in widths:
            outs.append(flat[o:o + n * w].view(*lead, w))
            o += n * w
        ctx.packed_shape, ctx.lead, ctx.widths = packed.shape, lead, widths
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):  # type: ignore[override]
        ref = next(g for g in grads if g is not None)
        n = math.prod(ctx.lead)
        parts = [g.reshape(-1) if g is not None else ref.new_zeros(n * w) for g, w in zip(grads, ctx.widths)]
        return torch.cat(parts).view(ctx.packed_shape), None, None


def unpack(packed: Tensor, lead, widths):
    return _Unpack.apply(packed, tuple(lead), tuple(widths))


class PackedAttentionCore(nn.Module):
    """Pipeline unit: ``x -> stack(x, core(x))`` so a stage boundary can fall
    between the attention core and its output projection.  A core whose ``o`` is
    not ``d_model`` wide (``head_dim``) packs ``[.., E + A]``, x then o
    block-concatenated (see :class:`_Unpack`)."""

    def __init__(self, core: AttentionCore) -> None:
        super().__init__()
        self.core = core

    def reset_parameters(self) -> None:
        self.core.reset_parameters()

    def forward(self, x: Tensor) -> Tensor:
        # x's residual-branch gradient comes back through the QKV dgrad epilogue (fan-out)
        o, xr = self.core.forward_fanout(x, FANOUT)
        if o.shape[-1] == xr.shape[-1]:
            return torch.stack((xr, o))
        return torch.cat((xr.reshape(-1), o.reshape(-1))).view(*x.shape[:-1], x.shape[-1] + o.shape[-1])

    def flops_per_token(self, seq_len: int) -> float:
        return self.core.flops_per_token(seq_len)


class PackedAttentionOutput(nn.Module):
    """Pipeline unit: ``stack(x, o) -> out(x, o)`` (``cat(x, o)`` of widths ``(E, A)`` when ``A != E``)."""

    def __init__(self, out: AttentionOutput) -> None:
        super().__init__()
        self.out = out

    def reset_parameters(self) -> None:
        self.out.reset_parameters()

    def forward(self, packed: Tensor) -> Tensor:
        e, a = self.out.d_model, self.out.attn_dim
        if a != e:
            x, o = unpack(packed, packed.shape[:-1], (e, a))
        else:
            x, o = unpack(packed, packed.shape[1:-1], (e, e))
        return self.out(x, o)

    def flops_per_token(self, seq_len: int) -> float:
        return self.out.flops_per_token(seq_len)


class FeedForwardIn(nn.Module):
    """First half of the MLP: ``h = drop(act(W1 x + b1))`` (pre-norm: of ``LN2(x)``)."""

    def __init__(self, d_model: int, dim_feedforward: int, dropout: float, activation: str, *, norm_first: bool,
                 layer_norm_eps: float, norm: str = "layer", bias: bool = True, device=None, dtype=None) -> None:
        super().__init__()
        fk = {"device": device, "dtype": dtype}
        self.d_model, self.dim_feedforward = d_model, dim_feedforward
        self.dropout, self.activation, self.norm_first, self.eps = dropout, activation, norm_first, layer_norm_eps
        self.norm = norm
        # "swiglu" / "geglu": the gate projection (rows [0, F)) and the up projection (rows [F, 2F)) in ONE weight
        width = 2 * dim_feedforward if activation in GATED_ACTS else dim_feedforward
        self.linear1_weight = mark_gemm_weight(nn.Parameter(torch.empty(width, d_model, **fk)))
        self.linear1_bias = nn.Parameter(torch.empty(width, **fk)) if bias else None
        if norm_first:
            _init_norm(self, d_model, norm, fk)
        self.reset_parameters()

    def reset_parameters(self) -> None:
        nn.init.kaiming_uniform_(self.linear1_weight, a=math.sqrt(5))
        if self.linear1_bias is not None:
            bound = 1.0 / math.sqrt(self.linear1_weight.shape[1])
            nn.init.uniform_(self.linear1_bias, -bound, bound)
        if self.norm_first:
            _reset_norm(self)

    def forward(self, x: Tensor) -> Tensor:
        return self.forward_fanout(x, fanout=False)[0]

    def forward_fanout(self, x: Tensor, fanout: bool = True, fold: Optional[ActFold] = None):
        """``(h, x')`` -- see :meth:`AttentionCore.forward_fanout`.  ``fold``: h's
        only consumer applies the activation backward (:class:`ActFold`)."""
        p = self.dropout if self.training else 0.0
        w, b, act = self.linear1_weight, self.linear1_bias, self.activation
        if act in GATED_ACTS:
            if p > 0.0:
                raise ValueError(f"activation={act!r} has no dropout between the gate and linear2: set "
                                 "act_dropout=0.0 (FeedForwardIn.dropout)")
            gate = ops.swiglu if act == "swiglu" else ops.geglu
            if self.norm_first:
                xn, xr = _norm_fanout(self, x) if fanout else (_norm(self, x, None, 0.0), x)
                return gate(ops.linear(xn, w, b)), xr
            gu, xr = ops.linear_fanout(x, w, b) if fanout else (ops.linear(x, w, b), x)
            return gate(gu), xr
        if self.norm_first:
            if fanout:
                xn, xr = _norm_fanout(self, x)
            else:
                xn, xr = _norm(self, x, None, 0.0), x
            return ops.linear(xn, w, b, act, p, self.training, act_fold_out=fold), xr
        if fanout:
            return ops.linear_fanout(x, w, b, act, p, self.training, act_fold_out=fold)
        return ops.linear(x, w, b, act, p, self.training, act_fold_out=fold), x

    def flops_per_token(self, seq_len: int) -> float:
        return 2 * self.d_model * self.linear1_weight.shape[0]  # the gated first GEMM is 2F wide


class FeedForwardOut(nn.Module):
    """Second half: ``LN2(x + drop(W2 h + b2))`` (pre-norm: ``x + drop(W2 h + b2)``;
    ``sandwich_norm``: ``x + RMSNorm(W2 h + b2) * post_norm_weight``)."""

    def __init__(self, d_model: int, dim_feedforward: int, dropout: float, *, norm_first: bool, layer_norm_eps: float,
                 norm: str = "layer", bias: bool = True, sandwich_norm: bool = False, device=None,
                 dtype=None) -> None:
        super().__init__()
        fk = {"device": device, "dtype": dtype}
        self.d_model, self.dim_feedforward = d_model, dim_feedforward
        self.dropout, self.norm_first, self.eps = dropout, norm_first, layer_norm_eps
        self.norm = norm
        self.linear2_weight = mark_gemm_weight(nn.Parameter(torch.empty(d_model, dim_feedforward, **fk)))
        self.linear2_bias = nn.Parameter(torch.empty(d_model, **fk)) if bias else None
        if not norm_first:
            _init_norm(self, d_model, norm, fk)
        self.sandwich_norm = _check_sandwich(sandwich_norm, norm_first, norm, dropout)
        if self.sandwich_norm:  # not a GEMM weight: the norm's backward writes its gradient
            self.post_norm_weight = nn.Parameter(torch.empty(d_model, **fk))
        self.reset_parameters()

    def reset_parameters(self) -> None:
        nn.init.kaiming_uniform_(self.linear2_weight, a=math.sqrt(5))
        if self.linear2_bias is not None:
            bound = 1.0 / math.sqrt(self.linear2_weight.shape[1])
            nn.init.uniform_(self.linear2_bias, -bound, bound)
        if not self.norm_first:
            _reset_norm(self)
        if self.sandwich_norm:
            nn.init.ones_(self.post_norm_weight)

    def forward(self, x: Tensor, h: Tensor, fold: Optional[ActFold] = None) -> Tensor:
        p = self.dropout if self.training else 0.0
        if self.sandwich_norm:
            h = ops.linear(h, self.linear2_weight, self.linear2_bias, act_fold_in=fold)
            return ops.rms_norm_residual(h, x, self.post_norm_weight, self.eps)
        if self.norm_first:
            return ops.linear_residual(h, self.linear2_weight, self.linear2_bias, x, p, self.training,
                                       act_fold_in=fold)
        h = ops.linear(h, self.linear2_weight, self.linear2_bias, act_fold_in=fold)
        return _norm(self, h, x, p)

    def flops_per_token(self, seq_len: int) -> float:
        return 2 * self.d_model * self.dim_feedforward


class FeedForwardBlock(nn.Module):
    """``LN2(x + drop(W2 drop(act(W1 x))))`` as two halves (:class:`FeedForwardIn`,
    :class:`FeedForwardOut`) so a pipeline boundary may fall between them."""

    def __init__(
        self,
        d_model: int,
        dim_feedforward: int,
        dropout: float = 0.1,
        activation: str = "relu",
        *,
        norm_first: bool = False,
        layer_norm_eps: float = 1e-5,
        norm: str = "layer",
        bias: bool = True,
        sandwich_norm: bool = False,
        device=None,
        dtype=None,
    ) -> None:
        super().__init__()
        self.d_model, self.dim_feedforward = d_model, dim_feedforward
        self.norm_first = norm_first
        self.fc_in = FeedForwardIn(d_model, dim_feedforward, dropout, activation, norm_first=norm_first,
                                   layer_norm_eps=layer_norm_eps, norm=norm, bias=bias, device=device, dtype=dtype)
        self.fc_out = FeedForwardOut(d_model, dim_feedforward, dropout, norm_first=norm_first,
                                     layer_norm_eps=layer_norm_eps, norm=norm, bias=bias,
                                     sandwich_norm=sandwich_norm, device=device, dtype=dtype)

    def reset_parameters(self) -> None:
        self.fc_in.reset_parameters()
        self.fc_out.reset_parameters()

    def forward(self, x: Tensor) -> Tensor:
        # h's only consumer is fc_out: its dgrad applies the activation backward
        fold = ActFold() if _folds(self.fc_in, self.training) else None
        h, xr = self.fc_in.forward_fanout(x, FANOUT, fold)
        out = self.fc_out(xr, h, fold)
        if fold is not None:
            fold.release()
        return out

    def flops_per_token(self, seq_len: int) -> float:
        return self.fc_in.flops_per_token(seq_len) + self.fc_out.flops_per_token(seq_len)


EXPERT_GEMMS = ("loop", "grouped")


def check_expert_gemm(expert_gemm: str, capacity_factor: Optional[float]) -> None:
    if expert_gemm not in EXPERT_GEMMS:
        raise ValueError(f"expert_gemm must be one of {EXPERT_GEMMS}, got {expert_gemm!r}")
    if expert_gemm == "grouped" and capacity_factor is not None:
        raise ValueError(f"expert_gemm='grouped' is dropless: it needs capacity_factor=None, got {capacity_factor!r}")


class MoEFeedForwardBlock(nn.Module):
    """Mixture-of-experts MLP half of a pre-norm layer (Mixtral, Qwen3-MoE): ``x + sum_j gate_j expert_{idx_j}(norm(x))``
    with ``n_experts`` gated MLPs (``activation="swiglu"`` or ``"geglu"``) of which every token runs its
    ``experts_per_token`` best, weighted by the softmax over their router logits.  Bias-free and pre-norm only, no
    dropout inside.

    Parameters: ``norm_weight``; a plain ``router_weight [Ne, E]`` (not a tagged GEMM weight: ``ops.linear`` runs it
    with ``torch.matmul`` where the tile kernel does not fit); per expert ``experts_w1[e] [2F, E]`` (gate rows
    first) and ``experts_w2[e] [E, F]``, each a GEMM weight of its own, so the flat optimizer, the deferred weight
    gradients and the checkpoint files treat them like any other.

    Forward: norm, router logits, ``ops.moe_route``, ``ops.moe_assign`` with ``C = ops.moe_capacity(T, Ne, k,
    capacity_factor)`` slots per expert (``T`` the tokens of the call; ``capacity_factor=None`` drops nothing),
    ``ops.moe_dispatch``, per expert ``ops.linear`` on its ``[C, E]`` rows, the gate kernel, ``ops.linear``, then
    ``ops.moe_combine`` with the residual.  Every shape is static.  Empty slots hold zeros and produce zeros.

    Load balancing (Switch / Mixtral): ``aux = Ne sum_e (counts_e / (T k)) (probs_sum_e / T)``.  It is not added to
    the loss tensor; the block feeds its gradient ``aux_coef * aux_scale * Ne / (T^2 k) * counts`` into the router's
    backward.  ``aux_scale`` (a float attribute, 1.0) is the factor the loss's own backward is seeded with:
    :class:`~mipipe.parallel.engine.PipelineEngine` sets it to ``1 / (chunks * grad_divisor)`` on every block of its
    modules; outside the engine set it yourself when the loss is scaled (gradient accumulation).  ``aux_coef=0``
    turns the term off.  ``last_aux`` and ``last_drop_fraction`` are detached device scalars of the last forward,
    for logging.

    ``expert_gemm="grouped"`` (needs ``capacity_factor=None``) is the dropless path: ``ops.moe_assign_sorted`` sorts
    the choices by expert into ``ops.moe_sorted_rows(T, Ne, k)`` rows (segments padded to whole 128-row tiles: about
    ``k T + 64 Ne`` rows, not ``Ne ceil64(T)``), and the experts run as ``ops.grouped_linear(w1)``, the gate op once,
    ``ops.grouped_linear(w2)``: three GEMM launches and one gate launch per direction whatever ``Ne``, no
    concatenation.  Nothing is dropped: ``last_drop_fraction`` is exactly 0.  Its weight gradients run in the
    backward, not in the deferred flush.  ``"loop"`` (the default) is the path described above."""

    def __init__(self, d_model: int, dim_feedforward: int, n_experts: int, experts_per_token: int = 2, *,
                 capacity_factor: Optional[float] = 1.25, aux_coef: float = 0.01, activation: str = "swiglu",
                 norm_first: bool = True, norm: str = "rms", layer_norm_eps: float = 1e-5, bias: bool = False,
                 expert_gemm: str = "loop", device=None, dtype=None) -> None:
        super().__init__()
        fk = {"device": device, "dtype": dtype}
        if not norm_first or bias:
            raise ValueError(f"MoEFeedForwardBlock is pre-norm and bias-free, got norm_first={norm_first}, bias={bias}")
        check_expert_gemm(expert_gemm, capacity_factor)
        self.expert_gemm = expert_gemm
        if activation not in GATED_ACTS:
            raise ValueError(f"MoEFeedForwardBlock: activation must be one of {GATED_ACTS}, got {activation!r}")
        if isinstance(n_experts, bool) or not isinstance(n_experts, int) or not 2 <= n_experts <= ops.moe.MAX_EXPERTS:
            raise ValueError(f"n_experts must be an int in [2, {ops.moe.MAX_EXPERTS}], got {n_experts!r}")
        if (isinstance(experts_per_token, bool) or not isinstance(experts_per_token, int)
                or not 1 <= experts_per_token <= min(ops.moe.MAX_TOP_K, n_experts)):
            raise ValueError(f"experts_per_token must be an int in [1, min({ops.moe.MAX_TOP_K}, n_experts)], got "
                             f"{experts_per_token!r}")
        if capacity_factor is not None and not (math.isfinite(capacity_factor) and capacity_factor > 0):
            raise ValueError(f"capacity_factor must be a finite number > 0 or None, got {capacity_factor!r}")
        self.d_model, self.dim_feedforward = d_model, dim_feedforward
        self.n_experts, self.experts_per_token = n_experts, experts_per_token
        self.capacity_factor, self.aux_coef, self.aux_scale = capacity_factor, float(aux_coef), 1.0
        self.activation, self.norm_first, self.norm, self.eps = activation, True, norm, layer_norm_eps
        _init_norm(self, d_model, norm, fk)
        self.router_weight = nn.Parameter(torch.empty(n_experts, d_model, **fk))
        self.experts_w1 = nn.ParameterList(
            [mark_gemm_weight(nn.Parameter(torch.empty(2 * dim_feedforward, d_model, **fk))) for _ in range(n_experts)])
        self.experts_w2 = nn.ParameterList(
            [mark_gemm_weight(nn.Parameter(torch.empty(d_model, dim_feedforward, **fk))) for _ in range(n_experts)])
        self.last_aux: Optional[Tensor] = None
        self.last_drop_fraction: Optional[Tensor] = None
        self.reset_parameters()

    def reset_parameters(self) -> None:
        _reset_norm(self)
        nn.init.normal_(self.router_weight, std=0.02)
        for w in list(self.experts_w1) + list(self.experts_w2):
            nn.init.kaiming_uniform_(w, a=math.sqrt(5))

    def route(self, logits: Tensor, tokens: int):
        """``(gate, slot, src, capacity)`` of the router ``logits [T, Ne]``; records the logging scalars and, when a
        graph is recorded, attaches the load-balancing gradient to the gate.  The grouped path returns ``(offsets,
        tile_expert)`` of the sorted layout in the capacity's place."""
        ne, k = self.n_experts, self.experts_per_token
        idx, gate, probs_sum = ops.moe_route(logits, k)
        if getattr(self, "expert_gemm", "loop") == "grouped":
            slot, src, counts, offsets, tile_expert = ops.moe_assign_sorted(idx, ne)
            cap = (offsets, tile_expert)
        else:
            cap = ops.moe_capacity(tokens, ne, k, self.capacity_factor)
            slot, src, counts = ops.moe_assign(idx, ne, cap)
        attach = self.aux_coef != 0.0 and torch.is_grad_enabled() and gate.requires_grad
        with torch.no_grad():
            load = counts.to(probs_sum.dtype)
            self.last_aux = (load * probs_sum).sum() * (ne / (float(tokens) * tokens * k))
            self.last_drop_fraction = (slot < 0).to(torch.float32).mean()
            if attach:
                dprobs = load * (self.aux_coef * self.aux_scale * ne / (float(tokens) * tokens * k))
        if attach:
            gate = ops.moe_attach_aux(gate, probs_sum, dprobs)
        return gate, slot, src, cap

    def experts(self, xe: Tensor, cap: int) -> Tensor:
        """The experts on their ``[C, E]`` slices of ``xe [Ne * C, E]``."""
        act = ops.swiglu if self.activation == "swiglu" else ops.geglu
        outs = []
        for e in range(self.n_experts):
            h = act(ops.linear(xe[e * cap:(e + 1) * cap], self.experts_w1[e]))
            outs.append(ops.linear(h, self.experts_w2[e]))
        return torch.cat(outs)

    def experts_grouped(self, xe: Tensor, offsets: Tensor, tile_expert: Tensor) -> Tensor:
        """The experts on their row ranges of the sorted ``xe [R, E]``: one launch per GEMM and one for the gate."""
        act = ops.swiglu if self.activation == "swiglu" else ops.geglu
        h = act(ops.grouped_linear(xe, list(self.experts_w1), tile_expert, offsets))
        return ops.grouped_linear(h, list(self.experts_w2), tile_expert, offsets)

    def forward(self, x: Tensor) -> Tensor:
        shape = x.shape
        xn, xr = _norm_fanout(self, x) if FANOUT else (_norm(self, x, None, 0.0), x)
        x2 = xn.reshape(-1, shape[-1])
        tokens = x2.shape[0]
        gate, slot, src, cap = self.route(ops.linear(x2, self.router_weight), tokens)
        if getattr(self, "expert_gemm", "loop") == "grouped":
            ye = self.experts_grouped(ops.moe_dispatch(x2, slot, src), *cap)
        else:
            ye = self.experts(ops.moe_dispatch(x2, slot, src), cap)
        return ops.moe_combine(ye, gate, slot, src, residual=xr.reshape(-1, shape[-1])).view(shape)

    def flops_per_token(self, seq_len: int) -> float:
        """The model's FLOPs: the router and the ``experts_per_token`` active experts, not the capacity padding."""
        e, f = self.d_model, self.dim_feedforward
        return 2 * e * self.n_experts + self.experts_per_token * (2 * e * 2 * f + 2 * e * f)


class PackedFeedForwardIn(nn.Module):
    """Pipeline unit: ``x -> [.., E + F]`` holding x and h block-concatenated
    (all of x, then all of h: see :class:`_Unpack`)."""

    def __init__(self, fc_in: FeedForwardIn) -> None:
        super().__init__()
        self.fc_in = fc_in

    def reset_parameters(self) -> None:
        self.fc_in.reset_parameters()

    def forward(self, x: Tensor) -> Tensor:
        h, xr = self.fc_in.forward_fanout(x, FANOUT)
        return torch.cat((xr.reshape(-1), h.reshape(-1))).view(*x.shape[:-1], x.shape[-1] + h.shape[-1])

    def flops_per_token(self, seq_len: int) -> float:
        return self.fc_in.flops_per_token(seq_len)


class PackedFeedForwardOut(nn.Module):
    """Pipeline unit: ``cat(x, h) -> fc_out(x, h)``."""

    def __init__(self, fc_out: FeedForwardOut) -> None:
        super().__init__()
        self.fc_out = fc_out

    def reset_parameters(self) -> None:
        self.fc_out.reset_parameters()

    def forward(self, packed: Tensor) -> Tensor:
        e = self.fc_out.d_model
        x, h = unpack(packed, packed.shape[:-1], (e, packed.shape[-1] - e))
        return self.fc_out(x, h)

    def flops_per_token(self, seq_len: int) -> float:
        return self.fc_out.flops_per_token(seq_len)


class TransformerEncoderLayer(nn.Sequential):
    """``nn.TransformerEncoderLayer`` equivalent (batch-first) as a 2-block Sequential."""

    def __init__(
        self,
        d_model: int,
        nhead: int,
        dim_feedforward: int = 2048,
        dropout: float = 0.1,
        activation: str = "relu",
        layer_norm_eps: float = 1e-5,
        norm_first: bool = False,
        causal: bool = False,
        device=None,
        dtype=None,
        *,
        norm: str = "layer",
        bias: bool = True,
        rope: bool = False,
        rope_base: float = 10000.0,
        n_kv_heads: Optional[int] = None,
        window: Optional[int] = None,
        qk_norm: bool = False,
        attn_softcap: Optional[float] = None,
        sandwich_norm: bool = False,
        head_dim: Optional[int] = None,
        attn_scale: Optional[float] = None,
        attn_sinks: bool = False,
    ) -> None:
        super().__init__(
            SelfAttentionBlock(d_model, nhead, dropout, norm_first=norm_first, causal=causal,
                               layer_norm_eps=layer_norm_eps, norm=norm, bias=bias, rope=rope, rope_base=rope_base,
                               n_kv_heads=n_kv_heads, window=window, qk_norm=qk_norm, attn_softcap=attn_softcap,
                               sandwich_norm=sandwich_norm, head_dim=head_dim, attn_scale=attn_scale,
                               attn_sinks=attn_sinks, device=device, dtype=dtype),
            FeedForwardBlock(d_model, dim_feedforward, dropout, activation, norm_first=norm_first,
                             layer_norm_eps=layer_norm_eps, norm=norm, bias=bias, sandwich_norm=sandwich_norm,
                             device=device, dtype=dtype),
        )

    @torch.no_grad()
    def load_from_torch(self, layer: nn.TransformerEncoderLayer) -> "TransformerEncoderLayer":
        """Copies weights from ``nn.TransformerEncoderLayer``."""
        attn, ff = self[0], self[1]
        if attn.core.n_kv_heads != attn.core.nhead:
            raise ValueError("load_from_torch: nn.TransformerEncoderLayer has no grouped-query attention "
                             f"(this layer has {attn.core.n_kv_heads} K/V heads for {attn.core.nhead} query heads)")
        attn.core.in_proj_weight.copy_(layer.self_attn.in_proj_weight)
        attn.core.in_proj_bias.copy_(layer.self_attn.in_proj_bias)
        attn.out.out_proj_weight.copy_(layer.self_attn.out_proj.weight)
        attn.out.out_proj_bias.copy_(layer.self_attn.out_proj.bias)
        norm1 = attn.core if attn.core.norm_first else attn.out
        norm1.norm_weight.copy_(layer.norm1.weight)
        norm1.norm_bias.copy_(layer.norm1.bias)
        ff.fc_in.linear1_weight.copy_(layer.linear1.weight)
        ff.fc_in.linear1_bias.copy_(layer.linear1.bias)
        ff.fc_out.linear2_weight.copy_(layer.linear2.weight)
        ff.fc_out.linear2_bias.copy_(layer.linear2.bias)
        norm2 = ff.fc_in if ff.norm_first else ff.fc_out
        norm2.norm_weight.copy_(layer.norm2.weight)
        norm2.norm_bias.copy_(layer.norm2.bias)
        return self


def check_global_every(global_every: Optional[int], window: Optional[int]) -> None:
    if global_every is None:
        return
    if isinstance(global_every, bool) or not isinstance(global_every, int) or global_every < 2:
        raise ValueError(f"global_every must be an int >= 2 or None, got {global_every!r}")
    if window is None:
        raise ValueError("global_every (local / global layers) needs a window for the local layers")


def layer_window(window: Optional[int], global_every: Optional[int], i: int) -> Optional[int]:
    """The window of layer ``i`` (0-based): none for a global layer, ``(i + 1) % global_every == 0``."""
    if global_every is not None and (i + 1) % global_every == 0:
        return None
    return window


def transformer_blocks(
    num_layers: int,
    d_model: int,
    nhead: int,
    dim_feedforward: int,
    dropout: float,
    activation: str = "relu",
    *,
    norm_first: bool = False,
    causal: bool = False,
    norm: str = "layer",
    bias: bool = True,
    rope: bool = False,
    rope_base: float = 10000.0,
    n_kv_heads: Optional[int] = None,
    window: Optional[int] = None,
    qk_norm: bool = False,
    attn_softcap: Optional[float] = None,
    sandwich_norm: bool = False,
    head_dim: Optional[int] = None,
    attn_scale: Optional[float] = None,
    global_every: Optional[int] = None,
    attn_sinks: bool = False,
    n_experts: Optional[int] = None,
    experts_per_token: int = 2,
    capacity_factor: Optional[float] = 1.25,
    moe_aux_coef: float = 0.01,
    expert_gemm: str = "loop",
    device=None,
    dtype=None,
) -> List[nn.Module]:
    """``2 * num_layers`` single-tensor blocks (attention, MLP, attention, ...).

    ``global_every=n`` (needs ``window``): layer ``i`` (0-based) with ``(i + 1) % n == 0`` is a global layer,
    built with ``window=None``; every other layer gets the window (:func:`layer_window`).

    ``n_experts=Ne`` (``None``: dense) builds a :class:`MoEFeedForwardBlock` of ``Ne`` experts of width
    ``dim_feedforward`` in place of the :class:`FeedForwardBlock` of every layer (pre-norm, bias-free, gated
    activation, no sandwich norm); ``expert_gemm="grouped"`` (with ``capacity_factor=None``) selects its dropless
    grouped-GEMM path."""
    check_global_every(global_every, window)
    blocks: List[nn.Module] = []
    if n_experts is not None:
        if sandwich_norm:
            raise ValueError("n_experts (a mixture-of-experts MLP) does not combine with sandwich_norm")
        for i in range(num_layers):
            blocks.append(SelfAttentionBlock(d_model, nhead, dropout, norm_first=norm_first, causal=causal, norm=norm,
                                             bias=bias, rope=rope, rope_base=rope_base, n_kv_heads=n_kv_heads,
                                             window=layer_window(window, global_every, i), qk_norm=qk_norm,
                                             attn_softcap=attn_softcap, head_dim=head_dim, attn_scale=attn_scale,
                                             attn_sinks=attn_sinks, device=device, dtype=dtype))
            blocks.append(MoEFeedForwardBlock(d_model, dim_feedforward, n_experts, experts_per_token,
                                              capacity_factor=capacity_factor, aux_coef=moe_aux_coef,
                                              activation=activation, norm_first=norm_first, norm=norm, bias=bias,
                                              expert_gemm=expert_gemm, device=device, dtype=dtype))
        return blocks
    for i in range(num_layers):
        layer = TransformerEncoderLayer(d_model, nhead, dim_feedforward, dropout, activation,
                                        norm_first=norm_first, causal=causal, norm=norm, bias=bias, rope=rope,
                                        rope_base=rope_base, n_kv_heads=n_kv_heads,
                                        window=layer_window(window, global_every, i), qk_norm=qk_norm,
                                        attn_softcap=attn_softcap, sandwich_norm=sandwich_norm, head_dim=head_dim,
                                        attn_scale=attn_scale, attn_sinks=attn_sinks, device=device, dtype=dtype)
        blocks.extend(layer.children())
    return blocks


def pipeline_units(blocks: List[nn.Module]) -> List[nn.Module]:
    """Expands every :class:`SelfAttentionBlock` and :class:`FeedForwardBlock`
    into its two packed halves so a pipeline stage boundary may fall inside it
    (see :func:`merge_units`): 4 units per layer.  A :class:`MoEFeedForwardBlock` stays whole (its cut would
    need the routing tables in the boundary tensor): 3 units per layer."""
    units: List[nn.Module] = []
    for b in blocks:
        if isinstance(b, SelfAttentionBlock):
            units += [PackedAttentionCore(b.core), PackedAttentionOutput(b.out)]
        elif isinstance(b, FeedForwardBlock):
            units += [PackedFeedForwardIn(b.fc_in), PackedFeedForwardOut(b.fc_out)]
        else:
            units.append(b)
    return units


def merge_units(units: List[nn.Module]) -> List[nn.Module]:
    """Inverse of :func:`pipeline_units` within one stage: an adjacent
    (PackedAttentionCore, PackedAttentionOutput) pair of the same layer runs
    unpacked (no stack copy)."""
    out: List[nn.Module] = []
    i = 0
    while i < len(units):
        u = units[i]
        nxt = units[i + 1] if i + 1 < len(units) else None
        if isinstance(u, PackedAttentionCore) and isinstance(nxt, PackedAttentionOutput):
            blk = SelfAttentionBlock.__new__(SelfAttentionBlock)
            nn.Module.__init__(blk)
            blk.core = u.core
            blk.out = nxt.out
            out.append(blk)
            i += 2
            continue
        if isinstance(u, PackedFeedForwardIn) and isinstance(nxt, PackedFeedForwardOut):
            blk = FeedForwardBlock.__new__(FeedForwardBlock)
            nn.Module.__init__(blk)
            blk.d_model, blk.dim_feedforward = u.fc_in.d_model, u.fc_in.dim_feedforward
            blk.norm_first = u.fc_in.norm_first
            blk.fc_in = u.fc_in
            blk.fc_out = nxt.fc_out
            out.append(blk)
            i += 2
            continue
        out.append(u)
        i += 1
    return out


def block_flops(block: nn.Module, seq_len: int) -> float:
    """Training FLOPs per token of a block (forward x 3)."""
    f = getattr(block, "flops_per_token", None)
    if f is None:
        return 0.0
    return 3.0 * f(seq_len)
