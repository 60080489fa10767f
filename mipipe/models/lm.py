"""Language-model front/back ends and model builders.

Mirrors the reference driver's model (``/root/reference/main.py:24-73,115-157``):
``Encoder`` (embedding x sqrt(E) + sinusoidal positions + dropout) ->
N x TransformerEncoderLayer -> ``Decoder`` (Linear E -> V).  Batch-first
throughout (the reference transposes to seq-first for nn.TransformerEncoder and
back in the decoder; here no transpose is needed).

Builders return flat lists of single-tensor blocks so the pipeline balancer can
place stage boundaries anywhere, including between the attention and MLP
halves of a layer.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional

import torch
from torch import Tensor, nn

from .. import ops
from ..ops.linear import mark_gemm_weight
from ..ops.softcap import softcap_owned
from .transformer import (GATED_ACTS, FeedForwardBlock, check_expert_gemm, check_global_every, layer_window,
                          transformer_blocks)

__all__ = [
    "Encoder",
    "Decoder",
    "LMConfig",
    "CONFIGS",
    "MOE_CONFIGS",
    "build_lm_blocks",
    "sinusoidal_positions",
]


def sinusoidal_positions(max_len: int, d_model: int) -> Tensor:
    """The reference's PositionalEncoding table (``main.py:57-70``), fp32 [max_len, d]."""
    pe = torch.zeros(max_len, d_model)
    position = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, d_model, 2).float() * (-math.log(10000.0) / d_model))
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe


class Encoder(nn.Module):
    """Token embedding x sqrt(E) + positional encoding + dropout: ``[B, S] -> [B, S, E]``.

    ``positions`` picks the position signal added to the embedding:
    ``"sinusoidal"`` (the reference's table), ``"learned"`` (GPT-2's learned
    position embedding; ``learned_positions=True`` says the same) or ``"none"``
    (rotary models: the positions enter in the attention blocks).
    """

    def __init__(self, ntoken: int, d_model: int, dropout: float = 0.5, max_len: int = 5000, *,
                 learned_positions: bool = False, scale_embedding: bool = True, positions: Optional[str] = None,
                 device=None, dtype=None) -> None:
        super().__init__()
        fk = {"device": device, "dtype": dtype}
        if positions is None:
            positions = "learned" if learned_positions else "sinusoidal"
        if positions not in ("sinusoidal", "learned", "none"):
            raise ValueError(f"positions must be 'sinusoidal', 'learned' or 'none', got {positions!r}")
        if learned_positions and positions != "learned":
            raise ValueError(f"learned_positions=True contradicts positions={positions!r}")
        self.ntoken, self.d_model, self.dropout = ntoken, d_model, dropout
        self.scale = math.sqrt(d_model) if scale_embedding else 1.0
        self.weight = nn.Parameter(torch.empty(ntoken, d_model, **fk))
        self.positions = positions
        self.learned_positions = positions == "learned"
        if positions == "learned":
            self.pos_weight = nn.Parameter(torch.empty(max_len, d_model, device=device, dtype=torch.float32))
        elif positions == "sinusoidal":
            self.register_buffer("pe", sinusoidal_positions(max_len, d_model).to(device), persistent=False)
        self.max_len = max_len
        self.reset_parameters()

    def reset_parameters(self) -> None:
        nn.init.uniform_(self.weight, -0.1, 0.1)  # main.py:32-34
        if self.learned_positions:
            nn.init.normal_(self.pos_weight, std=0.01)
        elif self.positions == "sinusoidal" and self.pe.device.type != "meta":
            with torch.no_grad():
                self.pe.copy_(sinusoidal_positions(self.max_len, self.d_model))

    def forward(self, tokens: Tensor) -> Tensor:
        # learned positions: the fused kernels add them and accumulate their gradient
        if self.positions == "none":
            pe = None
        else:
            pe = self.pos_weight if self.learned_positions else self.pe
        return ops.embed_scale_posenc_dropout(tokens, self.weight, pe, self.scale, self.dropout, self.training)

    def flops_per_token(self, seq_len: int) -> float:
        return 0.0


class _VocabSlice(torch.autograd.Function):
    """``y[..., :V]`` of the padded logits.  Backward: when the incoming
    gradient is the fused cross-entropy's zero-padded buffer (its usual
    producer), that buffer IS the padded gradient -- no zero-fill + copy."""

    @staticmethod
    def forward(ctx, y, v):  # type: ignore[override]
        ctx.shape = y.shape
        return y[..., :v]

    @staticmethod
    def backward(ctx, g):  # type: ignore[override]
        from ..ops.loss import take_zero_padded

        width = ctx.shape[-1]
        if take_zero_padded(g, width):
            return torch.as_strided(g, ctx.shape, torch.empty(ctx.shape, device="meta").stride()), None
        out = g.new_zeros(ctx.shape)
        out[..., : g.shape[-1]] = g
        return out, None


class Decoder(nn.Module):
    """Linear ``E -> V`` (``main.py:42-55``).

    The weight is stored with the vocabulary padded to a multiple of
    ``pad_to`` (256: the large GEMM tile) -- zero rows, zero bias -- so the logits
    GEMM runs on the MFMA tile kernel; ``forward`` returns the ``[..., :V]``
    view and the fused cross-entropy reads it in place (strided rows).

    ``final_softcap=c`` (Gemma-2's ``final_logit_softcapping``) caps the logits
    at ``c * tanh(y / c)``: ``ops.softcap`` on the padded GEMM output, before the
    slice -- the pad columns stay exactly 0 (``tanh(0) = 0``), and so do the
    pad columns of the gradient.  It overwrites the GEMM output
    (``ops.softcap_owned``): ``ops.linear`` without an activation reads no output
    in its backward, and the cap's backward needs the capped logits only, which
    the cross-entropy saves anyway -- the cap holds no logits-sized tensor.
    """

    def __init__(self, ntoken: int, d_model: int, *, pad_to: int = 256, final_softcap: Optional[float] = None,
                 device=None, dtype=None) -> None:
        super().__init__()
        fk = {"device": device, "dtype": dtype}
        self.ntoken = ntoken
        if final_softcap is not None:
            if (isinstance(final_softcap, bool) or not isinstance(final_softcap, (int, float))
                    or not math.isfinite(final_softcap) or final_softcap <= 0):
                raise ValueError(f"final_softcap must be a finite number > 0 or None, got {final_softcap!r}")
            final_softcap = float(final_softcap)
        self.final_softcap = final_softcap
        self.padded = (ntoken + pad_to - 1) // pad_to * pad_to
        self.weight = mark_gemm_weight(nn.Parameter(torch.empty(self.padded, d_model, **fk)))
        self.bias = nn.Parameter(torch.zeros(self.padded, **fk))
        self.reset_parameters()

    def reset_parameters(self) -> None:
        with torch.no_grad():
            nn.init.uniform_(self.weight, -0.1, 0.1)  # main.py:47-50
            self.weight[self.ntoken:].zero_()
            nn.init.zeros_(self.bias)

    def forward(self, x: Tensor) -> Tensor:
        y = ops.linear(x, self.weight, self.bias)
        if self.final_softcap is not None:
            y = softcap_owned(y, self.final_softcap)  # y is this forward's own: nothing else reads it
        if self.padded == self.ntoken:
            return y
        if y.is_cuda and torch.is_grad_enabled() and y.requires_grad:
            return _VocabSlice.apply(y, self.ntoken)
        return y[..., : self.ntoken]

    def flops_per_token(self, seq_len: int) -> float:
        return 2.0 * self.weight.shape[0] * self.weight.shape[1]


class FinalNorm(nn.Module):
    """Pre-norm models' final norm: LayerNorm (GPT-2's ln_f) or, with ``norm="rms"``, RMSNorm (no bias)."""

    def __init__(self, d_model: int, eps: float = 1e-5, *, norm: str = "layer", device=None, dtype=None) -> None:
        super().__init__()
        if norm not in ("layer", "rms"):
            raise ValueError(f"norm must be 'layer' or 'rms', got {norm!r}")
        self.norm = norm
        self.weight = nn.Parameter(torch.ones(d_model, device=device, dtype=dtype))
        if norm == "layer":
            self.bias = nn.Parameter(torch.zeros(d_model, device=device, dtype=dtype))
        self.eps = eps

    def reset_parameters(self) -> None:
        nn.init.ones_(self.weight)
        if self.norm == "layer":
            nn.init.zeros_(self.bias)

    def forward(self, x: Tensor) -> Tensor:
        if self.norm == "rms":
            return ops.add_dropout_rms_norm(x, None, self.weight, self.eps, 0.0, self.training)
        return ops.add_dropout_layer_norm(x, None, self.weight, self.bias, self.eps, 0.0, self.training)

    def flops_per_token(self, seq_len: int) -> float:
        return 0.0


@dataclass
class LMConfig:
    name: str
    num_layers: int
    d_model: int
    nhead: int
    dim_feedforward: int
    vocab: int
    seq_len: int
    dropout: float = 0.2
    activation: str = "relu"
    norm_first: bool = False
    causal: bool = False
    learned_positions: bool = False
    scale_embedding: bool = True
    # dropout between the MLP's activation and its second linear: None = `dropout` (torch's
    # TransformerEncoderLayer: linear2(dropout(act(linear1(x))))); GPT-2's MLP has none there
    # (c_fc -> gelu -> c_proj -> resid dropout)
    act_dropout: Optional[float] = None
    notes: str = ""
    # LLaMA-style block options (defaults: the blocks above)
    norm: str = "layer"            # "layer" | "rms" (no norm bias)
    bias: bool = True              # False: no bias in the attention and MLP linears
    rope: bool = False             # rotary position embeddings on Q and K
    rope_base: float = 10000.0
    positions: Optional[str] = None  # Encoder positions; None: "learned" if learned_positions else "sinusoidal"
    n_kv_heads: Optional[int] = None  # grouped-query attention: K/V heads (a divisor of nhead); None = nhead
    window: Optional[int] = None      # sliding-window attention: keys a query sees, its own included (causal only)
    attn_softcap: Optional[float] = None   # attention scores capped at c * tanh(s / c) before the softmax (Gemma-2)
    final_softcap: Optional[float] = None  # output logits capped the same way before the loss (Gemma-2)
    # Gemma-2 block options (activation="geglu" is the fourth)
    sandwich_norm: bool = False       # x + RMSNorm(branch) * w: a second norm on each branch, before the residual add
    head_dim: Optional[int] = None    # head width; None = d_model // nhead
    attn_scale: Optional[float] = None  # score scale; None = head_dim ** -0.5 (Gemma-2: query_pre_attn_scalar ** -0.5)
    global_every: Optional[int] = None  # layer i is global (no window) when (i + 1) % n == 0; needs window
    attn_sinks: bool = False          # a learned logit per query head in the softmax's denominator (gpt-oss): [nhead]
    # Mixture-of-experts MLP in every layer (Mixtral, Qwen3-MoE): None = the dense MLP
    n_experts: Optional[int] = None   # experts per layer, each a gated MLP of width dim_feedforward
    experts_per_token: int = 2        # experts a token runs, weighted by the softmax over their router logits
    capacity_factor: Optional[float] = 1.25  # slots per expert = factor * tokens * k / n_experts; None drops nothing
    moe_aux_coef: float = 0.01        # weight of the load-balancing term in the router's gradient
    expert_gemm: str = "loop"         # "loop": one GEMM per expert on capacity slices; "grouped": dropless, needs
    #                                   capacity_factor=None (MoEFeedForwardBlock)
    qk_norm: bool = False             # per-head RMSNorm on Q and K before the rotation (Qwen3): two [head_dim] weights

    def __post_init__(self) -> None:
        check_global_every(self.global_every, self.window)
        check_expert_gemm(self.expert_gemm, self.capacity_factor)

    def head_width(self) -> int:
        return self.d_model // self.nhead if self.head_dim is None else self.head_dim

    def attn_dim(self) -> int:
        """Width of the attention output before ``out_proj``: ``H D`` (``d_model`` unless ``head_dim`` is set)."""
        return self.nhead * self.head_width()

    def qkv_dim(self) -> int:
        """Width of the QKV projection: ``(H + 2 Hkv) D`` (``3 d_model`` without grouped-query attention)."""
        hkv = self.nhead if self.n_kv_heads is None else self.n_kv_heads
        return (self.nhead + 2 * hkv) * self.head_width()

    def layer_window(self, i: int) -> Optional[int]:
        """The window of layer ``i`` (0-based): ``None`` for a global layer under ``global_every``."""
        return layer_window(self.window, self.global_every, i)

    def encoder_positions(self) -> str:
        return self.positions if self.positions is not None else ("learned" if self.learned_positions else "sinusoidal")

    def params(self) -> int:
        """Parameter count of the model :func:`build_lm_blocks` builds, without the zero rows that
        pad the decoder's vocabulary to a multiple of 256 (an implementation detail of its GEMM)."""
        e, f, v = self.d_model, self.dim_feedforward, self.vocab
        f1 = 2 * f if self.activation in GATED_ACTS else f   # the gated first GEMM
        nb = 1 if self.bias else 0
        norm = e * (2 if self.norm == "layer" else 1)
        qkv = self.qkv_dim()
        if self.n_experts is not None:  # the router and the experts (bias-free) in place of the dense MLP
            mlp = self.n_experts * (e + f1 * e + e * f)
            layer = (qkv + self.attn_dim()) * e + 2 * norm + mlp + nb * (qkv + e)
        else:
            layer = (qkv + self.attn_dim()) * e + 2 * norm + f1 * e + e * f + nb * (qkv + e + f1 + e)
        if self.qk_norm:
            layer += 2 * self.head_width()
        if self.attn_sinks:
            layer += self.nhead
        if self.sandwich_norm:
            layer += 2 * e   # the two post-norm weights
        total = self.num_layers * layer + v * e
        if self.encoder_positions() == "learned":
            total += max(self.seq_len, 1024) * e
        if self.norm_first:
            total += norm
        return total + (v * e + v)


# What every Gemma-2 config shares: pre-norm RMSNorm with a second norm on each branch, GeGLU, rotary positions
# (base 10000), no biases, no dropout, every second layer global, soft caps 50 / 30, the embedding scaled by sqrt(E).
_GEMMA2 = dict(dropout=0.0, activation="geglu", norm_first=True, causal=True, scale_embedding=True, act_dropout=0.0,
               norm="rms", bias=False, rope=True, rope_base=10000.0, positions="none", global_every=2,
               sandwich_norm=True, attn_softcap=50.0, final_softcap=30.0)
_GEMMA2_NOTE = ("Not Gemma-2's: the decoder is untied and keeps its (zero-initialised) bias, the norms' eps is 1e-5 "
                "rather than 1e-6 (the block's layer_norm_eps is not a config field), and the norm weights are "
                "plain w rather than 1 + w")

# Mixture-of-experts configs.  Their layers are three pipeline units (core, out, moe), not the four of every config
# that CONFIGS lists, so they are kept apart: CONFIGS[name] finds them, a sweep over CONFIGS does not run into them.
MOE_CONFIGS = {
    # mistral_tiny with a mixture-of-experts MLP: 4 experts of width 512, every token runs its best 2.
    "moe_tiny": LMConfig("moe_tiny", 2, 256, 4, 512, 1000, 192, dropout=0.0, activation="swiglu",
                         norm_first=True, causal=True, scale_embedding=False, act_dropout=0.0, norm="rms",
                         bias=False, rope=True, positions="none", n_kv_heads=2, window=48, n_experts=4,
                         experts_per_token=2,
                         notes="mistral_tiny plus a mixture-of-experts MLP (4 experts, top-2, capacity 1.25) for tests"),
    # Mixtral 8x7B: mistral_7b's attention without the window, 8 experts of width 14336, top-2, 32768 tokens.
    "mixtral_8x7b": LMConfig("mixtral_8x7b", 32, 4096, 32, 14336, 32000, 32768, dropout=0.0, activation="swiglu",
                             norm_first=True, causal=True, scale_embedding=False, act_dropout=0.0, norm="rms",
                             bias=False, rope=True, rope_base=1000000.0, positions="none", n_kv_heads=8,
                             n_experts=8, experts_per_token=2,
                             notes="Mixtral 8x7B's block; the decoder is untied and keeps its (zero-initialised) "
                                   "bias"),
    # Qwen3-30B-A3B: 48 layers, 32 query heads over 4 K/V heads of width 128 on d_model 2048, QK-norm, 128 experts of
    # width 768, top-8.
    "qwen3_30b_a3b": LMConfig("qwen3_30b_a3b", 48, 2048, 32, 768, 151936, 32768, dropout=0.0, activation="swiglu",
                              norm_first=True, causal=True, scale_embedding=False, act_dropout=0.0, norm="rms",
                              bias=False, rope=True, rope_base=1000000.0, positions="none", n_kv_heads=4,
                              head_dim=128, qk_norm=True, n_experts=128, experts_per_token=8,
                              notes="Qwen3-30B-A3B's block; the decoder is untied and keeps its (zero-initialised) "
                                    "bias"),
}


class _ConfigTable(dict):
    """``CONFIGS``: a dict of the dense configs that also answers for the mixture-of-experts ones by name.

    ``CONFIGS[name]``, ``name in CONFIGS`` and ``CONFIGS.get(name)`` know every config, :data:`MOE_CONFIGS`
    included (``bench.py --config moe_tiny``).  Iterating it (``keys``, ``items``, ``values``, ``len``) lists the
    dense configs alone: code that sweeps the table relies on every entry's layer being the four units ``core,
    out, mlp_in, mlp_out`` (or Gemma-2's ``core_global``), which a mixture-of-experts layer is not.  Sweep
    ``MOE_CONFIGS`` as well where those are wanted."""

    def __missing__(self, name):
        return MOE_CONFIGS[name]

    def __contains__(self, name) -> bool:
        return dict.__contains__(self, name) or name in MOE_CONFIGS

    def get(self, name, default=None):
        return self[name] if name in self else default


CONFIGS = _ConfigTable({
    # BASELINE.json config #2/#3: 12-layer TransformerEncoder d_model=4096 nhead=16.
    # dim_feedforward = d_model and dropout 0.2 follow the reference driver's
    # convention (main.py:116-120: nhid = emsize, dropout = 0.2); the LM
    # front/back end and vocabulary are the driver's (WikiText-2, 28,782 tokens).
    "enc12_d4096": LMConfig("enc12_d4096", 12, 4096, 16, 4096, 28782, 128,
                            notes="post-norm ReLU TransformerEncoder, FF=d_model, LM head as main.py"),
    # The reference's own run (main.py): 16 layers, d=2048, 32 heads, FF=2048.
    "ref_main": LMConfig("ref_main", 16, 2048, 32, 2048, 28782, 128, notes="reference main.py model"),
    # BASELINE.json config #4: GPT-2-XL 1.5B (pre-norm, causal, GELU, learned positions).
    "gpt2_xl": LMConfig("gpt2_xl", 48, 1600, 25, 6400, 50257, 1024, dropout=0.1, activation="gelu",
                        norm_first=True, causal=True, learned_positions=True, scale_embedding=False,
                        act_dropout=0.0,
                        notes="GPT-2's block: attention / residual / embedding dropout 0.1, none after the GELU"),
    # Tiny config for smoke tests.
    "tiny": LMConfig("tiny", 2, 256, 4, 512, 1000, 64, dropout=0.1),
    # LLaMA-style block: pre-norm RMSNorm, SwiGLU MLP, rotary positions, no biases, causal.
    "llama_tiny": LMConfig("llama_tiny", 2, 256, 4, 512, 1000, 64, dropout=0.0, activation="swiglu",
                           norm_first=True, causal=True, scale_embedding=False, act_dropout=0.0, norm="rms",
                           bias=False, rope=True, positions="none", notes="tiny LLaMA-style model for tests"),
    # llama_tiny with grouped-query attention: 4 query heads share 2 K/V heads (head dim 64).
    "llama_gqa_tiny": LMConfig("llama_gqa_tiny", 2, 256, 4, 512, 1000, 64, dropout=0.0, activation="swiglu",
                               norm_first=True, causal=True, scale_embedding=False, act_dropout=0.0, norm="rms",
                               bias=False, rope=True, positions="none", n_kv_heads=2,
                               notes="tiny LLaMA-style model with grouped-query attention for tests"),
    # LLaMA-2 7B: full multi-head attention (32 query = 32 key/value heads).
    "llama2_7b": LMConfig("llama2_7b", 32, 4096, 32, 11008, 32000, 4096, dropout=0.0, activation="swiglu",
                          norm_first=True, causal=True, scale_embedding=False, act_dropout=0.0, norm="rms",
                          bias=False, rope=True, positions="none",
                          notes="LLaMA-2 7B's block; the decoder keeps its (zero-initialised) bias"),
    # LLaMA-3 8B: 32 query heads over 8 K/V heads (groups of 4), a 128,256-token vocabulary, rope base 500,000.
    "llama3_8b": LMConfig("llama3_8b", 32, 4096, 32, 14336, 128256, 8192, dropout=0.0, activation="swiglu",
                          norm_first=True, causal=True, scale_embedding=False, act_dropout=0.0, norm="rms",
                          bias=False, rope=True, rope_base=500000.0, positions="none", n_kv_heads=8,
                          notes="LLaMA-3 8B's block; the decoder is untied and keeps its (zero-initialised) bias"),
    # llama_gqa_tiny with sliding-window attention: at head dim 64 and 192 tokens a window of 48 skips key tiles
    # on both sides of the band.
    "mistral_tiny": LMConfig("mistral_tiny", 2, 256, 4, 512, 1000, 192, dropout=0.0, activation="swiglu",
                             norm_first=True, causal=True, scale_embedding=False, act_dropout=0.0, norm="rms",
                             bias=False, rope=True, positions="none", n_kv_heads=2, window=48,
                             notes="tiny Mistral-style model (grouped-query, sliding-window attention) for tests"),
    # Mistral 7B v0.1: llama3_8b's block with a 32,000-token vocabulary, rope base 10,000 and a 4096-key window.
    "mistral_7b": LMConfig("mistral_7b", 32, 4096, 32, 14336, 32000, 8192, dropout=0.0, activation="swiglu",
                           norm_first=True, causal=True, scale_embedding=False, act_dropout=0.0, norm="rms",
                           bias=False, rope=True, rope_base=10000.0, positions="none", n_kv_heads=8, window=4096,
                           notes="Mistral 7B's block; the decoder is untied and keeps its (zero-initialised) bias"),
    # mistral_tiny with Gemma-2's two soft caps (50 on the attention scores, 30 on the output logits); the rest of
    # the Gemma-2 block is in gemma2_block_tiny below.
    "gemma2_tiny": LMConfig("gemma2_tiny", 2, 256, 4, 512, 1000, 192, dropout=0.0, activation="swiglu",
                            norm_first=True, causal=True, scale_embedding=False, act_dropout=0.0, norm="rms",
                            bias=False, rope=True, positions="none", n_kv_heads=2, window=48, attn_softcap=50.0,
                            final_softcap=30.0,
                            notes="mistral_tiny plus Gemma-2's soft caps: attention scores at 50, output logits at "
                                  "30 (the Gemma-2 block itself -- head dim of its own, GeGLU, sandwich norms, local / "
                                  "global layers -- is gemma2_block_tiny)"),
    # mistral_tiny with attention sinks: every query head has a learned logit in its softmax's denominator, under
    # the grouped-query heads and the window (gpt-oss's attention; its QKV bias, YaRN, expert biases and clamped
    # SwiGLU are not here; the MoE MLP itself is moe_tiny's).
    "sink_tiny": LMConfig("sink_tiny", 2, 256, 4, 512, 1000, 192, dropout=0.0, activation="swiglu",
                          norm_first=True, causal=True, scale_embedding=False, act_dropout=0.0, norm="rms",
                          bias=False, rope=True, positions="none", n_kv_heads=2, window=48, attn_sinks=True,
                          notes="mistral_tiny plus attention sinks (one learned logit per query head) for tests"),
    # llama_gqa_tiny with QK-norm: every Q and K head RMS-normalised before the rotation.
    "qwen3_tiny": LMConfig("qwen3_tiny", 2, 256, 4, 512, 1000, 64, dropout=0.0, activation="swiglu",
                           norm_first=True, causal=True, scale_embedding=False, act_dropout=0.0, norm="rms",
                           bias=False, rope=True, positions="none", n_kv_heads=2, qk_norm=True,
                           notes="tiny Qwen3-style model (grouped-query attention, QK-norm) for tests"),
    # Qwen3 8B: 36 layers, 32 query heads over 8 K/V heads of width 128, QK-norm, rope base 1,000,000.
    "qwen3_8b": LMConfig("qwen3_8b", 36, 4096, 32, 12288, 151936, 32768, dropout=0.0, activation="swiglu",
                         norm_first=True, causal=True, scale_embedding=False, act_dropout=0.0, norm="rms",
                         bias=False, rope=True, rope_base=1000000.0, positions="none", n_kv_heads=8, qk_norm=True,
                         notes="Qwen3 8B's block; the decoder is untied and keeps its (zero-initialised) bias"),
    # The Gemma-2 block at test size: heads of 128 on d_model 256 (A = 512 != E), GeGLU, sandwich norms, layers 0 and
    # 2 local (48 keys) and 1 and 3 global, both soft caps, the embedding scaled by sqrt(E).  attn_scale is
    # (d_model / nhead) ** -0.5 as in the 27B model, not 128 ** -0.5, so a dropped argument shows.
    "gemma2_block_tiny": LMConfig("gemma2_block_tiny", 4, 256, 4, 512, 1000, 192, **_GEMMA2, n_kv_heads=2,
                                  head_dim=128, window=48, attn_scale=0.125,
                                  notes="tiny Gemma-2 block for tests.  " + _GEMMA2_NOTE),
    # Gemma-2 2B / 9B / 27B: 256,000 tokens, 8192 positions, every second layer global, the others a 4096-key window.
    "gemma2_2b": LMConfig("gemma2_2b", 26, 2304, 8, 9216, 256000, 8192, **_GEMMA2, n_kv_heads=4, head_dim=256,
                          window=4096, notes="Gemma-2 2B's block.  " + _GEMMA2_NOTE),
    "gemma2_9b": LMConfig("gemma2_9b", 42, 3584, 16, 14336, 256000, 8192, **_GEMMA2, n_kv_heads=8, head_dim=256,
                          window=4096, notes="Gemma-2 9B's block.  " + _GEMMA2_NOTE),
    # 27B: query_pre_attn_scalar is d_model / nhead = 144, not the head dim 128
    "gemma2_27b": LMConfig("gemma2_27b", 46, 4608, 32, 36864, 256000, 8192, **_GEMMA2, n_kv_heads=16, head_dim=128,
                           window=4096, attn_scale=144 ** -0.5, notes="Gemma-2 27B's block.  " + _GEMMA2_NOTE),
})


def build_lm_blocks(cfg: LMConfig, *, device=None, dtype=None) -> List[nn.Module]:
    """``[Encoder, attn0, mlp0, attn1, mlp1, ..., (FinalNorm), Decoder]``; with ``cfg.n_experts`` every ``mlp`` is a
    :class:`~mipipe.models.transformer.MoEFeedForwardBlock`."""
    blocks: List[nn.Module] = [
        Encoder(cfg.vocab, cfg.d_model, cfg.dropout, max_len=max(cfg.seq_len, 1024),
                positions=cfg.encoder_positions(), scale_embedding=cfg.scale_embedding,
                device=device, dtype=dtype)
    ]
    blocks += transformer_blocks(cfg.num_layers, cfg.d_model, cfg.nhead, cfg.dim_feedforward, cfg.dropout,
                                 cfg.activation, norm_first=cfg.norm_first, causal=cfg.causal, norm=cfg.norm,
                                 bias=cfg.bias, rope=cfg.rope, rope_base=cfg.rope_base, n_kv_heads=cfg.n_kv_heads,
                                 window=cfg.window, qk_norm=cfg.qk_norm, attn_softcap=cfg.attn_softcap,
                                 sandwich_norm=cfg.sandwich_norm, head_dim=cfg.head_dim, attn_scale=cfg.attn_scale,
                                 global_every=cfg.global_every, attn_sinks=cfg.attn_sinks, n_experts=cfg.n_experts,
                                 experts_per_token=cfg.experts_per_token, capacity_factor=cfg.capacity_factor,
                                 moe_aux_coef=cfg.moe_aux_coef, expert_gemm=cfg.expert_gemm, device=device,
                                 dtype=dtype)
    if cfg.act_dropout is not None:
        for b in blocks:
            if isinstance(b, FeedForwardBlock):
                b.fc_in.dropout = cfg.act_dropout
    if cfg.norm_first:
        blocks.append(FinalNorm(cfg.d_model, norm=cfg.norm, device=device, dtype=dtype))
    blocks.append(Decoder(cfg.vocab, cfg.d_model, final_softcap=cfg.final_softcap, device=device, dtype=dtype))
    return blocks


class TargetSequential(nn.Sequential):
    """``nn.Sequential`` that also hands the micro-batch targets to the children
    that want them (``wants_target``: the vocabulary-split decoder units)."""

    @property
    def wants_target(self) -> bool:
        return any(getattr(m, "wants_target", False) for m in self)

    @property
    def fused_loss(self) -> bool:
        return len(self) > 0 and getattr(self[-1], "fused_loss", False)

    def forward(self, x, target=None):  # type: ignore[override]
        for m in self:
            x = m(x, target) if getattr(m, "wants_target", False) else m(x)
        return x


def lm_pipeline_units(blocks: List[nn.Module], *, split_decoder: bool = False) -> List[nn.Module]:
    """:func:`~mipipe.models.transformer.pipeline_units` of an LM, optionally with
    the decoder cut along the vocabulary (:mod:`mipipe.models.vocab_split`)."""
    from .transformer import pipeline_units
    from .vocab_split import split_decoder as _split

    units = pipeline_units(blocks)
    # a soft-capped decoder is not split: the vocabulary-split kernels fuse the row statistics and know no cap
    if split_decoder and isinstance(units[-1], Decoder) and units[-1].final_softcap is None:
        head, tail = _split(units[-1])
        units = units[:-1] + [head, tail]
    return units
