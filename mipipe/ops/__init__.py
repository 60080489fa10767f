"""MI355X compute ops used by ``mipipe.models``.

Each op has one GPU implementation -- a hand-written CDNA4 HIP kernel in
``mipipe/csrc/kernels`` -- and an eager CPU implementation used only for
CPU tensors (plumbing tests).  GPU tensors never fall back to eager PyTorch:
a missing extension raises (``mipipe._native_loader.kernels``).
"""
from .layernorm import add_dropout_layer_norm, layer_norm_fanout, layer_norm_reference
from .rmsnorm import (add_dropout_rms_norm, rms_norm_fanout, rms_norm_reference, rms_norm_residual,
                      rms_norm_residual_reference)
from .linear import deferred_wgrad, flush_wgrad, linear, linear_fanout, linear_residual
from .attention import (attention, attention_gqa_packed, attention_packed, attention_reference, check_doc_bounds,
                        current_documents, use_documents)
from .activation import bias_act_dropout
from .softcap import softcap, softcap_owned, softcap_reference
from .swiglu import swiglu, swiglu_reference
from .geglu import geglu, geglu_reference
from .rope import rope_heads, rope_packed, rope_projection, rope_reference, rope_tables
from .qknorm import qk_norm_rope_heads, qk_norm_rope_projection, qk_norm_rope_reference
from .moe import (moe_assign, moe_assign_reference, moe_assign_sorted, moe_assign_sorted_reference, moe_attach_aux,
                  moe_capacity, moe_combine, moe_combine_reference, moe_dispatch, moe_dispatch_reference, moe_route,
                  moe_route_reference, moe_sorted_rows)
from .grouped_linear import grouped_linear, grouped_linear_reference
from .loss import cross_entropy
from .embedding import embed_scale_posenc_dropout

__all__ = [
    "add_dropout_layer_norm",
    "layer_norm_fanout",
    "layer_norm_reference",
    "add_dropout_rms_norm",
    "rms_norm_fanout",
    "rms_norm_reference",
    "rms_norm_residual",
    "rms_norm_residual_reference",
    "linear",
    "linear_fanout",
    "linear_residual",
    "deferred_wgrad",
    "flush_wgrad",
    "attention",
    "attention_packed",
    "attention_gqa_packed",
    "attention_reference",
    "check_doc_bounds",
    "use_documents",
    "current_documents",
    "bias_act_dropout",
    "softcap",
    "softcap_owned",
    "softcap_reference",
    "swiglu",
    "swiglu_reference",
    "geglu",
    "geglu_reference",
    "rope_tables",
    "rope_packed",
    "rope_projection",
    "rope_heads",
    "rope_reference",
    "qk_norm_rope_heads",
    "qk_norm_rope_projection",
    "qk_norm_rope_reference",
    "moe_route",
    "moe_assign",
    "moe_dispatch",
    "moe_combine",
    "moe_capacity",
    "moe_attach_aux",
    "moe_route_reference",
    "moe_assign_reference",
    "moe_dispatch_reference",
    "moe_combine_reference",
    "moe_assign_sorted",
    "moe_assign_sorted_reference",
    "moe_sorted_rows",
    "grouped_linear",
    "grouped_linear_reference",
    "cross_entropy",
    "embed_scale_posenc_dropout",
]
