"""Bit digest of the attention ops: one sha256 line per case for ``o``, the input gradients and ``dsinks``.

    python tools/attention_digest.py > digest.txt

The cases walk every branch of the dispatch in ``mipipe/ops/attention.py`` at its smallest shape (B = 2, H = 4)
through the three entry points: the S = 128, generic and long-sequence kernels, causal end padding, feature padding
with the spare-feature key mask, the fp32 key bound, grouped-query heads in place and repeated, and a window, a soft
cap, document bounds and sinks alone and together, with and without dropout.  Inputs are made on the CPU from a fixed
seed and ``torch.manual_seed`` runs before each case, so two builds that dispatch alike print the same lines: run it
at two commits on one machine and ``diff`` the outputs.  Only the public entry points are used.
"""
from __future__ import annotations

import hashlib
import os
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mipipe import checkpoint  # noqa: E402
from mipipe.ops import attention, attention_gqa_packed, attention_packed  # noqa: E402
from mipipe.ops.attention import clear_keep_words  # noqa: E402
from mipipe.utils.data import document_bounds_from_lengths  # noqa: E402

DEV = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")  # cpu: a dry run of the tool
B, H = 2, 4
BF, F32 = torch.bfloat16, torch.float32


def sha(t) -> str:
    if t is None:
        return "-"
    raw = t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()
    return hashlib.sha256(raw).hexdigest()[:16]


def options(S: int, which: str, gen: torch.Generator):
    """The keyword options of a case: ``which`` holds any of w(indow), c(ap), d(ocuments), s(inks)."""
    kw, sinks = {}, None
    if "w" in which:
        kw["window"] = 48
    if "c" in which:
        kw["softcap"] = 30.0
    if "d" in which:  # three documents a row, cut differently in each row
        a, b = S // 4, S // 2
        kw["doc_bounds"] = document_bounds_from_lengths([[a, b, S - a - b], [b + 1, a - 1, S - a - b]], S, DEV)
    if "s" in which:
        sinks = torch.randn(H, generator=gen)
        sinks[1] = float("-inf")
        sinks = sinks.to(DEV).requires_grad_()
        kw["sinks"] = sinks
    return kw, sinks


def run(name: str, entry: str, dtype, S: int, D: int, causal: bool, p: float, which: str = "", n_kv: int = H,
        ckpt: bool = False) -> None:
    gen = torch.Generator().manual_seed(1234)
    heads = 3 * H if entry == "packed" else H + 2 * n_kv
    if entry == "sep":
        leaves = [torch.randn(B, h, S, D, generator=gen).to(dtype).to(DEV).requires_grad_() for h in (H, n_kv, n_kv)]
    elif entry == "packed":
        leaves = [torch.randn(B, S, 3, H, D, generator=gen).to(dtype).to(DEV).requires_grad_()]
    else:
        leaves = [torch.randn(B, S, heads, D, generator=gen).to(dtype).to(DEV).requires_grad_()]
    kw, sinks = options(S, which, gen)
    g = torch.randn(*((B, H, S, D) if entry == "sep" else (B, S, H, D)), generator=gen).to(dtype).to(DEV)
    if entry == "sep":
        f = lambda *t: attention(*t, causal, p, True, **kw)  # noqa: E731
    elif entry == "packed":
        f = lambda t: attention_packed(t, causal, p, True, **kw)  # noqa: E731
    else:
        f = lambda t: attention_gqa_packed(t, n_kv, causal, p, True, **kw)  # noqa: E731
    clear_keep_words()
    torch.manual_seed(7)
    o = checkpoint(f, leaves[0]) if ckpt else f(*leaves)
    o.backward(g)
    if DEV.type == "cuda":
        torch.cuda.synchronize()
    grads = " ".join(sha(t.grad) for t in leaves)
    print(f"{name:<44} o={sha(o)} d={grads} dsinks={sha(None if sinks is None else sinks.grad)}", flush=True)


def main() -> None:
    warnings.simplefilter("ignore")  # the eager-path notes: the cases below take that path on purpose
    tag = lambda c, p: ("c" if c else "n") + ("_p" if p else "")  # noqa: E731
    for p in (0.0, 0.1):
        for entry in ("packed", "gqa", "sep"):
            n_kv = 2 if entry == "gqa" else H
            for causal in (False, True):
                t = f"{entry}_{tag(causal, p)}"
                run(f"s128_d64_{t}", entry, BF, 128, 64, causal, p, n_kv=n_kv)        # the S = 128 kernels
                run(f"s192_d128_{t}", entry, BF, 192, 128, causal, p, n_kv=n_kv)      # the generic kernels
                run(f"s256_d64_{t}", entry, BF, 256, 64, causal, p, n_kv=n_kv)        # the long-sequence kernels
                if entry != "sep":  # under a checkpoint: the recompute reuses the first forward's keep words
                    run(f"s256_d64_ckpt_{t}", entry, BF, 256, 64, causal, p, n_kv=n_kv, ckpt=True)
                run(f"f32_s64_d64_{t}", entry, F32, 64, 64, causal, p, n_kv=n_kv)
            run(f"s100_d64_pad_{entry}_{tag(True, p)}", entry, BF, 100, 64, True, p, n_kv=n_kv)   # end padding
            run(f"s100_d32_pad_{entry}_{tag(True, p)}", entry, BF, 100, 32, True, p, n_kv=n_kv)   # both paddings
            run(f"s64_d32_pad_{entry}_{tag(False, p)}", entry, BF, 64, 32, False, p, n_kv=n_kv)   # feature padding
            run(f"s72_d32_keymask_{entry}_{tag(False, p)}", entry, BF, 72, 32, False, p, n_kv=n_kv)  # + key mask
            run(f"f32_s72_d64_kvlen_{entry}_{tag(False, p)}", entry, F32, 72, 64, False, p, n_kv=n_kv)  # key bound
            run(f"f32_s100_d64_pad_{entry}_{tag(True, p)}", entry, F32, 100, 64, True, p, n_kv=n_kv)
            # a window, a cap, documents and sinks, alone and together, exact and padded
            for which in ("w", "c", "d", "s", "wc", "ds", "cs", "wcds"):
                for S, D in ((128, 64), (192, 128), (100, 64), (128, 32)):
                    run(f"s{S}_d{D}_{which}_{entry}_{tag(True, p)}", entry, BF, S, D, True, p, which, n_kv=n_kv)
            for which in ("c", "s", "cs"):  # the options that also run without the causal mask
                run(f"s128_d64_{which}_{entry}_{tag(False, p)}", entry, BF, 128, 64, False, p, which, n_kv=n_kv)
                run(f"s64_d32_{which}_{entry}_{tag(False, p)}", entry, BF, 64, 32, False, p, which, n_kv=n_kv)
            run(f"s72_d32_s_keymask_{entry}_{tag(False, p)}", entry, BF, 72, 32, False, p, "s", n_kv=n_kv)
        run(f"gqa_hkv_eq_h_{tag(True, p)}", "gqa", BF, 128, 64, True, p, n_kv=H)  # the same bytes as packed
        run(f"sep_hkv2_s192_d128_wcds_{tag(True, p)}", "sep", BF, 192, 128, True, p, "wcds", n_kv=2)  # repeated K/V
    # no native form: the eager math (p = 0: its dropout is torch's own)
    for entry in ("packed", "gqa", "sep"):
        n_kv = 2 if entry == "gqa" else H
        run(f"eager_s72_d32_cs_{entry}_n", entry, BF, 72, 32, False, 0.0, "cs", n_kv=n_kv)
        run(f"eager_s72_d256_{entry}_n", entry, BF, 72, 256, False, 0.0, n_kv=n_kv)
        run(f"eager_f32_s64_d64_wcds_{entry}_c", entry, F32, 64, 64, True, 0.0, "wcds", n_kv=n_kv)


if __name__ == "__main__":
    main()
