"""Bit digest of the GEMMs: one sha256 line per case over every tensor the case writes.

    python tools/gemm_digest.py > digest.txt

The cases walk the branches of the launch plan (``gemm_plan`` in ``mipipe/csrc/kernels/gemm.hip``) at the smallest
shape that reaches each: the 128x128 kernel, edge tiles, every epilogue variant of the 256-row kernel at both block
widths (the staged epilogue, the A^T emission, the three side operands, both bias-gradient folds), forced split-K
with its three reductions, per-round launches cut along N and along M, and the three fp32 tiles; then one layer
through ``ops.linear``.  Inputs are made on the CPU from a fixed seed and ``torch.manual_seed`` runs before each
case, so two builds that launch alike print the same lines: run it at two commits on one machine and ``diff`` the
outputs.  Under ``rocprofv3 --kernel-trace --stats`` the per-kernel call counts name the template variants taken.
"""
from __future__ import annotations

import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mipipe import ops  # noqa: E402
from mipipe._native_loader import kernels  # noqa: E402

DEV = torch.device("cuda", 0)
BF, F32 = torch.bfloat16, torch.float32
k = kernels()
gen = torch.Generator()


def rnd(*shape, dtype=BF):
    return torch.randn(*shape, generator=gen).to(dtype).to(DEV)


def sha(t) -> str:
    if t is None or not isinstance(t, torch.Tensor):
        return "-"
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]


def case(name: str, f) -> None:
    gen.manual_seed(1234)
    torch.manual_seed(7)
    out = f()
    torch.cuda.synchronize()
    print(f"{name:<40} " + " ".join(sha(t) for t in (out if isinstance(out, (tuple, list)) else (out,))), flush=True)


def fwd(M, N, K, act=0, p=0.0, bias=True, pre=False, res=False, xt=False, bits=False, dtype=BF):
    x, w = rnd(M, K, dtype=dtype), rnd(N, K, dtype=dtype)
    b = rnd(N, dtype=dtype) if bias else None
    r = rnd(M, N, dtype=dtype) if res else None
    xt_out = torch.zeros(K, M, dtype=dtype, device=DEV) if xt else None
    bits_out = torch.zeros(M, N // 8, dtype=torch.uint8, device=DEV) if bits else None
    y, aux, _, _ = k.linear_fwd(x, w, b, act, p, pre, r, xt_out, False, bits_out)
    return y, aux, xt_out, bits_out


def dgrad(M, N, K, res=False, act=0, p=0.0):
    """dx [M, K] = dy [M, N] . w [N, K], with the activation backward of ``act`` from a forward made here."""
    dy, w = rnd(M, N), rnd(N, K)
    r = rnd(M, K) if res else None
    saved, seed, off = None, 0, 0
    if act:  # the producer's forward: its saved tensor (output, pre-activation, GELU' or bit mask) and dropout draw
        bits = torch.zeros(M, K // 8, dtype=torch.uint8, device=DEV) if act == 4 else None
        y, aux, seed, off = k.linear_fwd(rnd(M, 64), rnd(K, 64), rnd(K), 1 if act in (1, 4) else 2, p, act in (2, 3),
                                         None, None, act == 3, bits)
        saved = {1: y, 2: aux, 3: aux, 4: bits}[act]
    return k.linear_dgrad(dy, w, r, None, act, saved, p, seed, off)


def wgrad1(N, Kin, T):
    main = rnd(N, Kin, dtype=F32)
    k.linear_wgrad(rnd(T, N), rnd(T, Kin), main, True)
    return main


def wgrad(N, Kin, T, nseg, xt=False, fold=False, accumulate=True):
    dys = [rnd(T, N) for _ in range(nseg)]
    xs = [rnd(Kin, T) if xt else rnd(T, Kin) for _ in range(nseg)]
    main, bg = rnd(N, Kin, dtype=F32), rnd(N, dtype=F32) if fold else None
    folded = (k.linear_wgrad_xt_segments if xt else k.linear_wgrad_segments)(dys, xs, main, accumulate, bg)
    assert folded == fold, "the bias-gradient fold was refused"
    return main, bg


def main() -> None:
    # the 128x128 kernel (exact multiples of 128, a grid too small for 256-row tiles), all three operand layouts
    case("small_fwd_128x128x64", lambda: fwd(128, 128, 64, act=2))
    case("small_dgrad_128x128x64", lambda: dgrad(128, 64, 128))
    case("small_wgrad_128x128x64", lambda: wgrad1(128, 128, 64))
    # edge tiles of the 256-row kernel
    case("edge_fwd_264x600x192", lambda: fwd(264, 600, 192, act=1))
    case("edge_dgrad_264x600x192", lambda: dgrad(264, 192, 600))
    case("edge_wgrad_264x600x192", lambda: wgrad1(264, 600, 192))
    # every variant of the 256-row kernel at one tile (200 rows: not the 128x128 kernel's), both widths
    for width in (128, 256):
        k.gemm_set_width(width)
        try:
            t = f"w{width}"
            case(f"plain_{t}", lambda: fwd(200, 256, 64, bias=False))
            case(f"gelu_{t}", lambda: fwd(200, 256, 64, act=2))
            case(f"extra_dropout_{t}", lambda: fwd(200, 256, 64, act=2, p=0.1))
            case(f"extra_aux_{t}", lambda: fwd(200, 256, 64, act=2, pre=True))
            case(f"extra_bits_{t}", lambda: fwd(200, 256, 64, act=1, p=0.1, bits=True))
            case(f"emit_{t}", lambda: fwd(200, 256, 128, act=1, xt=True))
            case(f"emit_extra_{t}", lambda: fwd(200, 256, 128, act=1, p=0.1, xt=True))
            case(f"side_res_fwd_{t}", lambda: fwd(200, 256, 64, res=True))
            case(f"side_res_emit_{t}", lambda: fwd(200, 256, 128, res=True, xt=True))
            case(f"side_res_dgrad_{t}", lambda: dgrad(200, 64, 256, res=True))
            case(f"side_bits_{t}", lambda: dgrad(200, 64, 256, act=4, p=0.1))
            case(f"side_bits_res_{t}", lambda: dgrad(200, 64, 256, res=True, act=4, p=0.1))
            case(f"side_saved_relu_{t}", lambda: dgrad(200, 64, 256, act=1, p=0.1))
            case(f"side_saved_gelu_{t}", lambda: dgrad(200, 64, 256, act=2, p=0.1))
            case(f"side_saved_grad_{t}", lambda: dgrad(200, 64, 256, act=3, p=0.1))
            case(f"wgrad_segments_{t}", lambda: wgrad(200, 256, 64, 3))
            case(f"wgrad_xt_segments_{t}", lambda: wgrad(200, 256, 64, 3, xt=True))
            case(f"colsum_fold_{t}", lambda: wgrad(256, 256, 64, 2, xt=True, fold=True))
            case(f"rowsum_fold_{t}", lambda: wgrad(256, 16 * width, 64, 2, fold=True))
        finally:
            k.gemm_set_width(0)
    # forced split-K: 132 K-tiles of 11 per segment, the three reductions (fp32, transposed + column sums, bf16 + res)
    for splits in (5, 7):
        k.gemm_set_splitk(splits)
        try:
            case(f"splitk{splits}_wgrad", lambda: wgrad(256, 256, 704, 12, accumulate=False))
            case(f"splitk{splits}_wgrad_xt_colsum", lambda: wgrad(256, 256, 704, 12, xt=True, fold=True))
            case(f"splitk{splits}_dgrad_res", lambda: dgrad(200, 8448, 256, res=True))
        finally:
            k.gemm_set_splitk(1)
    case("splitk_auto_dgrad_264x256x8192", lambda: dgrad(264, 8192, 256))
    # per-round launches: 2 x 129 = 258 tiles, cut along N (only the first chunk emits A^T) and along M
    k.gemm_set_rounds(2)
    try:
        case("rounds_along_n", lambda: fwd(264, 129 * 256, 64, act=1, p=0.1, xt=True, bits=True))
        case("rounds_along_n_res", lambda: fwd(264, 129 * 256, 64, res=True, xt=True))
        case("rounds_along_m", lambda: dgrad(129 * 256, 64, 264, res=True, act=4, p=0.1))
    finally:
        k.gemm_set_rounds(1)
    case("rounds_default_short_k", lambda: fwd(264, 129 * 256, 64, act=1))  # K < 4096: one launch
    # fp32: the 64x128 tile, the 128x64 tile, the 128x128 tile; and the activation epilogue
    case("f32_wide_128x128x64", lambda: k.gemm_f32(rnd(128, 64, dtype=F32), rnd(128, 64, dtype=F32), True, True))
    case("f32_tall_64x128x64", lambda: k.gemm_f32(rnd(64, 64, dtype=F32), rnd(64, 128, dtype=F32), False, False))
    case("f32_big_2048x4096x64", lambda: k.gemm_f32(rnd(2048, 64, dtype=F32), rnd(64, 4096, dtype=F32), True, False))
    case("f32_fwd_gelu_264x600x192", lambda: fwd(264, 600, 192, act=2, p=0.1, pre=True, res=True, dtype=F32))

    def layer():  # the public op: forward, dgrad and the weight / bias gradients of autograd
        x, w, b = rnd(264, 192).requires_grad_(), rnd(600, 192).requires_grad_(), rnd(600).requires_grad_()
        y = ops.linear(x, w, b, "gelu", 0.1, True)
        y.backward(rnd(264, 600))
        return y, x.grad, w.grad, b.grad

    case("ops_linear_264x600x192", layer)


if __name__ == "__main__":
    main()
