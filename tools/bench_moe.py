"""The mixture-of-experts kernels and block, timed in ONE process with interleaved rounds (so every call of a
group sees the same clocks and the same neighbours on the box), bf16:

* gathers: ``moe_gather_slots`` (dispatch), ``moe_gather_tokens`` (combine, k = 2, with the residual) and
  ``moe_combine_bwd`` at T 8192, E 4096, 8 experts, C 2560, next to ``bias_act``'s plain copy of a ``[T, E]``
  tensor; every rate is bytes actually moved (occupied rows read, every row written) over the median time, and
  the copy's own quartile spread stands next to them;
* routing: ``moe_route_fwd`` + ``moe_assign`` at ``[8192, 8]`` (k 2) and ``[8192, 128]`` (k 8) against the eager
  reference composition (sort, softmax, one-hot cumulative sum, scatter) on the same device;
* block: ``MoEFeedForwardBlock`` forward + backward at Mixtral's layer shape (E 4096, F 14336, 8 experts, top-2,
  T 8192) at ``capacity_factor`` 1.0 and 1.25 against the dense SwiGLU ``FeedForwardBlock`` on 2 T rows (the same
  useful GEMM work), and the routing ops of that shape (route, assign, dispatch, combine and their backwards)
  timed alone, as a share of the block.

    python tools/bench_moe.py [--rounds 20] [--sections gather,route,block] [--out FILE]

Times are device events around single calls, medians over the rounds, with the quartiles as the spread.  Nothing
is fixed in advance: the file records what was measured.  Needs a GPU: there is no CPU fallback.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_rowwise_llama import _clock, _time_interleaved  # noqa: E402


def _stat(ts):
    return statistics.median(ts), ts[len(ts) // 4], ts[(3 * len(ts)) // 4]


def _logits(T, Ne, dev):
    g = torch.Generator().manual_seed(0)
    return (torch.randn(T, Ne, generator=g) + torch.linspace(-1, 1, Ne)).to(torch.bfloat16).to(dev)


def gather_section(k, ops, rounds, lines):
    dev, bf = "cuda", torch.bfloat16
    T, E, Ne, kk, C = 8192, 4096, 8, 2, 2560
    g = torch.Generator(device=dev).manual_seed(7)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g).to(bf)  # noqa: E731
    idx, gate, _ = ops.moe_route(_logits(T, Ne, dev), kk)
    slot, src, counts = ops.moe_assign(idx, Ne, C)
    filled, kept = int((src >= 0).sum()), int((slot >= 0).sum())
    x, ye, dy = rn(T, E), rn(Ne * C, E), rn(T, E)
    row = E * 2
    res = _time_interleaved({
        "copy": lambda: k.bias_act_fwd(x, None, 0, 0.0),
        "gather_slots": lambda: k.moe_gather_slots(x, src, kk),
        "gather_tokens": lambda: k.moe_gather_tokens(ye, slot, gate, x),
        "gather_tokens_plain": lambda: k.moe_gather_tokens(ye, slot),
        "combine_bwd": lambda: k.moe_combine_bwd(dy, ye, gate, src),
    }, rounds)
    nbytes = {"copy": 2 * T * row, "gather_slots": (filled + Ne * C) * row, "gather_tokens": (kept + 2 * T) * row,
              "gather_tokens_plain": (kept + T) * row, "combine_bwd": (3 * filled + (Ne * C - filled)) * row}
    lines.append(f"# gathers: T {T}, E {E}, {Ne} experts, k {kk}, C {C}: {filled} of {Ne * C} slots filled, "
                 f"{kept} of {T * kk} choices kept, counts {counts.tolist()}")
    lines.append("# kernel                                median      [quartiles]        bytes moved   rate       q3 / q1")
    for name, ts in res.items():
        m, q1, q3 = _stat(ts)
        lines.append(f"{name:34s} {m:9.1f} us  [{q1:8.1f}, {q3:8.1f}]  {nbytes[name] / 1e6:9.1f} MB  "
                     f"{nbytes[name] / m / 1e6:6.2f} TB/s  {q3 / q1:7.3f}")


def route_section(k, ops, rounds, lines):
    from mipipe.ops import moe as M

    dev = "cuda"
    lines.append("# routing: moe_route_fwd + moe_assign against the eager reference composition")
    lines.append("# shape                                 native      [quartiles]        eager       [quartiles]      eager / native")
    for T, Ne, kk in ((8192, 8, 2), (8192, 128, 8)):
        C = ops.moe_capacity(T, Ne, kk, 1.25)
        lg = _logits(T, Ne, dev)

        def native():
            idx, _, _ = k.moe_route_fwd(lg, kk)
            k.moe_assign(idx, Ne, C)

        def eager():
            idx, _, _ = M.moe_route_reference(lg, kk)
            M.moe_assign_reference(idx, Ne, C)

        res = _time_interleaved({"native": native, "eager": eager}, rounds)
        n, n1, n3 = _stat(res["native"])
        e, e1, e3 = _stat(res["eager"])
        lines.append(f"{f'[{T}, {Ne}] k {kk} C {C}':34s} {n:9.1f} us  [{n1:8.1f}, {n3:8.1f}]  {e:9.1f} us  "
                     f"[{e1:8.1f}, {e3:8.1f}]  {e / n:8.1f}")


def block_section(k, ops, rounds, lines):
    from mipipe.models.transformer import FeedForwardBlock, MoEFeedForwardBlock
    from mipipe.optim import FlatAdam

    dev, bf = "cuda", torch.bfloat16
    T, E, F, Ne, kk = 8192, 4096, 14336, 8, 2
    g = torch.Generator(device=dev).manual_seed(7)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g).to(bf)  # noqa: E731
    lines.append(f"# block: forward + backward, T {T}, E {E}, F {F}, {Ne} experts, top-{kk}; dense: SwiGLU "
                 f"FeedForwardBlock on {2 * T} rows (the same useful GEMM work)")
    torch.manual_seed(0)
    dense = FeedForwardBlock(E, F, 0.0, "swiglu", norm_first=True, norm="rms", bias=False).to(dev, bf).train()
    dopt = FlatAdam(dense.parameters(), lr=0.0)
    xd, dyd = rn(1, 2 * T, E).requires_grad_(), rn(1, 2 * T, E)

    def run(mod, opt, x, dy):
        def f():
            opt.zero_grad()
            mod(x).backward(dy)
        return f

    calls = {"dense 2T": run(dense, dopt, xd, dyd)}
    x, dy = rn(1, T, E).requires_grad_(), rn(1, T, E)
    blocks = {}
    for cf in (1.0, 1.25):
        torch.manual_seed(0)
        blk = MoEFeedForwardBlock(E, F, Ne, kk, capacity_factor=cf).to(dev, bf).train()
        blocks[cf] = blk
        calls[f"moe cf {cf}"] = run(blk, FlatAdam(blk.parameters(), lr=0.0), x, dy)
    res = _time_interleaved(calls, rounds, warmup=3)
    d, d1, d3 = _stat(res["dense 2T"])
    lines.append("# call                                  median      [quartiles]        / dense    dense q3 / q1")
    lines.append(f"{'dense 2T':34s} {d / 1e3:9.2f} ms  [{d1 / 1e3:8.2f}, {d3 / 1e3:8.2f}]")
    for cf, blk in blocks.items():
        m, m1, m3 = _stat(res[f"moe cf {cf}"])
        lines.append(f"{f'moe cf {cf} (C {ops.moe_capacity(T, Ne, kk, cf)})':34s} {m / 1e3:9.2f} ms  "
                     f"[{m1 / 1e3:8.2f}, {m3 / 1e3:8.2f}]  {m / d:8.3f}   {d3 / d1:8.3f}   drop "
                     f"{float(blk.last_drop_fraction):.3f} aux {float(blk.last_aux):.3f}")
    # the routing ops of this shape alone (what the block adds to the experts' GEMMs and gate passes)
    C = ops.moe_capacity(T, Ne, kk, 1.25)
    x2, ye, dy2 = rn(T, E), rn(Ne * C, E), rn(T, E)
    lg = _logits(T, Ne, dev)
    idx, gate, _ = k.moe_route_fwd(lg, kk)
    slot, src, _ = k.moe_assign(idx, Ne, C)
    dgate = torch.randn(T, kk, device=dev, generator=g)
    dprobs = torch.rand(Ne, device=dev, generator=g)

    def routing():
        i, _, _ = k.moe_route_fwd(lg, kk)
        k.moe_assign(i, Ne, C)
        k.moe_gather_slots(x2, src, kk)
        k.moe_gather_tokens(ye, slot, gate, x2)
        k.moe_combine_bwd(dy2, ye, gate, src)
        k.moe_gather_tokens(ye, slot)
        k.moe_route_bwd(lg, idx, gate, dgate, dprobs)

    r, r1, r3 = _stat(_time_interleaved({"routing": routing}, rounds)["routing"])
    m = statistics.median(res["moe cf 1.25"])
    lines.append(f"{'routing ops alone (cf 1.25)':34s} {r / 1e3:9.2f} ms  [{r1 / 1e3:8.2f}, {r3 / 1e3:8.2f}]  "
                 f"{r / m:8.3f} of the block")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--sections", default="gather,route,block")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_moe.py measures GPU kernels: no GPU found")
    from mipipe import ops
    from mipipe._native_loader import kernels

    k = kernels()
    lines = [f"# tools/bench_moe.py --rounds {args.rounds} --sections {args.sections}",
             f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}, {time.strftime('%Y-%m-%d %H:%M:%S')}",
             f"# clock: {_clock()}; {args.rounds} interleaved rounds per group after warm-up rounds; bf16"]
    sections = {"gather": gather_section, "route": route_section, "block": block_section}
    for name in args.sections.split(","):
        sections[name](k, ops, args.rounds, lines)
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
