"""The grouped expert GEMMs and the dropless block, timed in ONE process with interleaved rounds (so every call of
a group sees the same clocks and the same neighbours on the box), bf16:

* kernels: ``grouped_gemm_rows`` (forward, dgrad) and ``grouped_gemm_wgrad`` over expert-sorted rows against a loop
  of ``linear_fwd`` / ``linear_dgrad`` / ``linear_wgrad`` over the same experts' rows, for the first expert GEMM
  (``W1 [2F, E]``) of Mixtral's layer (E 4096, F 14336, 8 experts, top-2, T 8192) and of Qwen3-30B-A3B's (E 2048,
  F 768, 128 experts, top-8, T 8192), with balanced counts and with skewed counts (a seeded router whose expert 0
  gets about 4x the mean, or every token where that is less).  The loop runs ``ceil64`` of every expert's count
  (its weight gradient takes whole 64-row K tiles), the grouped kernels ``ceil128``; the TFLOP/s are the USEFUL
  FLOPs, ``2 * sum(counts) * 2F * E``, over the median time.
* block: ``MoEFeedForwardBlock`` forward + backward with ``expert_gemm="grouped"`` against ``"loop"`` at
  ``capacity_factor`` 1.0 and 1.25 and against the dense SwiGLU ``FeedForwardBlock`` on ``k T`` rows, at both
  layer shapes.
* resources: registers, LDS, scratch and occupancy of the new kernels from
  ``hipcc -Rpass-analysis=kernel-resource-usage``.

    python tools/bench_moe_grouped.py [--rounds 20] [--sections kernels,block,resources] [--out FILE]

Times are device events around single calls, medians over the rounds, with the quartiles as the spread.  Nothing
is fixed in advance: the file records what was measured.  Needs a GPU: there is no CPU fallback.
"""
import argparse
import os
import re
import shutil
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_rowwise_llama import _clock, _time_interleaved  # noqa: E402

SHAPES = {"mixtral": (8192, 4096, 14336, 8, 2), "qwen3_30b_a3b": (8192, 2048, 768, 128, 8)}   # T, E, F, Ne, k


def _stat(ts):
    return statistics.median(ts), ts[len(ts) // 4], ts[(3 * len(ts)) // 4]


def _balanced_idx(T, Ne, kk):
    t = torch.arange(T)[:, None]
    return ((t * kk + torch.arange(kk)[None, :]) % Ne).to(torch.int32)


def _skewed_idx(T, Ne, kk, ops):
    """Top-k of seeded logits with a bias on expert 0, bisected so that expert 0 gets min(4 * mean, T) choices."""
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(T, Ne, generator=g)
    want = min(4 * T * kk // Ne, T)
    lo, hi = 0.0, 16.0
    for _ in range(30):
        mid = (lo + hi) / 2
        lg = logits.clone()
        lg[:, 0] += mid
        idx = ops.moe_route(lg, kk)[0]
        if int((idx == 0).sum()) < want:
            lo = mid
        else:
            hi = mid
    return idx


def kernels_section(k, ops, rounds, lines):
    dev, bf = "cuda", torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(7)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g).to(bf)  # noqa: E731
    lines.append("# kernels: the first expert GEMM (W1 [2F, E]); grouped = one launch, loop = one launch per expert "
                 "on ceil64(count) rows; TFLOP/s over the useful FLOPs 2 * sum(counts) * 2F * E")
    lines.append("# shape, counts, kernel                      grouped     [quartiles]       TF/s    loop        "
                 "[quartiles]       TF/s   loop / grouped  loop q3 / q1")
    for name, (T, E, F, Ne, kk) in SHAPES.items():
        N, K = 2 * F, E
        ws = [rn(N, K) * K ** -0.5 for _ in range(Ne)]
        wtab = torch.tensor([w.data_ptr() for w in ws], dtype=torch.int64).to(dev)
        mains = [torch.zeros(N, K, device=dev) for _ in range(Ne)]
        mtab = torch.tensor([m.data_ptr() for m in mains], dtype=torch.int64).to(dev)
        for kind in ("balanced", "skewed"):
            idx = (_balanced_idx(T, Ne, kk) if kind == "balanced" else _skewed_idx(T, Ne, kk, ops)).to(dev)
            slot, src, counts, offsets, tile_expert = ops.moe_assign_sorted(idx, Ne)
            R = src.shape[0]
            x = ops.moe_dispatch(rn(T, K), slot, src)
            dy = rn(R, N)
            off, cnt = offsets.tolist(), counts.tolist()
            rows = [(off[e], off[e] + (c + 63) // 64 * 64) for e, c in enumerate(cnt) if c > 0]
            live = [e for e, c in enumerate(cnt) if c > 0]
            xs = [x[a:b] for a, b in rows]
            dys = [dy[a:b] for a, b in rows]
            flops = 2.0 * sum(cnt) * N * K

            def loop_fwd():
                for e, xe in zip(live, xs):
                    k.linear_fwd(xe, ws[e], None, 0, 0.0, False)

            def loop_dgrad():
                for e, de in zip(live, dys):
                    k.linear_dgrad(de, ws[e])

            def loop_wgrad():
                for e, de, xe in zip(live, dys, xs):
                    k.linear_wgrad(de, xe, mains[e], False)

            calls = {
                "fwd grouped": lambda: k.grouped_gemm_rows(x, wtab, tile_expert, N, True),
                "fwd loop": loop_fwd,
                "dgrad grouped": lambda: k.grouped_gemm_rows(dy, wtab, tile_expert, K, False),
                "dgrad loop": loop_dgrad,
                "wgrad grouped": lambda: k.grouped_gemm_wgrad(dy, x, offsets, mtab, False),
                "wgrad loop": loop_wgrad,
            }
            res = _time_interleaved(calls, rounds, warmup=3)
            lines.append(f"# {name} {kind}: {sum(cnt)} choices in {R} rows ({int(offsets[-1])} in live tiles), counts "
                         f"min {min(cnt)} max {max(cnt)} mean {sum(cnt) / Ne:.0f}")
            for op in ("fwd", "dgrad", "wgrad"):
                gm, g1, g3 = _stat(res[f"{op} grouped"])
                lm, l1, l3 = _stat(res[f"{op} loop"])
                lines.append(f"{f'{name} {kind} {op}':38s} {gm:9.1f} us  [{g1:8.1f}, {g3:8.1f}]  {flops / gm / 1e6:7.1f}  "
                             f"{lm:9.1f} us  [{l1:8.1f}, {l3:8.1f}]  {flops / lm / 1e6:7.1f}  {lm / gm:8.3f}      "
                             f"{l3 / l1:8.3f}")
            del x, dy, xs, dys
        del ws, mains
        torch.cuda.empty_cache()


def block_section(k, ops, rounds, lines):
    from mipipe.models.transformer import FeedForwardBlock, MoEFeedForwardBlock
    from mipipe.optim import FlatAdam

    dev, bf = "cuda", torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(7)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g).to(bf)  # noqa: E731

    def run(mod, opt, x, dy):
        def f():
            opt.zero_grad()
            mod(x).backward(dy)
        return f

    for name, (T, E, F, Ne, kk) in SHAPES.items():
        lines.append(f"# block {name}: forward + backward, T {T}, E {E}, F {F}, {Ne} experts, top-{kk}; dense: SwiGLU "
                     f"FeedForwardBlock on {kk * T} rows (the same useful GEMM work)")
        torch.manual_seed(0)
        dense = FeedForwardBlock(E, F, 0.0, "swiglu", norm_first=True, norm="rms", bias=False, device=dev, dtype=bf)
        dense.train()
        xd, dyd = rn(1, kk * T, E).requires_grad_(), rn(1, kk * T, E)
        calls = {f"dense {kk}T": run(dense, FlatAdam(dense.parameters(), lr=0.0), xd, dyd)}
        x, dy = rn(1, T, E).requires_grad_(), rn(1, T, E)
        blocks = {}
        for label, kw in (("loop cf 1.0", dict(capacity_factor=1.0)), ("loop cf 1.25", dict(capacity_factor=1.25)),
                          ("grouped", dict(capacity_factor=None, expert_gemm="grouped"))):
            torch.manual_seed(0)
            blk = MoEFeedForwardBlock(E, F, Ne, kk, device=dev, dtype=bf, **kw).train()
            blocks[label] = blk
            calls[label] = run(blk, FlatAdam(blk.parameters(), lr=0.0), x, dy)
        res = _time_interleaved(calls, rounds, warmup=3)
        d, d1, d3 = _stat(res[f"dense {kk}T"])
        gm = statistics.median(res["grouped"])
        lines.append("# call                                  median      [quartiles]        / dense   grouped / this   "
                     "this q3 - q1")
        lines.append(f"{f'dense {kk}T':34s} {d / 1e3:9.2f} ms  [{d1 / 1e3:8.2f}, {d3 / 1e3:8.2f}]     1.000  "
                     f"{gm / d:8.3f}      {(d3 - d1) / 1e3:8.3f} ms")
        for label, blk in blocks.items():
            m, m1, m3 = _stat(res[label])
            rows = (ops.moe_sorted_rows(T, Ne, kk) if label == "grouped"
                    else Ne * ops.moe_capacity(T, Ne, kk, blk.capacity_factor))
            lines.append(f"{f'{label} ({rows} rows)':34s} {m / 1e3:9.2f} ms  [{m1 / 1e3:8.2f}, {m3 / 1e3:8.2f}]  "
                         f"{m / d:8.3f}  {gm / m:8.3f}      {(m3 - m1) / 1e3:8.3f} ms   drop "
                         f"{float(blk.last_drop_fraction):.3f} aux {float(blk.last_aux):.3f}")
        l, l1, l3 = _stat(res["loop cf 1.25"])
        lines.append(f"# {name}: loop cf 1.25 - grouped = {(l - gm) / 1e3:.3f} ms, the loop's quartile spread "
                     f"{(l3 - l1) / 1e3:.3f} ms: grouped is {'FASTER' if l - gm > l3 - l1 else 'NOT faster'} "
                     f"beyond the spread (grouped / loop = {gm / l:.3f})")
        del dense, blocks, calls, xd, dyd, x, dy
        torch.cuda.empty_cache()


def resources_section(k, ops, rounds, lines):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "mipipe", "csrc", "kernels", "gemm_grouped.hip")
    cmd = [hipcc, "-std=c++17", "--offload-arch=gfx950", "-O3", "-ffp-contract=fast", "-munsafe-fp-atomics", "-mllvm",
           "-pragma-unroll-threshold=1000000", "--offload-device-only", "-c", src, "-o", os.devnull,
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    lines.append("# resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage on "
                 "gemm_grouped.hip); LDS is dynamic: 65536 bytes per block at launch, 2 blocks per CU")
    lines.append("# kernel                                     SGPRs VGPRs AGPRs scratch waves/SIMD")
    cur = {}
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|"
                      r"Occupancy \[waves/SIMD\]): (\S+)", line)
        if not m:
            continue
        cur[m.group(1)] = m.group(2)
        if m.group(1).startswith("Occupancy"):
            fn = subprocess.run(["c++filt", cur["Function Name"]], capture_output=True, text=True).stdout.strip()
            fn = fn.replace("mipipe::(anonymous namespace)::", "").replace("void ", "")
            fn = re.sub(r"\(.*", "", fn)
            lines.append(f"{fn:44s} {cur['TotalSGPRs']:>5s} {cur['VGPRs']:>5s} {cur['AGPRs']:>5s} "
                         f"{cur['ScratchSize [bytes/lane]']:>7s} {cur['Occupancy [waves/SIMD]']:>10s}")
            cur = {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--sections", default="kernels,block,resources")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_moe_grouped.py measures GPU kernels: no GPU found")
    from mipipe import ops
    from mipipe._native_loader import kernels

    k = kernels()
    lines = [f"# tools/bench_moe_grouped.py --rounds {args.rounds} --sections {args.sections}",
             f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}, {time.strftime('%Y-%m-%d %H:%M:%S')}",
             f"# clock: {_clock()}; {args.rounds} interleaved rounds per group after warm-up rounds; bf16"]
    sections = {"kernels": kernels_section, "block": block_section, "resources": resources_section}
    for name in args.sections.split(","):
        sections[name](k, ops, args.rounds, lines)
        torch.cuda.empty_cache()
        if args.out:   # what has been measured so far survives a later section
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
