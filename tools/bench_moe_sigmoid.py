"""The sigmoid router (moe_sigmoid.hip), timed in ONE process with interleaved rounds, bf16: route forward and
backward at ``[8192, 256]`` (k 8, 8 groups of which 4 stay: DeepSeek-V3's gate) and at ``[8192, 64]`` (k 6,
ungrouped), each against (a) the softmax ``moe_route`` on the same tensor, which moves the same bytes, and (b) the
eager reference of the same routing; then the compiler's resource report of the new kernels.

    python tools/bench_moe_sigmoid.py [--rounds 30] [--out profiles/moe_sigmoid.txt]

Times are device events around single calls, medians over the rounds with the quartiles as the spread.  Nothing is
fixed in advance: the file records what was measured.  Needs a GPU: there is no CPU fallback.
"""
import argparse
import math
import os
import re
import shutil
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_moe_grouped import _stat  # noqa: E402
from tools.bench_rowwise_llama import _clock, _time_interleaved  # noqa: E402

SHAPES = [(8192, 256, 8, 8, 4), (8192, 64, 6, 1, 1)]   # T, Ne, k, n_group, topk_group


def route_section(ops, rounds, lines):
    from mipipe.ops.moe import moe_route_reference

    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    for T, Ne, kk, n_group, topk_group in SHAPES:
        lg = torch.randn(T, Ne, device=dev, generator=g).to(torch.bfloat16).requires_grad_()
        bias = torch.rand(Ne, device=dev, generator=g) - 0.5
        dgate, dprobs = torch.randn(T, kk, device=dev, generator=g), torch.randn(Ne, device=dev, generator=g)
        kw = dict(score="sigmoid", bias=bias, n_group=n_group, topk_group=topk_group, renormalize=True, scale=2.5)
        fwd = {"sigmoid": lambda: ops.moe_route(lg, kk, **kw), "softmax": lambda: ops.moe_route(lg, kk),
               "eager": lambda: moe_route_reference(lg, kk, **kw)}
        calls = {}
        for name, f in fwd.items():
            _, gate, probs = f()
            out = (gate * dgate).sum() + (probs * dprobs).sum()
            calls[f"fwd {name}"] = f
            calls[f"bwd {name}"] = (lambda o: lambda: torch.autograd.grad(o, lg, retain_graph=True))(out)
        res = _time_interleaved(calls, rounds, warmup=3)
        L = min(64, 1 << max(1, math.ceil(math.log2(Ne))))
        shuffles = ((2 + topk_group if n_group > 1 else 0) + kk) * int(math.log2(L))
        lines.append(f"# [{T}, {Ne}] k {kk}, {n_group} groups, {topk_group} kept: about {shuffles} shuffle rounds per row "
                     f"((2 + topk_group + k) log2 L), the softmax kernel k log2 L = {kk * int(math.log2(L))}; the "
                     "backward times are autograd.grad of sum(gate dgate) + sum(probs_sum dprobs): the route's "
                     "backward kernel plus two small eager products")
        lines.append("# call                 median     [quartiles]      / softmax   softmax q3 / q1   eager / this")
        for d in ("fwd", "bwd"):
            a, a1, a3 = _stat(res[f"{d} softmax"])
            e = _stat(res[f"{d} eager"])[0]
            for name in ("softmax", "sigmoid", "eager"):
                m, m1, m3 = _stat(res[f"{d} {name}"])
                lines.append(f"{f'{d} {name}':18s} {m:9.1f} us  [{m1:8.1f}, {m3:8.1f}]  {m / a:8.3f}       {a3 / a1:8.3f}      "
                             f"{e / m:8.1f}")


def resources_section(ops, rounds, lines):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "mipipe", "csrc", "kernels", "moe_sigmoid.hip")
    cmd = [hipcc, "-std=c++17", "--offload-arch=gfx950", "-O3", "-ffp-contract=fast", "-munsafe-fp-atomics", "-mllvm",
           "-pragma-unroll-threshold=1000000", "--offload-device-only", "-c", src, "-o", os.devnull,
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    lines.append("# resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage on moe_sigmoid.hip)")
    lines.append("# kernel                                         SGPRs VGPRs scratch waves/SIMD LDS bytes")
    cur = {}
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        cur[m.group(1)] = m.group(2)
        if m.group(1).startswith("LDS"):
            fn = subprocess.run(["c++filt", cur["Function Name"]], capture_output=True, text=True).stdout.strip()
            fn = re.sub(r"\(.*", "", fn.replace("mipipe::(anonymous namespace)::", "").replace("void ", ""))
            lines.append(f"{fn:48s} {cur['TotalSGPRs']:>5s} {cur['VGPRs']:>5s} {cur['ScratchSize [bytes/lane]']:>7s} "
                         f"{cur['Occupancy [waves/SIMD]']:>10s} {cur['LDS Size [bytes/block]']:>9s}")
            cur = {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_moe_sigmoid.py measures GPU kernels: no GPU found")
    from mipipe import ops

    lines = [f"# tools/bench_moe_sigmoid.py --rounds {args.rounds}",
             f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}, {time.strftime('%Y-%m-%d %H:%M:%S')}",
             f"# clock: {_clock()}; {args.rounds} interleaved rounds per group after warm-up rounds; bf16"]
    for section in (route_section, resources_section):
        section(ops, args.rounds, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
