"""Attention with head dims (192, 128) on its native kernels (attention_mla.hip) against the only way the
D = 256 kernels can run the same tensors: q, k and v zero-padded to 256 and the result sliced back to 128.  Both
sides go through ``ops.attention`` on the same values, in ONE process and interleaved (so every call of a group
sees the same clocks and the same neighbours on the box), bf16, causal, p = 0:

* B 2, S 4096, H 16 (DeepSeek-V2-Lite's heads) and B 1, S 4096, H 128 (DeepSeek-V3's);
* q, k, v are transposed views of ``[B, S, H, D]`` tensors, so neither side copies; the padded side's tensors
  are padded before the clock starts (the pad is not charged to it), its scale is the native ``1 / sqrt(192)``;
* forward: one ``ops.attention`` call; backward: ``autograd.grad`` of that call's result (delta, dK/dV, dQ);
* each ratio stands next to the padded call's own quartile spread (q3 / q1): a ratio inside it is not resolved
  by this measurement.  The MFMA-work ratio is (192 + 128) / (256 + 256) = 0.625 forward.

    python tools/bench_attn_mla.py [--rounds 20] [--out FILE]

Times are device events around single calls, medians over the rounds, with the quartiles as the spread.  Nothing
is fixed in advance: the file records what was measured.  Needs a GPU: there is no CPU fallback.
"""
import argparse
import math
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_rowwise_llama import _clock, _time_interleaved  # noqa: E402

CASES = [(2, 4096, 16), (1, 4096, 128)]
DQK, DV, DP = 192, 128, 256


def _stat(ts):
    return statistics.median(ts), ts[len(ts) // 4], ts[(3 * len(ts)) // 4]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_mla.py measures GPU kernels: no GPU found")
    from mipipe import ops

    dev, bf = "cuda", torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(7)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g).to(bf)  # noqa: E731
    scale = 1.0 / math.sqrt(DQK)
    lines = [f"# tools/bench_attn_mla.py --rounds {args.rounds}",
             f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}, {time.strftime('%Y-%m-%d %H:%M:%S')}",
             f"# clock: {_clock()}; {args.rounds} interleaved rounds per group after 5 warm-up rounds; bf16, causal, "
             "p = 0, head dims (192, 128)",
             "# call                                                    median      [quartiles]       "
             "native / padded   padded q3 / q1"]
    for B, S, H in CASES:
        q, k, v = rn(B, S, H, DQK), rn(B, S, H, DQK), rn(B, S, H, DV)
        do = rn(B, S, H, DV).transpose(1, 2)
        native = [t.transpose(1, 2).requires_grad_() for t in (q, k, v)]
        padded = [F.pad(t, (0, DP - t.shape[-1])).transpose(1, 2).requires_grad_() for t in (q, k, v)]
        run = {"native": lambda: ops.attention(*native, True, scale=scale),
               "padded 256": lambda: ops.attention(*padded, True, scale=scale)[..., :DV]}
        outs = {n: fn() for n, fn in run.items()}
        diff = (outs["native"].float() - outs["padded 256"].float()).abs().max().item()
        fwd = _time_interleaved(run, args.rounds)
        bwd = _time_interleaved({n: (lambda o=o, x=x: torch.autograd.grad(o, x, do, retain_graph=True))
                                 for (n, o), x in zip(outs.items(), (native, padded))}, args.rounds)
        tag = f"B{B} S{S} H{H}"
        for what, res in (("fwd", fwd), ("bwd", bwd)):
            u, u1, u3 = _stat(res["padded 256"])
            m, m1, m3 = _stat(res["native"])
            lines.append(f"{tag + ' ' + what + ' padded to 256':56s} {u:9.1f} us  [{u1:8.1f}, {u3:8.1f}]")
            lines.append(f"{tag + ' ' + what + ' native (192, 128)':56s} {m:9.1f} us  [{m1:8.1f}, {m3:8.1f}]  "
                         f"{m / u:12.3f}   {u3 / u1:14.3f}")
        lines.append(f"{tag + ' max |o native - o padded|':56s} {diff:9.2e}")
        del q, k, v, do, native, padded, outs, run
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
