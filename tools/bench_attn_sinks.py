"""Attention with sinks against the same call without them, of the same build on the same
tensors, timed in ONE process and interleaved (so every call of a group sees the same
clocks and the same neighbours on the box), bf16, causal, p = 0, grouped-query heads read
in place, a window of S / 4 so that both sides run the generic 16-rows-per-wave kernels:

* B 4, S 2048, H 32, Hkv 8, D 128 and B 8, S 1024, H 24, Hkv 8, D 64;
* forward: the sink is one more term folded in after the key loop (an epilogue);
* backward: the same three kernels on the forward's lse, plus the ``dsinks`` reduction;
* each ratio stands next to the sinkless call's own quartile spread (q3 / q1): a ratio
  inside it is not resolved by this measurement;
* the ``dsinks`` kernel alone (``attention_dsink`` on the backward's lse and a delta of
  the same shape).

    python tools/bench_attn_sinks.py [--rounds 20] [--out FILE]

Times are device events around single calls, medians over the rounds, with the quartiles
as the spread.  Nothing is fixed in advance: the file records what was measured.  Needs a
GPU: there is no CPU fallback.
"""
import argparse
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_rowwise_llama import _clock, _time_interleaved  # noqa: E402

CASES = [(4, 2048, 32, 8, 128), (8, 1024, 24, 8, 64)]


def _stat(ts):
    return statistics.median(ts), ts[len(ts) // 4], ts[(3 * len(ts)) // 4]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_sinks.py measures GPU kernels: no GPU found")
    from mipipe._native_loader import kernels

    k = kernels()
    dev, bf = "cuda", torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(7)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g).to(bf)  # noqa: E731
    lines = [f"# tools/bench_attn_sinks.py --rounds {args.rounds}",
             f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}, {time.strftime('%Y-%m-%d %H:%M:%S')}",
             f"# clock: {_clock()}; {args.rounds} interleaved rounds per group after 5 warm-up rounds; bf16, causal, "
             "p = 0, sinks linspace(0, 4, H)",
             "# call                                                    median      [quartiles]       "
             "with / without   sinkless q3 / q1"]
    for B, S, H, Hkv, D in CASES:
        scale = 1.0 / math.sqrt(D)
        W = S // 4
        qkv = rn(B, S, H + 2 * Hkv, D)
        q, kk, v = qkv[:, :, :H], qkv[:, :, H:H + Hkv], qkv[:, :, H + Hkv:]
        do = rn(B, S, H, D)
        dqkv = torch.empty_like(qkv)
        dq, dk, dv = dqkv[:, :, :H], dqkv[:, :, H:H + Hkv], dqkv[:, :, H + Hkv:]
        sinks = torch.linspace(0.0, 4.0, H, device=dev)
        ds = torch.empty(H, device=dev)
        tag = f"B{B} S{S} H{H}/{Hkv} D{D} window {W}"
        plain = k.attention_fwd(q, kk, v, True, 0.0, scale, window=W)
        sunk = k.attention_fwd(q, kk, v, True, 0.0, scale, window=W, sinks=sinks)
        fwd = _time_interleaved({
            "without": lambda: k.attention_fwd(q, kk, v, True, 0.0, scale, window=W),
            "with sinks": lambda: k.attention_fwd(q, kk, v, True, 0.0, scale, window=W, sinks=sinks),
        }, args.rounds)
        bwd = _time_interleaved({
            "without": lambda: k.attention_bwd(do, q, kk, v, plain[0], plain[1], True, 0.0, scale, 0, 0, dq, dk, dv,
                                               None, 0, W),
            "with sinks": lambda: k.attention_bwd(do, q, kk, v, sunk[0], sunk[1], True, 0.0, scale, 0, 0, dq, dk, dv,
                                                  None, 0, W, 0.0, None, sinks, ds),
        }, args.rounds)
        for what, res in (("fwd", fwd), ("bwd", bwd)):
            u, u1, u3 = _stat(res["without"])
            m, m1, m3 = _stat(res["with sinks"])
            lines.append(f"{tag + ' ' + what:56s} {u:9.1f} us  [{u1:8.1f}, {u3:8.1f}]")
            lines.append(f"{tag + ' ' + what + ' with sinks':56s} {m:9.1f} us  [{m1:8.1f}, {m3:8.1f}]  "
                         f"{m / u:12.3f}   {u3 / u1:14.3f}")
        delta = torch.randn(B, H, S, device=dev, generator=g)
        alone = _time_interleaved({"dsinks": lambda: k.attention_dsink(sunk[1], delta, sinks, ds)}, args.rounds)
        m, m1, m3 = _stat(alone["dsinks"])
        nb = 2 * B * H * S * 4
        lines.append(f"{tag + ' dsinks kernel alone':56s} {m:9.1f} us  [{m1:8.1f}, {m3:8.1f}]  "
                     f"({nb / 1e6:.2f} MB read, {H} blocks)")
        del qkv, dqkv, do, plain, sunk
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
