"""Sliding-window attention against full causal attention of the same build on the
same tensors, timed in ONE process and interleaved (causal, windowed, causal,
... so both see the same clocks and the same neighbours on the box), bf16,
causal, p = 0, grouped-query heads read in place:

* B 2, S 8192, H 32, Hkv 8, D 128, windows 4096 and 1024 (Mistral 7B's shape);
* B 4, S 4096, H 32, Hkv 8, D 128, window 1024 (a shorter sequence, same heads);
* B 8, S 1024, H 24, Hkv 8, D 64, window 256: the windowed call on the generic
  16-rows-per-wave kernels against the causal call on the long-sequence kernels.

The windowed kernels visit, per 64-row tile, only the 64-key tiles that hold a
key of the band; the share of the causal call's tiles they visit is computed
from the shapes and printed next to the measured time ratio.

    python tools/bench_attn_window.py [--rounds 20] [--out FILE]

Times are device events around single calls, medians over the rounds, with the
quartiles as the spread.  Needs a GPU: there is no CPU fallback.
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

CASES = [(2, 8192, 32, 8, 128, (4096, 1024)), (4, 4096, 32, 8, 128, (1024,)), (8, 1024, 24, 8, 64, (256,))]
TILE = 64


def tile_share(S, W):
    """Visited 64 x 64 tiles of the windowed kernels over those of the causal ones.  Forward and dQ: query
    tile qt visits the key tiles max(0, 64 qt - W + 1) // 64 .. qt; dK/dV visits the transposed set."""
    n = S // TILE
    causal = n * (n + 1) // 2
    band = sum(qt - max(0, TILE * qt - W + 1) // TILE + 1 for qt in range(n))
    dkv = sum(min(n - 1, (TILE * kt + TILE - 1 + W - 1) // TILE) - kt + 1 for kt in range(n))
    assert dkv == band
    return band / causal


def _stat(ts):
    return statistics.median(ts), ts[len(ts) // 4], ts[(3 * len(ts)) // 4]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_window.py measures GPU kernels: no GPU found")
    from mipipe._native_loader import kernels

    k = kernels()
    dev, bf = "cuda", torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(7)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g).to(bf)  # noqa: E731
    lines = [f"# tools/bench_attn_window.py --rounds {args.rounds}",
             f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}, {time.strftime('%Y-%m-%d %H:%M:%S')}",
             f"# clock: {_clock()}; {args.rounds} interleaved rounds per group after 5 warm-up rounds; bf16, causal, p = 0",
             "# call                                              median      [quartiles]       time / causal   tiles / causal"]
    verdicts = []
    for B, S, H, Hkv, D, windows in CASES:
        scale = 1.0 / math.sqrt(D)
        qkv = rn(B, S, H + 2 * Hkv, D)
        q, kk, v = qkv[:, :, :H], qkv[:, :, H:H + Hkv], qkv[:, :, H + Hkv:]
        do = rn(B, S, H, D)
        dqkv = torch.empty_like(qkv)
        dq, dk, dv = dqkv[:, :, :H], dqkv[:, :, H:H + Hkv], dqkv[:, :, H + Hkv:]
        tag = f"B{B} S{S} H{H}/{Hkv} D{D}"
        lines.append(f"# {tag}: causal on the {'long-sequence' if k.attention_long_supported(S, D) else 'generic'} "
                     "kernels, windowed on the generic ones")
        outs = {0: k.attention_fwd(q, kk, v, True, 0.0, scale)}
        for W in windows:
            outs[W] = k.attention_fwd(q, kk, v, True, 0.0, scale, window=W)
        name = lambda W: "causal" if W == 0 else f"window {W}"  # noqa: E731
        fwd = _time_interleaved({name(W): (lambda W=W: k.attention_fwd(q, kk, v, True, 0.0, scale, window=W))
                                 for W in outs}, args.rounds)
        bwd = _time_interleaved({name(W): (lambda W=W: k.attention_bwd(do, q, kk, v, outs[W][0], outs[W][1], True,
                                                                       0.0, scale, 0, 0, dq, dk, dv, None, 0, W))
                                 for W in outs}, args.rounds)
        for what, res in (("fwd", fwd), ("bwd", bwd)):
            c, c1, c3 = _stat(res["causal"])
            lines.append(f"{tag + ' ' + what + ' causal':50s} {c:9.1f} us  [{c1:8.1f}, {c3:8.1f}]")
            for W in windows:
                m, q1, q3 = _stat(res[name(W)])
                share = tile_share(S, W)
                lines.append(f"{tag + ' ' + what + ' ' + name(W):50s} {m:9.1f} us  [{q1:8.1f}, {q3:8.1f}]  "
                             f"{m / c:12.3f}   {share:12.3f}")
                if (S, W) == (8192, 1024):
                    spread = max(c3 - c1, q3 - q1)
                    ok = c - m > spread
                    verdicts.append(f"# {tag} {what} window {W}: causal - windowed = {c - m:+.1f} us, interquartile "
                                    f"spread {spread:.1f} us: "
                                    f"{'faster beyond the spread' if ok else 'NOT faster beyond the spread'}")
        del qkv, dqkv, do, outs
    text = "\n".join(lines + verdicts) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
