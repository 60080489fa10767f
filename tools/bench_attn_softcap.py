"""Soft-capped attention against the uncapped call of the same build on the same
tensors, timed in ONE process and interleaved (so every call of a group sees the
same clocks and the same neighbours on the box), bf16, causal, p = 0,
grouped-query heads read in place:

* B 4, S 2048, H 32, Hkv 8, D 128 and B 8, S 1024, H 24, Hkv 8, D 64, forward and
  backward, cap 50:
  1. capped + window W = S / 4 against the same window uncapped -- both run the
     generic 16-rows-per-wave kernels, so the ratio isolates the tanh (two exp2
     and one rcp per score instead of one exp2);
  2. capped causal against plain causal -- what a user sees: the uncapped call
     may run the wide or the long-sequence kernels, the capped one never does;
* ``ops.softcap`` forward and backward at [4096, 32000] bf16, in TB/s (the forward
  reads and writes the tensor once, the backward reads two and writes one), next
  to ``bias_act_dropout`` (identity, no bias, p = 0: a pure copy through the same
  16-byte loads and stores) on the same tensor.

    python tools/bench_attn_softcap.py [--rounds 20] [--out FILE]

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

CASES = [(4, 2048, 32, 8, 128), (8, 1024, 24, 8, 64)]
CAP = 50.0


def _stat(ts):
    return statistics.median(ts), ts[len(ts) // 4], ts[(3 * len(ts)) // 4]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_softcap.py measures GPU kernels: no GPU found")
    from mipipe._native_loader import kernels

    k = kernels()
    dev, bf = "cuda", torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(7)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g).to(bf)  # noqa: E731
    lines = [f"# tools/bench_attn_softcap.py --rounds {args.rounds}",
             f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}, {time.strftime('%Y-%m-%d %H:%M:%S')}",
             f"# clock: {_clock()}; {args.rounds} interleaved rounds per group after 5 warm-up rounds; bf16, causal, "
             f"p = 0, cap {CAP:g}",
             "# call                                                    median      [quartiles]       capped / uncapped"]
    for B, S, H, Hkv, D in CASES:
        scale = 1.0 / math.sqrt(D)
        W = S // 4
        qkv = rn(B, S, H + 2 * Hkv, D)
        q, kk, v = qkv[:, :, :H], qkv[:, :, H:H + Hkv], qkv[:, :, H + Hkv:]
        do = rn(B, S, H, D)
        dqkv = torch.empty_like(qkv)
        dq, dk, dv = dqkv[:, :, :H], dqkv[:, :, H:H + Hkv], dqkv[:, :, H + Hkv:]
        tag = f"B{B} S{S} H{H}/{Hkv} D{D}"
        if k.attention_long_supported(S, D):
            plain = "long-sequence"
        else:
            plain = "wide" if D == 64 and S % 128 == 0 else "generic"
        lines.append(f"# {tag}: plain causal on the {plain} kernels; window {W} and every capped call on the generic ones")
        # name -> (window, cap); each capped call is listed right after its uncapped partner
        calls = {f"window {W}": (W, 0.0), f"window {W} capped": (W, CAP), "causal": (0, 0.0), "causal capped": (0, CAP)}
        outs = {n: k.attention_fwd(q, kk, v, True, 0.0, scale, window=w, softcap=c) for n, (w, c) in calls.items()}
        fwd = _time_interleaved({n: (lambda w=w, c=c: k.attention_fwd(q, kk, v, True, 0.0, scale, window=w, softcap=c))
                                 for n, (w, c) in calls.items()}, args.rounds)
        bwd = _time_interleaved({n: (lambda n=n, w=w, c=c: k.attention_bwd(do, q, kk, v, outs[n][0], outs[n][1], True,
                                                                           0.0, scale, 0, 0, dq, dk, dv, None, 0, w, c))
                                 for n, (w, c) in calls.items()}, args.rounds)
        for what, res in (("fwd", fwd), ("bwd", bwd)):
            for base in (f"window {W}", "causal"):
                u, u1, u3 = _stat(res[base])
                m, m1, m3 = _stat(res[base + " capped"])
                lines.append(f"{tag + ' ' + what + ' ' + base:56s} {u:9.1f} us  [{u1:8.1f}, {u3:8.1f}]")
                lines.append(f"{tag + ' ' + what + ' ' + base + ' capped':56s} {m:9.1f} us  [{m1:8.1f}, {m3:8.1f}]  "
                             f"{m / u:12.3f}")
        del qkv, dqkv, do, outs

    # ---- ops.softcap against bias_act (identity) on [4096, 32000] bf16
    rows, cols = 4096, 32000
    x, dy = rn(rows, cols), rn(rows, cols)
    y = k.softcap_fwd(x, 30.0)
    nb = x.numel() * 2
    res = _time_interleaved({
        "softcap fwd": lambda: k.softcap_fwd(x, 30.0),
        "bias_act fwd (copy)": lambda: k.bias_act_fwd(x, None, 0, 0.0),
        "softcap bwd": lambda: k.softcap_bwd(dy, y, 30.0),
        "bias_act bwd (copy)": lambda: k.bias_act_bwd(dy, y, None, 0, 0.0, 0, 0, False, None),
    }, args.rounds)
    lines.append(f"# [{rows}, {cols}] bf16, cap 30: bytes moved = tensors read + written (new outputs included)")
    for name, moved in (("softcap fwd", 2 * nb), ("bias_act fwd (copy)", 2 * nb), ("softcap bwd", 3 * nb),
                        ("bias_act bwd (copy)", 2 * nb)):
        m, q1, q3 = _stat(res[name])
        lines.append(f"{name:56s} {m:9.1f} us  [{q1:8.1f}, {q3:8.1f}]  {moved / 1e6:9.1f} MB  {moved / m / 1e6:6.2f} TB/s")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
