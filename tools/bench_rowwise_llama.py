"""The LLaMA-style block's memory-bound kernels against the existing kernels that
move comparable bytes, timed in ONE process and interleaved (A, B, A, B, ...
so both see the same clocks and the same neighbours on the box):

* RMSNorm forward / backward against LayerNorm forward / backward at
  16384 x 4096 bf16, with a residual, p = 0 (same bytes; RMSNorm reads no beta
  and does one row reduction instead of two);
* SwiGLU forward / backward against bias_act_dropout (GELU, no bias, p = 0) at
  16384 x 11008, compared per byte moved;
* RoPE alone, as effective TB/s at B 4, S 4096, H 32, D 128 (in place and out
  of place).

    python tools/bench_rowwise_llama.py [--rounds 30] [--out profiles/llama_rowwise.txt]

Times are device events around single calls, medians over the rounds, with the
quartiles as the spread.  Needs a GPU: there is no CPU fallback.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time_interleaved(calls, rounds, warmup=5):
    """calls: {name: fn}.  Returns {name: sorted per-call times in us}, the calls run in rotation."""
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    ts = {n: [] for n in calls}
    for _ in range(rounds):
        for n, fn in calls.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            ts[n].append(s.elapsed_time(e) * 1e3)
    return {n: sorted(v) for n, v in ts.items()}


def _row(name, ts, nbytes):
    med = statistics.median(ts)
    q1, q3 = ts[len(ts) // 4], ts[(3 * len(ts)) // 4]
    return med, f"{name:34s} {med:9.1f} us  [{q1:8.1f}, {q3:8.1f}]  {nbytes / 1e6:9.1f} MB  {nbytes / med / 1e6:6.2f} TB/s"


def _clock():
    try:
        return f"{torch.cuda.clock_rate()} MHz (SM clock at start)"
    except Exception as exc:  # no SMI library in this environment
        return f"not available ({type(exc).__name__})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rowwise_llama.py measures GPU kernels: no GPU found")
    from mipipe import ops
    from mipipe._native_loader import kernels

    k = kernels()
    dev, bf = "cuda", torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(7)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g).to(bf)  # noqa: E731
    lines = [f"# tools/bench_rowwise_llama.py --rounds {args.rounds}",
             f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}, {time.strftime('%Y-%m-%d %H:%M:%S')}",
             f"# clock: {_clock()}; {args.rounds} interleaved rounds per pair after 5 warm-up rounds",
             "# kernel                                median      [quartiles]        bytes moved   rate"]
    verdicts = []

    # ---- RMSNorm vs LayerNorm, 16384 x 4096 bf16, residual, p = 0
    rows, cols = 16384, 4096
    x, res, dy = rn(rows, cols), rn(rows, cols), rn(rows, cols)
    w, b = (1 + 0.1 * rn(cols)), 0.1 * rn(cols)
    _, zl, mean, rstd_l, _, _ = k.layernorm_fwd(x, res, w, b, 1e-5, 0.0, True)
    _, zr, rstd_r, _, _ = k.rmsnorm_fwd(x, res, w, 1e-5, 0.0, True)
    t = rows * cols * 2
    fwd = _time_interleaved({"layernorm fwd": lambda: k.layernorm_fwd(x, res, w, b, 1e-5, 0.0, True),
                             "rmsnorm fwd": lambda: k.rmsnorm_fwd(x, res, w, 1e-5, 0.0, True)}, args.rounds)
    bwd = _time_interleaved({"layernorm bwd": lambda: k.layernorm_bwd(dy, zl, mean, rstd_l, w, 0.0, 0, 0),
                             "rmsnorm bwd": lambda: k.rmsnorm_bwd(dy, zr, rstd_r, w, 0.0, 0, 0)}, args.rounds)
    for pair, nb in ((fwd, 4 * t), (bwd, 3 * t)):  # fwd: x, res -> y, z; bwd: dy, z -> dz
        meds = []
        for n, ts in pair.items():
            m, line = _row(f"{n} {rows}x{cols}", ts, nb)
            meds.append(m)
            lines.append(line)
        ratio = meds[1] / meds[0]
        verdicts.append(f"# {list(pair)[1]} / {list(pair)[0]} time: {ratio:.3f} "
                        f"({'within' if ratio <= 1.05 else 'MISSES'} the 1.05 allowed)")
    del x, res, dy, zl, zr

    # ---- SwiGLU vs bias_act (GELU, no bias, p = 0), 16384 x 11008: per byte moved
    rows, F = 16384, 11008
    gu, dh = rn(rows, 2 * F), rn(rows, F)
    pre = gu.view(-1)[: rows * F].view(rows, F)  # bias_act at rows x F, the same memory
    t = rows * F * 2
    fwd = _time_interleaved({"bias_act gelu fwd": lambda: k.bias_act_fwd(pre, None, 2, 0.0),
                             "swiglu fwd": lambda: k.swiglu_fwd(gu)}, args.rounds)
    bwd = _time_interleaved({"bias_act gelu bwd": lambda: k.bias_act_bwd(dh, pre, None, 2, 0.0, 0, 0, False),
                             "swiglu bwd": lambda: k.swiglu_bwd(dh, gu)}, args.rounds)
    # bias_act fwd: 1 read + 1 write; swiglu fwd: 2F read + F written; bwd: 2 reads + 1 write against F + 2F read, 2F written
    for pair, nbs in ((fwd, (2 * t, 3 * t)), (bwd, (3 * t, 5 * t))):
        rates = []
        for (n, ts), nb in zip(pair.items(), nbs):
            m, line = _row(f"{n} {rows}x{F}", ts, nb)
            rates.append(nb / m)
            lines.append(line)
        ratio = rates[1] / rates[0]
        verdicts.append(f"# {list(pair)[1]} / {list(pair)[0]} bytes per second: {ratio:.3f} "
                        f"({'within' if ratio >= 0.95 else 'MISSES'} the 0.95 asked for)")
    del gu, dh, pre

    # ---- RoPE alone
    B, S, H, D = 4, 4096, 32, 128
    qkv = rn(B, S, 3, H, D)
    out = torch.empty_like(qkv)
    cos, sin = ops.rope_tables(S, D, device=dev)
    t = qkv.numel() * 2
    rope = _time_interleaved({"rope out of place": lambda: k.rope_packed(qkv, cos, sin, out),
                              "rope in place": lambda: k.rope_packed(qkv, cos, sin, qkv)}, args.rounds)
    for (n, ts), nb in zip(rope.items(), (2 * t, 2 * t * 2 // 3)):  # in place: Q and K read and written, V untouched
        lines.append(_row(f"{n} B{B} S{S} H{H} D{D}", ts, nb)[1])
    text = "\n".join(lines + verdicts) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
