"""Native grouped-query attention against the same kernels on repeated K/V heads
(what the code could run before it had GQA), timed in ONE process and
interleaved (A, B, A, B, ... so both see the same clocks and the same
neighbours on the box), bf16, causal, p = 0:

* B 4, S 2048, H 32, Hkv 8, D 128 (LLaMA-3 8B's heads; the generic kernels);
* B 8, S 1024, H 24, Hkv 8, D 64 (the long-sequence kernels).

Forward: ``attention_fwd`` on the packed ``[B, S, H + 2 Hkv, D]`` buffer against
``[B, S, 3, H, D]`` with every K/V head repeated.  Backward: ``attention_bwd``
with the per-query-head scratch and the group-sum kernel inside the call,
against the repeated-head backward (which leaves the group sum to whoever
consumes its dK / dV).  The group-sum kernel alone is reported as bytes per
second next to ``rope_packed`` out of place, which moves comparable bytes.

    python tools/bench_attn_gqa.py [--rounds 30] [--out FILE]

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

SHAPES = [(4, 2048, 32, 8, 128), (8, 1024, 24, 8, 64)]  # B, S, H, Hkv, D


def _stat(ts):
    return statistics.median(ts), ts[len(ts) // 4], ts[(3 * len(ts)) // 4]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_gqa.py measures GPU kernels: no GPU found")
    from mipipe import ops
    from mipipe._native_loader import kernels

    k = kernels()
    dev, bf = "cuda", torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(7)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g).to(bf)  # noqa: E731
    lines = [f"# tools/bench_attn_gqa.py --rounds {args.rounds}",
             f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}, {time.strftime('%Y-%m-%d %H:%M:%S')}",
             f"# clock: {_clock()}; {args.rounds} interleaved rounds per pair after 5 warm-up rounds; bf16, causal, p = 0",
             "# call                                              median      [quartiles]"]
    for B, S, H, Hkv, D in SHAPES:
        G, scale = H // Hkv, 1.0 / math.sqrt(D)
        qkv = rn(B, S, H + 2 * Hkv, D)
        q, kk, v = qkv[:, :, :H], qkv[:, :, H:H + Hkv], qkv[:, :, H + Hkv:]
        x5 = torch.stack((q, kk.repeat_interleave(G, 2), v.repeat_interleave(G, 2)), dim=2).contiguous()
        q5, k5, v5 = x5.select(2, 0), x5.select(2, 1), x5.select(2, 2)
        do = rn(B, S, H, D)
        o, lse, _, _, _ = k.attention_fwd(q, kk, v, True, 0.0, scale)
        o5, lse5, _, _, _ = k.attention_fwd(q5, k5, v5, True, 0.0, scale)
        assert torch.equal(o, o5)
        dqkv, d5 = torch.empty_like(qkv), torch.empty_like(x5)
        dq, dk, dv = dqkv[:, :, :H], dqkv[:, :, H:H + Hkv], dqkv[:, :, H + Hkv:]
        tag = f"B{B} S{S} H{H}/{Hkv} D{D}"
        lines.append(f"# {tag}: {'long-sequence' if k.attention_long_supported(S, D) else 'generic'} kernels")
        fwd = _time_interleaved({
            "fwd repeated heads": lambda: k.attention_fwd(q5, k5, v5, True, 0.0, scale),
            "fwd native GQA": lambda: k.attention_fwd(q, kk, v, True, 0.0, scale)}, args.rounds)
        bwd = _time_interleaved({
            "bwd repeated heads": lambda: k.attention_bwd(do, q5, k5, v5, o5, lse5, True, 0.0, scale, 0, 0,
                                                          d5.select(2, 0), d5.select(2, 1), d5.select(2, 2), None, 0),
            "bwd native GQA (+ group sum)": lambda: k.attention_bwd(do, q, kk, v, o, lse, True, 0.0, scale, 0, 0,
                                                                    dq, dk, dv, None, 0)}, args.rounds)
        assert torch.equal(dq, d5.select(2, 0))
        dkv = rn(B, S, 2, H, D)
        cos, sin = ops.rope_tables(S, D, device=dev)
        rope_out = torch.empty_like(x5)
        mem = _time_interleaved({
            "gqa_reduce_dkv alone": lambda: k.gqa_reduce_dkv(dkv, dqkv, H, Hkv),
            "rope_packed out of place": lambda: k.rope_packed(x5, cos, sin, rope_out)}, args.rounds)
        meds = {}
        for pair in (fwd, bwd):
            for n, ts in pair.items():
                m, q1, q3 = _stat(ts)
                meds[n] = (m, q1, q3)
                lines.append(f"{tag + ' ' + n:50s} {m:9.1f} us  [{q1:8.1f}, {q3:8.1f}]")
        nbytes = {"gqa_reduce_dkv alone": (dkv.numel() + 2 * B * S * Hkv * D) * 2,
                  "rope_packed out of place": 2 * x5.numel() * 2}
        for n, ts in mem.items():
            m, q1, q3 = _stat(ts)
            meds[n] = (m, q1, q3)
            lines.append(f"{tag + ' ' + n:50s} {m:9.1f} us  [{q1:8.1f}, {q3:8.1f}]  {nbytes[n] / 1e6:8.1f} MB  "
                         f"{nbytes[n] / m / 1e6:5.2f} TB/s")
        f0, f1 = meds["fwd repeated heads"], meds["fwd native GQA"]
        spread = max(f0[2] - f0[1], f1[2] - f1[1])
        lines.append(f"# {tag} forward native - repeated: {f1[0] - f0[0]:+.1f} us (interquartile spread {spread:.1f} us): "
                     f"{'no slower beyond the spread' if f1[0] - f0[0] <= spread else 'SLOWER than the spread'}")
        b0, b1 = meds["bwd repeated heads"], meds["bwd native GQA (+ group sum)"]
        lines.append(f"# {tag} backward native - repeated: {b1[0] - b0[0]:+.1f} us; the group-sum kernel alone: "
                     f"{meds['gqa_reduce_dkv alone'][0]:.1f} us")
        del qkv, x5, dqkv, d5, dkv, rope_out, o, o5, do
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
