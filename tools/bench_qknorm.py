"""The fused QK-norm + RoPE kernels against the kernel that moves the same bytes
and against the unfused composition, timed in ONE process and interleaved (A,
B, C, A, B, C, ... so all see the same clocks and the same neighbours on the
box), at two bf16 shapes:

* B 4, S 2048, 32 query / 8 K/V heads, D 128 (Qwen3-8B's and LLaMA-3's attention);
* B 8, S 1024, 24 query / 8 K/V heads, D 64.

Per shape, forward and backward:

* fused: ``qk_norm_rope_fwd`` (out of place, rstd written) and ``qk_norm_rope_bwd``
  (with its ``reduce_parts`` pass: the whole backward of the op);
* rope_heads out of place on the same tensor -- the yardstick: it reads and
  writes every element once, like the fused forward;
* unfused: an eager per-head RMSNorm of the Q and K heads (the reference's
  arithmetic, written back into a packed tensor) followed by ``rope_heads``; its
  backward is autograd's through the same two steps.

    python tools/bench_qknorm.py [--rounds 30] [--out profiles/qknorm.txt]

Times are device events around single calls, medians over the rounds, with the
quartiles as the spread; bytes are the tensors each call must read and write.
Needs a GPU: there is no CPU fallback.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(4, 2048, 32, 8, 128), (8, 1024, 24, 8, 64)]
EPS = 1e-6


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
    tail = (f"{nbytes / 1e6:9.1f} MB  {nbytes / med / 1e6:6.2f} TB/s" if nbytes
            else "(bytes not counted: several eager kernels)")
    return med, f"{name:52s} {med:9.1f} us  [{q1:8.1f}, {q3:8.1f}]  {tail}"


def _unfused(x, wq, wk, cos, sin, n_q, n_k, ops):
    """Eager per-head RMSNorm of the Q and K heads, then rope_heads: what the ops before the fused kernel allow."""
    n = n_q + n_k
    D = x.shape[-1]
    qk = x[:, :, :n].float()
    w = torch.cat((wq.float().expand(n_q, D), wk.float().expand(n_k, D)), 0)
    normed = (qk * torch.rsqrt(qk.pow(2).mean(-1, keepdim=True) + EPS) * w).to(x.dtype)
    return ops.rope_heads(torch.cat((normed, x[:, :, n:]), dim=2), cos, sin, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_qknorm.py measures GPU kernels: no GPU found")
    from mipipe import ops
    from mipipe._native_loader import kernels

    k = kernels()
    dev, bf = "cuda", torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(7)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g).to(bf)  # noqa: E731
    lines = [f"# tools/bench_qknorm.py --rounds {args.rounds}",
             f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}, {time.strftime('%Y-%m-%d %H:%M:%S')}",
             f"# {args.rounds} interleaved rounds per group after 5 warm-up rounds; bf16",
             "# call                                          median      [quartiles]        bytes moved   rate"]
    verdicts = []
    for B, S, H, Hkv, D in SHAPES:
        heads, n = H + 2 * Hkv, H + Hkv
        x, dout = rn(B, S, heads, D), rn(B, S, heads, D)
        wq, wk = 1 + 0.1 * rn(D), 1 + 0.1 * rn(D)
        cos, sin = ops.rope_tables(S, D, device=dev)
        out = torch.empty_like(x)
        _, rstd = k.qk_norm_rope_fwd(x, wq, wk, EPS, cos, sin, None, H, Hkv, 0, True)
        t = x.numel() * 2
        r = B * S * n * 4  # rstd
        tag = f"B{B} S{S} {H}/{Hkv} D{D}"
        lines.append(f"# ---- {tag}: x [{B}, {S}, {heads}, {D}] = {t / 1e6:.1f} MB")
        # the results agree before anything is timed (the unfused path rounds once more, after the norm)
        y = k.qk_norm_rope_fwd(x, wq, wk, EPS, cos, sin, None, H, Hkv, 0, False)[0]
        yu = _unfused(x, wq, wk, cos, sin, H, Hkv, ops)
        err = (y.float() - yu.float()).abs().max().item()
        lines.append(f"# max |fused - unfused| = {err:.3e} (bf16 outputs of magnitude {yu.float().abs().max().item():.2f})")

        fwd = _time_interleaved({
            "rope_heads fwd (yardstick)": lambda: k.rope_heads(x, cos, sin, out, n, 0, False),
            "fused qk-norm+rope fwd": lambda: k.qk_norm_rope_fwd(x, wq, wk, EPS, cos, sin, out, H, Hkv, 0, True),
            "unfused eager norm + rope_heads fwd": lambda: _unfused(x, wq, wk, cos, sin, H, Hkv, ops),
        }, args.rounds)
        # rope: x -> out; fused: the same plus rstd; unfused (least traffic it could have): Q, K read and written
        # by the norm, then the rope pass
        nbs = (2 * t, 2 * t + r, 2 * t + 2 * t * n // heads)
        meds = []
        for (name, ts), nb in zip(fwd.items(), nbs):
            m, line = _row(f"{name} {tag}", ts, nb)
            meds.append(m)
            lines.append(line)
        spread = (fwd["rope_heads fwd (yardstick)"][(3 * args.rounds) // 4]
                  - fwd["rope_heads fwd (yardstick)"][args.rounds // 4]) / meds[0]
        verdicts.append(f"# {tag} fwd: fused / rope_heads time {meds[1] / meds[0]:.3f} (rope_heads' own quartile spread "
                        f"{spread:.3f}); unfused / fused {meds[2] / meds[1]:.2f}")
        fwd_rate = nbs[1] / meds[1]

        # backward: the fused op's, rope_heads' (the inverse rotation: the same kernel) and autograd's through
        # the unfused composition
        xs, qs, ks = x.clone().requires_grad_(), wq.clone().requires_grad_(), wk.clone().requires_grad_()
        yu = _unfused(xs, qs, ks, cos, sin, H, Hkv, ops)

        def unfused_bwd():
            torch.autograd.grad(yu, (xs, qs, ks), dout, retain_graph=True)

        bwd = _time_interleaved({
            "rope_heads bwd (yardstick)": lambda: k.rope_heads(dout, cos, sin, out, n, 0, True),
            "fused qk-norm+rope bwd": lambda: k.qk_norm_rope_bwd(dout, x, rstd, wq, wk, cos, sin, H, Hkv, 0),
            "unfused autograd bwd": unfused_bwd,
        }, args.rounds)
        # fused: dout and x read (Q, K heads of x only), dx written, rstd read
        nbs = (2 * t, 2 * t + t * n // heads + r, 0)
        meds = []
        for (name, ts), nb in zip(bwd.items(), nbs):
            m, line = _row(f"{name} {tag}", ts, nb)
            meds.append(m)
            lines.append(line)
        bwd_rate = nbs[1] / meds[1]
        verdicts.append(f"# {tag} bwd: fused {bwd_rate / 1e6:.2f} TB/s against the fused forward's {fwd_rate / 1e6:.2f} "
                        f"TB/s (ratio {bwd_rate / fwd_rate:.3f}); fused / rope_heads time {meds[1] / meds[0]:.3f}; "
                        f"unfused / fused {meds[2] / meds[1]:.2f}")
        del x, dout, out, xs, yu, y
    text = "\n".join(lines + verdicts) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
