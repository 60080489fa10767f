"""The Gemma-2 block's two new kernels, each against the existing kernel that
moves the same bytes on the same tensors, timed in ONE process and interleaved
(A, B, A, B, ... so all see the same clocks and the same neighbours on the box),
in bf16:

* ``geglu`` forward and backward against ``swiglu`` on one ``gu [4096, 2 * 14336]``
  (Gemma-2 9B's MLP width): the same loads and stores, another gate.
* ``rms_norm_residual`` forward at ``[8192, 3584]`` (9B) and ``[8192, 2304]`` (2B)
  against ``add_dropout_rms_norm(x, residual)`` on the same tensors.  At p = 0
  and without a backward that kernel writes no z: it reads x, residual and gamma
  and writes y and rstd, exactly the bytes of the new kernel -- the yardstick.
* the same forward against the unfused composition: the RMSNorm kernel on x
  alone, then an eager add of the residual.

    python tools/bench_gemma2_block.py [--rounds 30] [--out profiles/gemma2_block.txt]

Times are device events around single calls (each call allocates its outputs, as
the ops do), medians over the rounds with the quartiles as the spread; bytes are
the tensors each call must read and write.  Every ratio is printed next to the
baseline kernel's own quartile spread.  Needs a GPU: there is no CPU fallback.
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GLU_SHAPE = (4096, 14336)                  # rows, F
NORM_SHAPES = [(8192, 3584), (8192, 2304)]
EPS = 1e-5


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
    return med, (f"{name:52s} {med:9.1f} us  [{q1:8.1f}, {q3:8.1f}]  {nbytes / 1e6:9.1f} MB  "
                 f"{nbytes / med / 1e6:6.2f} TB/s")


def _spread(ts):
    return (ts[(3 * len(ts)) // 4] - ts[len(ts) // 4]) / statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gemma2_block.py measures GPU kernels: no GPU found")
    from mipipe import ops
    from mipipe._native_loader import kernels

    k = kernels()
    dev, bf = "cuda", torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(7)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g).to(bf)  # noqa: E731
    lines = [f"# tools/bench_gemma2_block.py --rounds {args.rounds}",
             f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}, {time.strftime('%Y-%m-%d %H:%M:%S')}",
             f"# {args.rounds} interleaved rounds per group after 5 warm-up rounds; bf16",
             "# call                                          median      [quartiles]        bytes moved   rate"]
    verdicts = []

    # ---- the gate
    rows, F = GLU_SHAPE
    gu, dh = rn(rows, 2 * F), rn(rows, F)
    t = rows * F * 2  # bytes of one [rows, F] bf16 tensor
    tag = f"[{rows}, 2 x {F}]"
    lines.append(f"# ---- gate on gu {tag} = {2 * t / 1e6:.1f} MB")
    ref = ops.geglu_reference(gu[:64].float())
    err = (k.geglu_fwd(gu[:64].contiguous()).float() - ref).abs().max().item()
    lines.append(f"# max |geglu kernel - eager fp32| on the first 64 rows = {err:.3e} (outputs of magnitude "
                 f"{ref.abs().max().item():.2f})")
    fwd = _time_interleaved({"swiglu fwd (yardstick)": lambda: k.swiglu_fwd(gu),
                             "geglu fwd": lambda: k.geglu_fwd(gu)}, args.rounds)
    bwd = _time_interleaved({"swiglu bwd (yardstick)": lambda: k.swiglu_bwd(dh, gu),
                             "geglu bwd": lambda: k.geglu_bwd(dh, gu)}, args.rounds)
    for group, nb, what in ((fwd, 3 * t, "fwd"), (bwd, 5 * t, "bwd")):  # fwd: gu read, h written; bwd: dh, gu, dgu
        meds = []
        for name, ts in group.items():
            m, line = _row(f"{name} {tag}", ts, nb)
            meds.append(m)
            lines.append(line)
        base = next(iter(group.values()))
        verdicts.append(f"# gate {what}: geglu / swiglu time {meds[1] / meds[0]:.3f} (swiglu's own quartile spread "
                        f"{_spread(base):.3f})")
    del gu, dh

    # ---- the sandwich norm
    for rows, cols in NORM_SHAPES:
        x, res = rn(rows, cols), rn(rows, cols)
        w = 1 + 0.1 * rn(cols)
        t = rows * cols * 2
        nb = 3 * t + rows * 4 + cols * 2  # x, residual, gamma read; y, rstd written
        tag = f"[{rows}, {cols}]"
        lines.append(f"# ---- norm on x {tag} = {t / 1e6:.1f} MB; the yardstick add_dropout_rms_norm(x, residual) at "
                     "p = 0 with no backward reads x, residual, gamma and writes y, rstd (no z)")
        y = k.rmsnorm_residual_fwd(x, res, w, EPS, True)[0]
        yu = k.rmsnorm_fwd(x, None, w, EPS, 0.0, False)[0] + res
        err = (y.float() - yu.float()).abs().max().item()
        lines.append(f"# max |fused - unfused| = {err:.3e} (the unfused path rounds the norm's output before the add; "
                     f"bf16 outputs of magnitude {yu.float().abs().max().item():.2f})")
        grp = _time_interleaved({
            "add_dropout_rms_norm(x, res) fwd (yardstick)": lambda: k.rmsnorm_fwd(x, res, w, EPS, 0.0, False),
            "rms_norm_residual fwd": lambda: k.rmsnorm_residual_fwd(x, res, w, EPS, True),
            "unfused: rms_norm(x) fwd + eager add": lambda: k.rmsnorm_fwd(x, None, w, EPS, 0.0, False)[0] + res,
        }, args.rounds)
        # unfused, the least it could move: x, gamma read, n, rstd written; then n, residual read, y written
        nbs = (nb, nb, 5 * t + rows * 4 + cols * 2)
        meds = []
        for (name, ts), b in zip(grp.items(), nbs):
            m, line = _row(f"{name} {tag}", ts, b)
            meds.append(m)
            lines.append(line)
        base = next(iter(grp.values()))
        verdicts.append(f"# norm {tag} fwd: rms_norm_residual / add_dropout_rms_norm time {meds[1] / meds[0]:.3f} "
                        f"(the yardstick's own quartile spread {_spread(base):.3f}); unfused / fused "
                        f"{meds[2] / meds[1]:.2f}")
        del x, res, y, yu
    text = "\n".join(lines + verdicts) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
