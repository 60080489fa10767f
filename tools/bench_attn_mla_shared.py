"""Multi-head latent attention's shared rope key head read in place (``ops.attention(..., k_rope=)``, the SHARED
kernels of attention_mla.hip) against what a caller had to do without it: broadcast the one rope head to all heads,
concatenate it behind every head's nope features and pass the ``[B, S, H, 192]`` tensor to ``ops.attention``, with
autograd slicing and summing the gradient back.  Both sides run the same values in ONE process, interleaved, bf16,
causal, p = 0:

* B 2, S 4096, H 16 (DeepSeek-V2-Lite's heads) and B 1, S 4096, H 128 (DeepSeek-V3's);
* k_nope and v are the two halves of one ``[B, S, H, 256]`` tensor (the up-projection's output), read in place;
* forward: the call, the baseline's concatenation included; backward: ``autograd.grad`` of the result to q, k_nope,
  v and k_rope (the baseline's includes the concatenation's backward: the slice and the sum over the heads);
* each ratio stands next to the baseline's own quartile spread (q3 / q1): a ratio inside it is not resolved.

    python tools/bench_attn_mla_shared.py [--rounds 20] [--out FILE]

Times are device events around single calls, medians over the rounds, with the quartiles as the spread.  Nothing is
fixed in advance: the file records what was measured.  Needs a GPU: there is no CPU fallback.
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_attn_mla import CASES, _stat  # noqa: E402
from tools.bench_rowwise_llama import _clock, _time_interleaved  # noqa: E402

DN, R, DV = 128, 64, 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_mla_shared.py measures GPU kernels: no GPU found")
    from mipipe import ops

    dev, bf = "cuda", torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(7)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g).to(bf)  # noqa: E731
    lines = [f"# tools/bench_attn_mla_shared.py --rounds {args.rounds}",
             f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}, {time.strftime('%Y-%m-%d %H:%M:%S')}",
             f"# clock: {_clock()}; {args.rounds} interleaved rounds per group after 5 warm-up rounds; bf16, causal, "
             "p = 0, head dims (128 + 64, 128)",
             "# call                                                    median      [quartiles]       "
             "shared / concat   concat q3 / q1"]
    for B, S, H in CASES:
        q = rn(B, S, H, DN + R).transpose(1, 2).requires_grad_()
        kv = rn(B, S, H, DN + DV).transpose(1, 2)
        kn, v = kv[..., :DN].requires_grad_(), kv[..., DN:].requires_grad_()
        kr = rn(B, S, R).requires_grad_()
        do = rn(B, S, H, DV).transpose(1, 2)
        leaves = (q, kn, v, kr)

        def concat():
            return ops.attention(q, torch.cat([kn, kr[:, None].expand(-1, H, -1, -1)], -1), v, True)

        run = {"shared": lambda: ops.attention(q, kn, v, True, k_rope=kr), "concat": concat}
        outs = {n: fn() for n, fn in run.items()}
        same = torch.equal(outs["shared"], outs["concat"])
        fwd = _time_interleaved(run, args.rounds)
        bwd = _time_interleaved({n: (lambda o=o: torch.autograd.grad(o, leaves, do, retain_graph=True))
                                 for n, o in outs.items()}, args.rounds)
        tag = f"B{B} S{S} H{H}"
        for what, res in (("fwd", fwd), ("bwd", bwd)):
            u, u1, u3 = _stat(res["concat"])
            m, m1, m3 = _stat(res["shared"])
            lines.append(f"{tag + ' ' + what + ' cat(k_nope, k_rope) + attention':56s} {u:9.1f} us  [{u1:8.1f}, {u3:8.1f}]")
            lines.append(f"{tag + ' ' + what + ' k_rope= (read in place)':56s} {m:9.1f} us  [{m1:8.1f}, {m3:8.1f}]  "
                         f"{m / u:12.3f}   {u3 / u1:14.3f}")
        lines.append(f"{tag + ' o bit-identical':56s} {same}")
        del q, kv, kn, v, kr, do, leaves, outs, run
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
