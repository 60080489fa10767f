"""Document-masked attention (packed sequences) against plain causal attention of
the same build on the same tensors, timed in ONE process and interleaved
(causal, packed, causal, ... so all see the same clocks and the same neighbours
on the box), bf16, causal, p = 0, grouped-query heads read in place:

* B 2, S 8192, H 32, Hkv 8, D 128: both calls on the generic kernels;
* B 8, S 1024, H 24, Hkv 8, D 64: the call with bounds on the generic
  16-rows-per-wave kernels against the causal call on the long-sequence kernels
  -- a comparison of two kernels as well as of two masks.

Packings: equal documents of S / 4 and of S / 16 tokens, one of uneven lengths
that do not sit on the 64-key tile edges, and one document of S tokens -- the
causal mask on the document kernels, which shows what the bounds cost per tile
apart from what the skipping saves.  The kernels visit, per 64-row
tile, only the 64-key tiles between the tile's first document and the diagonal
(forward, dQ) and only the query tiles up to the key tile's last document
(dK/dV); the share of the causal call's tiles they visit is computed from the
bounds and printed next to the measured time ratio.

    python tools/bench_attn_docs.py [--rounds 20] [--out FILE]

Times are device events around single calls, medians over the rounds, with the
quartiles as the spread.  Needs a GPU: there is no CPU fallback.
"""
import argparse
import itertools
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mipipe.utils.data import document_bounds_from_lengths  # noqa: E402
from tools.bench_attn_window import _stat  # noqa: E402
from tools.bench_rowwise_llama import _clock, _time_interleaved  # noqa: E402

CASES = [(2, 8192, 32, 8, 128), (8, 1024, 24, 8, 64)]
TILE = 64


def packings(S):
    """{name: document lengths of one row}."""
    uneven, left = [], S
    for n in itertools.cycle((S // 8 + 37, S // 16 - 19, S // 4 + 5, S // 32 + 11)):
        n = min(n, left)
        uneven.append(n)
        left -= n
        if left == 0:
            break
    assert all(sum(uneven[:i]) % TILE for i in range(1, len(uneven)))  # no boundary on a tile edge
    return {f"1 x {S}": [S], f"4 x {S // 4}": [S // 4] * 4, f"16 x {S // 16}": [S // 16] * 16,
            f"uneven ({len(uneven)} docs)": uneven}


def tile_shares(bounds, S):
    """(forward / dQ, dK/dV) visited 64 x 64 tiles over the causal call's, from row 0 of ``bounds [B, 2, S]``
    (every row has the same packing here), as the kernels pick their loop bounds."""
    n = S // TILE
    start, end = bounds[0, 0].tolist(), bounds[0, 1].tolist()
    causal = n * (n + 1) // 2
    fwd = sum(qt - start[TILE * qt] // TILE + 1 for qt in range(n))
    dkv = sum((end[TILE * kt + TILE - 1] - 1) // TILE + 1 - kt for kt in range(n))
    return fwd / causal, dkv / causal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_docs.py measures GPU kernels: no GPU found")
    from mipipe._native_loader import kernels

    k = kernels()
    dev, bf = "cuda", torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(7)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g).to(bf)  # noqa: E731
    lines = [f"# tools/bench_attn_docs.py --rounds {args.rounds}",
             f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}, {time.strftime('%Y-%m-%d %H:%M:%S')}",
             f"# clock: {_clock()}; {args.rounds} interleaved rounds per group after 5 warm-up rounds; bf16, causal, p = 0",
             "# tiles / causal: forward and dQ visit the first share, dK/dV the second (the backward line shows their mean)",
             "# call                                              median      [quartiles]       time / causal   tiles / causal"]
    for B, S, H, Hkv, D in CASES:
        scale = 1.0 / math.sqrt(D)
        qkv = rn(B, S, H + 2 * Hkv, D)
        q, kk, v = qkv[:, :, :H], qkv[:, :, H:H + Hkv], qkv[:, :, H + Hkv:]
        do = rn(B, S, H, D)
        dqkv = torch.empty_like(qkv)
        dq, dk, dv = dqkv[:, :, :H], dqkv[:, :, H:H + Hkv], dqkv[:, :, H + Hkv:]
        tag = f"B{B} S{S} H{H}/{Hkv} D{D}"
        lines.append(f"# {tag}: causal on the {'long-sequence' if k.attention_long_supported(S, D) else 'generic'} "
                     "kernels, documents on the generic ones")
        docs = {"causal": None}
        for name, lengths in packings(S).items():
            docs[name] = document_bounds_from_lengths([lengths] * B, S, device=dev)
        outs = {n: k.attention_fwd(q, kk, v, True, 0.0, scale, doc_bounds=d) for n, d in docs.items()}
        fwd = _time_interleaved({n: (lambda d=d: k.attention_fwd(q, kk, v, True, 0.0, scale, doc_bounds=d))
                                 for n, d in docs.items()}, args.rounds)
        bwd = _time_interleaved({n: (lambda n=n, d=d: k.attention_bwd(do, q, kk, v, outs[n][0], outs[n][1], True, 0.0,
                                                                       scale, 0, 0, dq, dk, dv, None, 0, 0, 0.0, d))
                                 for n, d in docs.items()}, args.rounds)
        for what, res in (("fwd", fwd), ("bwd", bwd)):
            c, c1, c3 = _stat(res["causal"])
            lines.append(f"{tag + ' ' + what + ' causal':50s} {c:9.1f} us  [{c1:8.1f}, {c3:8.1f}]")
            for n, d in docs.items():
                if d is None:
                    continue
                m, q1, q3 = _stat(res[n])
                sf, sk = tile_shares(d.cpu(), S)
                share = sf if what == "fwd" else (sf + sk) / 2
                lines.append(f"{tag + ' ' + what + ' ' + n:50s} {m:9.1f} us  [{q1:8.1f}, {q3:8.1f}]  "
                             f"{m / c:12.3f}   {share:12.3f}")
        del qkv, dqkv, do, outs
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
