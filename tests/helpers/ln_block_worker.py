"""LayerNorm's one-row-per-block kernels at widths the wave-per-row kernels
normally take (launched by tests/test_gpu_rowwise_edges.py with
MIPIPE_LN_ROWS=0, which the extension reads once per process).

Runs the forward/backward comparison against fp64 at 8, 256, 1600 and 2048
columns -- ln_fwd_kernel / ln_bwd_kernel<T, 1, 2>, reachable no other way --
and exits non-zero on the first mismatch."""
import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from helpers.rowwise_cases import check_layernorm  # noqa: E402

# rows: 1 and 7 (fewer rows than the two row groups of a block / an odd count),
# 1100 (three trips of the 256-block, two-row grid: an odd trip count), 67, and
# 530 (two trips, the second partly filled)
CASES = [(8, 1), (8, 7), (256, 1100), (1600, 67), (2048, 530)]


def main() -> int:
    if os.environ.get("MIPIPE_LN_ROWS") != "0":
        print("ln_block_worker: MIPIPE_LN_ROWS=0 is not set", flush=True)
        return 2
    from mipipe._native_loader import kernels

    kernels()  # raises if the extension is missing
    for cols, rows in CASES:
        for dtype in (torch.float32, torch.bfloat16):
            for residual in (False, True):
                try:
                    check_layernorm(cols, rows, dtype, residual)
                except AssertionError:
                    traceback.print_exc()
                    return 1
                print(f"ok {rows}x{cols} {dtype} residual={residual}", flush=True)
    torch.cuda.synchronize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
