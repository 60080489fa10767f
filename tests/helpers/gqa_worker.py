"""The grouped-query attention kernels behind an environment switch the
extension reads once per process (launched by tests/test_gpu_gqa_kernels.py
with MIPIPE_ATTN_LONG=0 or MIPIPE_ATTN_DKDV8=0).

Runs the native-against-repeated-heads comparison at S=256, D=64 with 4 query
heads over 2 K/V heads, causal and not, without and with dropout, and exits
non-zero on the first mismatch.  MIPIPE_ATTN_LONG=0 sends this shape to the
generic kernels, MIPIPE_ATTN_DKDV8=0 to the 4-wave long-sequence dK/dV kernel."""
import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from helpers.gqa_cases import check_native_against_expanded  # noqa: E402


def main() -> int:
    if os.environ.get("MIPIPE_ATTN_LONG") != "0" and os.environ.get("MIPIPE_ATTN_DKDV8") != "0":
        print("gqa_worker: neither MIPIPE_ATTN_LONG=0 nor MIPIPE_ATTN_DKDV8=0 is set", flush=True)
        return 2
    from mipipe._native_loader import kernels

    kernels()  # raises if the extension is missing
    for causal in (False, True):
        for p in (0.0, 0.1):
            try:
                check_native_against_expanded(2, 256, 4, 2, 64, causal, p)
            except AssertionError:
                traceback.print_exc()
                return 1
            print(f"ok causal={causal} p={p}", flush=True)
    torch.cuda.synchronize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
