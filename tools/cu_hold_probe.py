#!/usr/bin/env python3
"""What a resident RCCL-shaped kernel holding k CUs costs a training step.

VERDICT r4 "What's missing" #1: an RCCL receive is a kernel that spins on its
CUs until the data lands, and the pipeline engine pre-posts its receives, so
one sits resident through most of a phase.  Our 256x256 GEMM block takes a
whole CU (512 threads, ~240 VGPRs, 130-160 KiB of LDS) and its grids are
exact multiples of 256 tiles, so one lost CU can turn a 2-round GEMM into 3.

For each k this starts ``tools/micro/bin/cu_hold k`` (k blocks with the
footprint of torch's RCCL ``rcclGenericKernel``: 256 threads, 19.7 KiB LDS,
one wave per SIMD) in its own process, waits until every block is resident,
runs ``bench.py`` beside it and releases the blocks.  Prints one line per run
and a table of step time vs k.

    python tools/cu_hold_probe.py --ks 0,1,2,4,8,16,0 --bench "--steps 20 --warmup 5"
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOLD = os.path.join(ROOT, "tools", "micro", "bin", "cu_hold")


def run_one(k: int, bench_args: list[str], out_dir: str, timeout: float) -> dict:
    ready = os.path.join(out_dir, f"hold_ready_{os.getpid()}")
    rel = os.path.join(out_dir, f"hold_release_{os.getpid()}")
    for p in (ready, rel):
        if os.path.exists(p):
            os.remove(p)
    hold = subprocess.Popen([HOLD, str(k), str(timeout + 120), ready, rel], stdout=subprocess.PIPE,
                            stderr=subprocess.STDOUT, text=True)
    try:
        t0 = time.time()
        while not os.path.exists(ready):
            if hold.poll() is not None:
                raise RuntimeError(f"cu_hold exited early: {hold.stdout.read()}")
            if time.time() - t0 > 60:
                raise RuntimeError("cu_hold not ready after 60 s")
            time.sleep(0.05)
        t1 = time.time()
        res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *bench_args], capture_output=True,
                             text=True, timeout=timeout, cwd=ROOT)
        wall = time.time() - t1
    finally:
        open(rel, "w").close()
        try:
            hold.wait(timeout=60)
        except subprocess.TimeoutExpired:
            hold.kill()
            raise
    if res.returncode != 0:
        raise RuntimeError(f"bench rc={res.returncode}: {res.stderr[-2000:]}")
    line = [ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1]
    js = json.loads(line)
    return {"k": k, "value": js["value"], "ms": js["ms_per_step"], "wall_s": round(wall, 1),
            "telemetry": js.get("telemetry")}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="0,1,2,4,8,16,0")
    ap.add_argument("--bench", default="--full --steps 20 --warmup 5",
                    help="bench.py arguments (--full: the JSON telemetry printed per run)")
    ap.add_argument("--label", default="enc12 PP=1")
    ap.add_argument("--timeout", type=float, default=400.0)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "gpurun_out"))
    args = ap.parse_args()
    os.makedirs(args.out_dir, exist_ok=True)
    ks = [int(x) for x in args.ks.split(",")]
    rows = []
    for k in ks:
        r = run_one(k, args.bench.split(), args.out_dir, args.timeout)
        rows.append(r)
        print(f"[{args.label}] k={k:3d}  {r['value']:>10.1f} tok/s  {r['ms']:9.3f} ms/step  (bench wall {r['wall_s']} s)"
              f"  telemetry={r['telemetry']}", flush=True)
    base = [r["ms"] for r in rows if r["k"] == 0]
    b = sum(base) / len(base) if base else None
    print(f"# {args.label}: bench.py {args.bench}; k blocks of an RCCL-shaped resident kernel beside the step")
    print("#   k   ms/step   vs k=0")
    for r in rows:
        rel = f"{100.0 * (r['ms'] / b - 1.0):+6.1f} %" if b else "   n/a"
        print(f"  {r['k']:3d}  {r['ms']:9.3f}  {rel}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
