"""The multi-rank engine case of tests/test_document_ops.py: two gloo CPU ranks run one
``PipelineEngine.step(..., doc_bounds=...)`` on a packed batch -- every rank gets the bounds, as every
stage's attention cores need them -- and the caller compares loss and gradients with the unpipelined
model run under ``ops.use_documents``.  The worker is this module's own (helpers/engine_cases.py's
passes no bounds); it borrows that module's data, naming and port helpers."""
import dataclasses
import os
import queue as _queue
import time as _time

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from helpers import engine_cases

from mipipe import ops
from mipipe.models import CONFIGS, TargetSequential, build_lm_blocks, lm_pipeline_units
from mipipe.models.transformer import merge_units
from mipipe.optim import FlatAdam
from mipipe.parallel import PipelineEngine, plan_stages
from mipipe.parallel.stage import stage_input_shape
from mipipe.utils.data import document_bounds

EOS = 0
M, MB = 4, 2


def documents_cfg(window=5):
    """A 4-layer d 32 replica of ``mistral_tiny``: 4 query heads over 2 K/V heads, 16 tokens of a 16-word
    vocabulary (so every row holds a few EOS tokens) and a window of 5 that the bounds are merged with."""
    return dataclasses.replace(CONFIGS["mistral_tiny"], num_layers=4, d_model=32, nhead=4, n_kv_heads=2,
                               dim_feedforward=64, vocab=16, seq_len=16, window=window)


def packed_data(cfg):
    """Per-micro-batch inputs, targets and bounds; at least one row holds two or more documents."""
    inputs, targets = engine_cases._data(cfg, M, MB)
    bounds = [document_bounds(x, EOS) for x in inputs]
    assert any(int(b[:, 0].max()) > 0 for b in bounds)
    return inputs, targets, bounds


def worker(rank, world, port, checkpoint, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cfg = documents_cfg()
        dev = torch.device("cpu")
        torch.manual_seed(0)
        full = torch.nn.Sequential(*build_lm_blocks(cfg))
        names = {id(p): n for n, p in full.named_parameters()}
        units = lm_pipeline_units(list(full.children()), split_decoder=False)
        plan = plan_stages(cfg, world, 1, split_decoder=False)
        chunks = [TargetSequential(*merge_units([units[i] for i in plan.slice(s)])).train()
                  for s in plan.vstages(rank)]
        stage = torch.nn.ModuleList(chunks)
        opt = FlatAdam(stage.parameters(), lr=1e-3)
        eng = PipelineEngine(chunks, chunks=M, checkpoint=checkpoint,
                             act_shape=[stage_input_shape(cfg, plan, s, MB) for s in plan.vstages(rank)],
                             act_dtype=torch.float32,
                             loss_fn=engine_cases._loss_fn(cfg) if rank == world - 1 else None, device=dev,
                             watchdog=120.0, transport="rccl")
        inputs, targets, bounds = packed_data(cfg)
        opt.zero_grad()
        st = eng.step(inputs if rank == 0 else None, targets, doc_bounds=bounds)  # the bounds on EVERY rank
        opt.fold_grads()
        assert ops.current_documents() is None
        q.put((rank, None if st.loss is None else float(st.loss), engine_cases._grads(stage.parameters(), names)))
        q.close()
        q.join_thread()
    finally:
        dist.destroy_process_group()


def unpipelined_reference(documents=True):
    """Loss and gradients of the whole model on the whole batch in one call under ``use_documents``."""
    cfg = documents_cfg()
    torch.manual_seed(0)
    model = torch.nn.Sequential(*build_lm_blocks(cfg)).train()
    inputs, targets, bounds = packed_data(cfg)
    with ops.use_documents(torch.cat(bounds) if documents else None):
        loss = engine_cases._loss_fn(cfg)(model(torch.cat(inputs)), torch.cat(targets))
    loss.backward()
    return float(loss.detach()), {n: p.grad.clone() for n, p in model.named_parameters()}


def run_documents_engine_case(world=2, checkpoint="always"):
    ref_loss, ref = unpipelined_reference()
    plain_loss, _ = unpipelined_reference(documents=False)
    assert abs(plain_loss - ref_loss) > 1e-4 * abs(ref_loss)  # the mask matters on this batch
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = engine_cases._port()
    procs = [ctx.Process(target=worker, args=(r, world, port, checkpoint, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = []
    deadline = _time.time() + 300
    try:
        while len(results) < world:
            try:
                results.append(q.get(timeout=1.0))
            except _queue.Empty:
                dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
                if dead or _time.time() > deadline:
                    raise AssertionError(f"rank(s) failed (exit codes {dead}) or timed out; "
                                         f"{len(results)}/{world} results")
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.exitcode is None:
                p.kill()
    seen = set()
    for rank, loss, grads in sorted(results, key=lambda r: r[0]):
        if loss is not None:  # engine_cases.run_engine_case's CPU bounds
            assert abs(loss - ref_loss) < 1e-5 * abs(ref_loss), (loss, ref_loss)
        for name, g in grads.items():
            r = ref[name]
            assert (torch.from_numpy(g) - r).abs().max().item() <= 1e-4 * (r.abs().max().item() + 1e-6), name
            seen.add(name)
    assert seen == set(ref)
