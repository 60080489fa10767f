"""The multi-rank engine case of tests/test_moe_grouped_ops.py: helpers/moe_engine.py's worker with the dropless
grouped-GEMM experts (``expert_gemm="grouped"``, ``capacity_factor=None``) in the replica's config.  The wrapped
engine also asserts that every MoE block of the rank runs the grouped path."""
import dataclasses

from helpers import engine_cases, moe_engine

from mipipe.models.transformer import MoEFeedForwardBlock


def moe_cfg(mode=None):
    """helpers.moe_engine's replica of ``moe_tiny`` with the grouped experts."""
    return dataclasses.replace(moe_engine.moe_cfg(mode), expert_gemm="grouped", capacity_factor=None)


def checked_engine(modules, **kwargs):
    eng = moe_engine.checked_engine(modules, **kwargs)
    blocks = [m for mod in eng.modules for m in mod.modules() if isinstance(m, MoEFeedForwardBlock)]
    assert all(b.expert_gemm == "grouped" and b.capacity_factor is None for b in blocks)
    return eng


def worker(*args, **kwargs):
    engine_cases.case_cfg = moe_cfg
    engine_cases.PipelineEngine = checked_engine
    return engine_cases.worker(*args, **kwargs)
