"""The multi-rank engine case of tests/test_gemma2_ops.py: helpers/engine_cases.py builds its own
config (``case_cfg``) and plan in every spawned rank, so the ranks start here, swap the config for
the Gemma-2 block replica and the plan for one whose stage boundary falls between a decoupled
attention core and its output projection, and then run the unchanged ``engine_cases.worker``."""
import dataclasses

from helpers import engine_cases

from mipipe.models import CONFIGS
from mipipe.parallel.stage import StagePlan, block_costs


def gemma2_cfg(mode=None):
    """A 2-layer d 32 replica of ``gemma2_block_tiny``: 4 query heads over 2 K/V heads of width 16 (A = 64 != E),
    8 tokens, layer 0 with a window of 3 keys and layer 1 global."""
    return dataclasses.replace(CONFIGS["gemma2_block_tiny"], num_layers=2, d_model=32, nhead=4, n_kv_heads=2,
                               head_dim=16, dim_feedforward=64, vocab=100, seq_len=8, window=3,
                               attn_scale=8 ** -0.5)


def cut_after_core(cfg, world, virtual=1, **kwargs):
    """Two stages: [enc, layer 0, core of layer 1] and [the rest]."""
    assert world == 2 and virtual == 1
    costs = block_costs(cfg, False)
    return StagePlan([6, len(costs) - 6], costs, 1, False)


def worker(*args, **kwargs):
    engine_cases.case_cfg = gemma2_cfg
    engine_cases.plan_stages = cut_after_core
    return engine_cases.worker(*args, **kwargs)
