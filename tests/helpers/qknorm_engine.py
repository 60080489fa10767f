"""The multi-rank engine case of tests/test_qknorm_ops.py: helpers/engine_cases.py builds its own
config (``case_cfg``) in every spawned rank, so the ranks start here, swap that config for the
QK-norm replica and then run the unchanged ``engine_cases.worker``."""
import dataclasses

from helpers import engine_cases

from mipipe.models import CONFIGS


def qknorm_cfg(mode=None):
    """A 2-layer d 32 replica of ``qwen3_tiny``: 4 query heads over 2 K/V heads of width 8, 8 tokens."""
    return dataclasses.replace(CONFIGS["qwen3_tiny"], d_model=32, nhead=4, n_kv_heads=2, dim_feedforward=64,
                               vocab=100, seq_len=8)


def worker(*args, **kwargs):
    engine_cases.case_cfg = qknorm_cfg
    return engine_cases.worker(*args, **kwargs)
