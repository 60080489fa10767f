"""The multi-rank engine case of tests/test_sink_ops.py: helpers/engine_cases.py builds its own config
(``case_cfg``) in every spawned rank, so the ranks start here, swap that config for the replica with attention
sinks and then run the unchanged ``engine_cases.worker``."""
import dataclasses

from helpers import engine_cases

from mipipe.models import CONFIGS


def sink_cfg(mode=None):
    """A 2-layer d 32 replica of ``sink_tiny``: 4 query heads (each with a sink) over 2 K/V heads, 8 tokens, a
    window of 3."""
    return dataclasses.replace(CONFIGS["sink_tiny"], d_model=32, nhead=4, n_kv_heads=2, dim_feedforward=64,
                               vocab=100, seq_len=8, window=3)


def worker(*args, **kwargs):
    engine_cases.case_cfg = sink_cfg
    return engine_cases.worker(*args, **kwargs)
