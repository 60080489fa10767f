"""The multi-rank engine case of tests/test_softcap_ops.py: helpers/engine_cases.py builds its own
config (``case_cfg``) in every spawned rank, so the ranks start here, swap that config for the
soft-capped replica and then run the unchanged ``engine_cases.worker``."""
import dataclasses

from helpers import engine_cases

from mipipe.models import CONFIGS


def softcap_cfg(mode=None):
    """A 2-layer d 32 replica of ``gemma2_tiny``: 4 query heads over 2 K/V heads, 8 tokens, a window of 3, and
    caps small enough to bite at initialisation (0.5 on the attention scores, 1.0 on the logits)."""
    return dataclasses.replace(CONFIGS["gemma2_tiny"], d_model=32, nhead=4, n_kv_heads=2, dim_feedforward=64,
                               vocab=100, seq_len=8, window=3, attn_softcap=0.5, final_softcap=1.0)


def worker(*args, **kwargs):
    engine_cases.case_cfg = softcap_cfg
    return engine_cases.worker(*args, **kwargs)
