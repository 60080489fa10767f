"""The multi-rank engine case of tests/test_moe_ops.py: helpers/engine_cases.py builds its own config
(``case_cfg``) in every spawned rank, so the ranks start here, swap that config for the mixture-of-experts
replica and then run the unchanged ``engine_cases.worker``.  The engine the helper builds is wrapped so that
every rank (and the single-rank reference) also asserts the ``aux_scale`` the engine gave its MoE blocks."""
import dataclasses

from helpers import engine_cases

from mipipe.models import CONFIGS
from mipipe.models.transformer import MoEFeedForwardBlock
from mipipe.parallel import PipelineEngine


def moe_cfg(mode=None):
    """A 2-layer d 32 replica of ``moe_tiny``: 4 experts of width 64, top-2, 8 tokens, a window of 3."""
    return dataclasses.replace(CONFIGS["moe_tiny"], d_model=32, nhead=4, n_kv_heads=2, dim_feedforward=64,
                               vocab=100, seq_len=8, window=3)


def checked_engine(modules, **kwargs):
    """``PipelineEngine(modules, **kwargs)`` after asserting ``aux_scale = 1 / (chunks * grad_divisor)`` on every
    MoE block; a rank must own at least one."""
    eng = PipelineEngine(modules, **kwargs)
    blocks = [m for mod in eng.modules for m in mod.modules() if isinstance(m, MoEFeedForwardBlock)]
    assert blocks, "no mixture-of-experts block on this rank"
    want = 1.0 / (eng.chunks * eng.grad_divisor)
    assert eng.chunks > 1 and all(b.aux_scale == want for b in blocks), ([b.aux_scale for b in blocks], want)
    return eng


def worker(*args, **kwargs):
    engine_cases.case_cfg = moe_cfg
    engine_cases.PipelineEngine = checked_engine
    return engine_cases.worker(*args, **kwargs)
