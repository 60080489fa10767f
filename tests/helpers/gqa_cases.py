"""Shared case code of tests/test_gpu_gqa_kernels.py and its worker
(tests/helpers/gqa_worker.py): the native grouped-query attention kernels
against the existing kernels on repeated K/V heads.

Both runs do the same arithmetic on the same values (a query head's block
reads the same K and V numbers, from another address), so ``o`` and ``dq`` are
compared bit for bit.  ``dk`` / ``dv`` of the native run are one rounding of an
fp32 sum of the group's (at most 6) bf16 partials, which the expanded run
leaves in its leaves' ``.grad``: they are compared against the fp64 sum of
those partials at the project's bf16 bound ``2**-8 |ref| + 1e-4``
(``rowwise_cases.assert_close``); the fp32 sum's own error is below
``2**-24 * sum|partial|``, inside the absolute term for randn inputs."""
import torch

from helpers.rowwise_cases import assert_close

DEV = "cuda"
HEADS = [(4, 4), (4, 2), (4, 1), (6, 2)]


def expand(qkv, H, Hkv):
    """``[B, S, H + 2 Hkv, D]`` -> ``[B, S, 3, H, D]``, K/V heads repeated per group (a plain copy)."""
    g = H // Hkv
    q = qkv[:, :, :H]
    k = qkv[:, :, H:H + Hkv].repeat_interleave(g, dim=2)
    v = qkv[:, :, H + Hkv:].repeat_interleave(g, dim=2)
    return torch.stack((q, k, v), dim=2).contiguous()


def gqa_inputs(B, S, H, Hkv, D, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed + 131 * S + 7 * D + H * 3 + Hkv)
    qkv = torch.randn(B, S, H + 2 * Hkv, D, device=DEV, generator=g).to(torch.bfloat16)
    do = torch.randn(B, S, H, D, device=DEV, generator=g).to(torch.bfloat16)
    return qkv, do


def run_native(qkv, do, Hkv, causal, p, seed=11):
    from mipipe.ops import attention_gqa_packed

    x = qkv.clone().requires_grad_()
    torch.manual_seed(seed)  # the device generator: the Philox draw of the dropout mask
    o = attention_gqa_packed(x, Hkv, causal=causal, dropout_p=p, training=True)
    o.backward(do)
    return o.detach(), x.grad


def run_expanded(qkv, do, H, Hkv, causal, p, seed=11):
    from mipipe.ops import attention_packed

    x5 = expand(qkv, H, Hkv).requires_grad_()
    torch.manual_seed(seed)
    o = attention_packed(x5, causal=causal, dropout_p=p, training=True)
    o.backward(do)
    return o.detach(), x5.grad


def check_native_against_expanded(B, S, H, Hkv, D, causal, p=0.0):
    """Raises AssertionError naming the first tensor that differs."""
    qkv, do = gqa_inputs(B, S, H, Hkv, D)
    tag = f"B{B} S{S} H{H}/{Hkv} D{D} causal={causal} p={p}"
    o, dqkv = run_native(qkv, do, Hkv, causal, p)
    o5, d5 = run_expanded(qkv, do, H, Hkv, causal, p)
    torch.cuda.synchronize()
    assert o.shape == (B, S, H, D) and dqkv.shape == qkv.shape
    assert torch.isfinite(o.float()).all() and torch.isfinite(dqkv.float()).all(), tag
    assert torch.equal(o, o5), tag + ": o"
    assert torch.equal(dqkv[:, :, :H], d5[:, :, 0]), tag + ": dq"
    g = H // Hkv
    for name, lo, which in (("dk", H, 1), ("dv", H + Hkv, 2)):
        ref = d5[:, :, which].double().view(B, S, Hkv, g, D).sum(3)
        assert_close(dqkv[:, :, lo:lo + Hkv], ref, torch.bfloat16, f"{tag}: {name}")
    if Hkv == H:  # the same layout byte for byte: the whole gradient equals attention_packed's
        assert torch.equal(dqkv.view(B, S, 3, H, D), d5), tag + ": dqkv"
