"""The bf16 store pass of the 256-row GEMM kernel per side-operand mode (none, the
addend ``res``, the ReLU bit mask, a saved activation) and the staged dropout / aux
epilogue, on interior tiles (straight-line: loads grouped ahead of the stores) and on
edge tiles (predicated per chunk) of ONE launch.

Shapes are the smallest with an interior and an edge tile in both directions: T in
{264, 520}; N in {264, 520} at block width 256 and {136, 264} at width 128 (forced
with ``gemm_set_width``); inner dimension 64 (one K-tile) and 192.

Two checks per case:
 (a) against the fp32 torch reference, the dropout mask rebuilt from the Philox
     layout (common.h drop_sub: block (row / 4) * (N / 2) + col / 2, word row % 4,
     half col % 2).  Tolerances are those of test_gpu_kernels.py for the same
     epilogues: test_linear_residual_epilogue (forward atol = rtol = 3e-2, the
     input gradient atol 6e-2, rtol 5e-2), test_linear_dgrad_activation_backward_epilogue
     (max error over max magnitude < 1e-2, 2e-2 for a saved GELU'), the dropout
     forward of test_gemm_round_chunks (atol 5e-2, rtol 3e-2) and, for the bits,
     test_relu_bits_fold_bit_exact (the packed nonzeros of the output, exactly).
 (b) interior against edge, bit for bit: the same inputs run on the full problem
     and on its T / N prefixes.  Rows 256-263 (columns alike) are interior in the
     larger launch and in an edge tile in the smaller one, and the K loop of an
     output element does not depend on the launch, so the common part is equal
     bitwise.  With dropout the mask's row length is N, so only T prefixes share a
     mask (the bindings take no mask coordinates); the CPU test below checks that
     the rebuilt mask itself has that prefix property for the seeds used here."""
import math

import numpy as np
import pytest
import torch

from test_gpu_kernels import _philox4x32_10

DEV = "cuda"
gpu = pytest.mark.gpu

T_FULL, T_PART = 520, 264
N_BY_WIDTH = {256: (520, 264), 128: (264, 136)}  # (full, prefix)
KS = (64, 192)
SEED = 1234
P = 0.2


@pytest.fixture(scope="module")
def k():
    from mipipe._native_loader import kernels

    return kernels()


@pytest.fixture(params=[256, 128])
def width(request, k):
    k.gemm_set_width(request.param)
    try:
        yield request.param
    finally:
        k.gemm_set_width(0)


def _keep_mask(rows, cols, p, seed, offset):
    """Dropout keep mask of an [rows, cols] GEMM output (common.h drop_sub / drop_keep)."""
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    sub = (r >> 2).astype(np.uint64) * np.uint64(cols >> 1) + (c >> 1).astype(np.uint64)
    seed &= 0xFFFFFFFFFFFFFFFF
    offset &= 0xFFFFFFFFFFFFFFFF
    m32 = np.uint64(0xFFFFFFFF)
    words = _philox4x32_10(sub & m32, sub >> np.uint64(32), np.uint64(offset) & m32, np.uint64(offset) >> np.uint64(32),
                           seed & 0xFFFFFFFF, seed >> 32)
    w = np.choose(r & 3, words)
    u16 = (w >> (np.uint64(16) * (c & 1).astype(np.uint64))) & np.uint64(0xFFFF)
    thr16 = min(int(p * 4294967296.0), 0xFFFFFFFF) >> 16
    return torch.from_numpy(u16 >= np.uint64(thr16))


def test_rebuilt_mask_has_the_row_prefix_property():
    """The reference mask of the T = 264 launch is the first 264 rows of the T = 520 one
    (same N), for the seed used below and the offsets a fresh generator hands out."""
    for n in (136, 264, 520):
        for offset in (0, 4):
            full = _keep_mask(T_FULL, n, P, SEED, offset)
            part = _keep_mask(T_PART, n, P, SEED, offset)
            assert torch.equal(full[:T_PART], part)
            assert abs(full.float().mean().item() - (1 - P)) < 0.02


def _rel(got, ref):
    return ((got.float() - ref).abs().max() / ref.abs().max()).item()


def _gelu_grad(s):
    return 0.5 * (1 + torch.erf(s / math.sqrt(2))) + s * torch.exp(-0.5 * s * s) / math.sqrt(2 * math.pi)


def _rand(*shape, scale=1.0, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, device=DEV, generator=g) * scale).to(torch.bfloat16)


def _prefixes(width):
    nf, npart = N_BY_WIDTH[width]
    return nf, [(T_FULL, npart), (T_PART, nf), (T_PART, npart)]


def _check_prefixes(run, width, along_n=True):
    """run(T, N) -> tuple of outputs on the [T, N] prefix of the problem; every prefix launch must
    reproduce the full launch's bits.  Returns the full launch's outputs."""
    nf, parts = _prefixes(width)
    full = run(T_FULL, nf)

    def same(got, ref, t, n):
        for a, b in zip(got, ref):
            assert torch.equal(a, b[:t, :a.shape[1]]), (t, n)

    if along_n:
        for t, n in parts:
            same(run(t, n), full, t, n)
    else:  # a mask of its own per N: T prefixes only, at both N
        same(run(T_PART, nf), full, T_PART, nf)
        npart = N_BY_WIDTH[width][1]
        same(run(T_PART, npart), run(T_FULL, npart), T_PART, npart)
    return full


# ------------------------------------------------------------------ dgrad: dx = dy . w (x mask) (+ res)
@gpu
@pytest.mark.parametrize("K", KS)
def test_dgrad_res_strided(k, width, K):
    nf, _ = _prefixes(width)
    dy = _rand(T_FULL, K, seed=1)
    w = _rand(K, nf, scale=1 / math.sqrt(K), seed=2)
    wide = _rand(T_FULL, nf + 72, seed=3)  # res: a column slice of a wider tensor (ldr != ldc)

    def run(t, n):
        return (k.linear_dgrad(dy[:t], w[:, :n], wide[:t, 8:8 + n]),)

    (dx,) = _check_prefixes(run, width)
    ref = dy.float() @ w.float() + wide[:, 8:8 + nf].float()
    assert torch.allclose(dx.float(), ref, atol=6e-2, rtol=5e-2)


@gpu
@pytest.mark.parametrize("K", KS)
def test_dgrad_relu_bits(k, width, K):
    nf, _ = _prefixes(width)
    dy = _rand(T_FULL, K, seed=4)
    w = _rand(K, nf, scale=1 / math.sqrt(K), seed=5)
    g = torch.Generator(device=DEV).manual_seed(6)
    bits = torch.randint(0, 256, (T_FULL, nf // 8), device=DEV, generator=g, dtype=torch.uint8)

    def run(t, n):
        return (k.linear_dgrad(dy[:t], w[:, :n], None, None, 4, bits[:t, :n // 8].contiguous(), P, 0, 0),)

    (dx,) = _check_prefixes(run, width)
    mask = ((bits.unsqueeze(-1) >> torch.arange(8, device=DEV, dtype=torch.uint8)) & 1).reshape(T_FULL, nf).float()
    ref = (dy.float() @ w.float()) * mask / (1 - P)
    assert _rel(dx, ref) < 1e-2
    assert (dx[mask == 0] == 0).all()  # masked-off elements are exact zeros


@gpu
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("act,with_res", [(2, False), (2, True), (3, False), (1, False)])
def test_dgrad_saved_activation(k, width, K, act, with_res):
    """act 2: saved = the GELU pre-activation; 3: saved = GELU'(pre); 1: saved = the ReLU output."""
    nf, _ = _prefixes(width)
    dy = _rand(T_FULL, K, seed=7)
    w = _rand(K, nf, scale=1 / math.sqrt(K), seed=8)
    pre = _rand(T_FULL, nf, seed=9)
    saved = {2: pre, 3: _gelu_grad(pre.float()).to(torch.bfloat16), 1: torch.relu(pre)}[act]
    wide = _rand(T_FULL, nf + 72, seed=10)

    def run(t, n):
        res = wide[:t, 8:8 + n] if with_res else None
        return (k.linear_dgrad(dy[:t], w[:, :n], res, None, act, saved[:t, :n], 0.0, 0, 0),)

    (dx,) = _check_prefixes(run, width)
    d = {2: _gelu_grad(pre.float()), 3: saved.float(), 1: (pre > 0).float()}[act]
    ref = (dy.float() @ w.float()) * d
    if with_res:
        ref = ref + wide[:, 8:8 + nf].float()
    assert _rel(dx, ref) < (2e-2 if act == 3 else 1e-2)


@gpu
def test_dgrad_saved_gelu_with_dropout(k, width):
    """p > 0: the staged epilogue regenerates the forward's mask and multiplies by GELU'(saved)."""
    nf, _ = _prefixes(width)
    K = 192
    dy = _rand(T_FULL, K, seed=11)
    w = _rand(K, nf, scale=1 / math.sqrt(K), seed=12)
    pre = _rand(T_FULL, nf, seed=13)

    def run(t, n):
        return (k.linear_dgrad(dy[:t], w[:, :n], None, None, 2, pre[:t, :n], P, SEED, 4),)

    (dx,) = _check_prefixes(run, width, along_n=False)
    keep = _keep_mask(T_FULL, nf, P, SEED, 4).to(DEV).float()
    ref = (dy.float() @ w.float()) * keep / (1 - P) * _gelu_grad(pre.float())
    assert _rel(dx, ref) < 1e-2
    assert (dx[keep == 0] == 0).all()


# ------------------------------------------------------------------ forward: y = (res +) drop(act(x . w^T + b))
@gpu
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("bias,with_res", [(True, False), (False, False), (True, True)])
def test_forward_bias_and_res(k, width, K, bias, with_res):
    nf, _ = _prefixes(width)
    x = _rand(T_FULL, K, seed=14)
    w = _rand(nf, K, scale=1 / math.sqrt(K), seed=15)
    b = _rand(nf, seed=16) if bias else None
    wide = _rand(T_FULL, nf + 72, seed=17)

    def run(t, n):
        res = wide[:t, 8:8 + n] if with_res else None
        return (k.linear_fwd(x[:t], w[:n], None if b is None else b[:n], 0, 0.0, False, res)[0],)

    (y,) = _check_prefixes(run, width)
    ref = x.float() @ w.float().t()
    if bias:
        ref = ref + b.float()
    if with_res:
        ref = ref + wide[:, 8:8 + nf].float()
    assert torch.allclose(y.float(), ref, atol=3e-2, rtol=3e-2)


@gpu
@pytest.mark.parametrize("K", KS)
def test_forward_relu_dropout_bits(k, width, K):
    nf, _ = _prefixes(width)
    x = _rand(T_FULL, K, seed=18)
    w = _rand(nf, K, scale=1 / math.sqrt(K), seed=19)
    b = _rand(nf, seed=20)
    draws = []

    def run(t, n):
        assert k.linear_bits_ok(t, n, K, 1, P)
        bits = torch.zeros(t, n // 8, dtype=torch.uint8, device=DEV)
        torch.cuda.manual_seed(SEED)  # every launch draws the same (seed, offset)
        y, _, seed, offset = k.linear_fwd(x[:t], w[:n], b[:n], 1, P, False, None, None, False, bits)
        draws.append((seed, offset))
        return y, bits

    y, bits = _check_prefixes(run, width, along_n=False)
    assert len(set(draws)) == 1
    seed, offset = draws[0]
    keep = _keep_mask(T_FULL, nf, P, seed, offset).to(DEV)
    want = torch.relu(x.float() @ w.float().t() + b.float())
    ref = want * keep.float() / (1 - P)
    assert torch.allclose(y.float(), ref, atol=5e-2, rtol=3e-2)
    assert (y[~keep] == 0).all()
    clearly = keep & (want > 0.05)  # positive under bf16 rounding: zero only where dropped
    assert (y[clearly] != 0).all()
    nz = (y != 0).to(torch.uint8).view(T_FULL, nf // 8, 8)
    packed = (nz << torch.arange(8, device=DEV, dtype=torch.uint8)).sum(-1, dtype=torch.int32).to(torch.uint8)
    assert torch.equal(bits, packed)


@gpu
@pytest.mark.parametrize("K", KS)
def test_forward_aux_preactivation(k, width, K):
    nf, _ = _prefixes(width)
    x = _rand(T_FULL, K, seed=21)
    w = _rand(nf, K, scale=1 / math.sqrt(K), seed=22)
    b = _rand(nf, seed=23)

    def run(t, n):
        y, pre, _, _ = k.linear_fwd(x[:t], w[:n], b[:n], 2, 0.0, True)
        return y, pre

    y, pre = _check_prefixes(run, width)
    ref = x.float() @ w.float().t() + b.float()
    assert torch.allclose(pre.float(), ref, atol=3e-2, rtol=3e-2)
    assert torch.allclose(y.float(), torch.nn.functional.gelu(ref), atol=3e-2, rtol=3e-2)
