"""Row-wise and optimizer HIP kernels at their dispatch edges, against fp64
references and exact Philox dropout masks (one MI355X).

test_gpu_kernels.py runs these kernels on randn inputs at the benchmark's
shapes; here every dispatch branch runs (LayerNorm MAXV 1/2/4/8 and both row
groupings, Adam's three loops and tile variants, the vector and scalar bodies
of the cross-entropy, second trips of grid-stride loops), with non-zero means,
large and -inf logits, exact zeros, and the dropout masks checked bit for bit.

Tolerances are those of tests/helpers/rowwise_cases.py unless a test says
otherwise.  Every kernel comes from mipipe/_C.so: the tests fail if the
extension is missing."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers.rowwise_cases import (assert_close, assert_close_slack, assert_reduction, check_layernorm, ln_inputs,
                                   ln_reference, ln_saved_z_slack)
from test_gpu_kernels import _philox4x32_10

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float32, torch.bfloat16]
_M32 = 0xFFFFFFFF
_M64 = 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope="module")
def k():
    from mipipe._native_loader import kernels

    return kernels()


def _all_zero(t):
    return bool((t == 0).all().item())


# ------------------------------------------------------------------ 0. mask references
def _thr16(p):
    return int(float(np.float32(p)) * 2 ** 32) >> 16  # the kernels receive p as float


def _philox_blocks(nblk, seed, offset):
    """[nblk, 4] Philox words of subsequences 0..nblk-1 at (seed, offset)."""
    seed, offset = int(seed) & _M64, int(offset) & _M64
    blk = np.arange(nblk, dtype=np.uint64)
    words = _philox4x32_10(blk & np.uint64(_M32), blk >> np.uint64(32), offset & _M32, offset >> 32, seed & _M32,
                           seed >> 32)
    return np.stack([np.broadcast_to(w, blk.shape) for w in words], axis=1)


def keep8(n_elems, p, seed, offset):
    """dropout_keep8's layout (LayerNorm, embedding): flat element e draws Philox
    block e >> 3, word (e & 7) >> 1, 16-bit half e & 1 (low half for even e);
    kept iff that u16 >= thr16."""
    nblk = (n_elems + 7) // 8
    w = _philox_blocks(nblk, seed, offset)
    halves = np.stack([w & np.uint64(0xFFFF), (w >> np.uint64(16)) & np.uint64(0xFFFF)], axis=2)  # [blk, word, half]
    u16 = halves.reshape(nblk * 8)[:n_elems]
    return torch.from_numpy(u16 >= np.uint64(_thr16(p)))


def keep_rc(rows, cols, p, seed, offset):
    """drop_sub / drop_keep's layout (bias_act, GEMM epilogues): element (r, c)
    draws block (r >> 2) * (cols >> 1) + (c >> 1), word r & 3, half c & 1."""
    w = _philox_blocks(((rows + 3) // 4) * (cols // 2), seed, offset)
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    word = w[(r >> 2) * (cols >> 1) + (c >> 1), r & 3]
    u16 = (word >> (np.uint64(16) * (c & 1).astype(np.uint64))) & np.uint64(0xFFFF)
    return torch.from_numpy(u16 >= np.uint64(_thr16(p)))


# ------------------------------------------------------------------ 1. LayerNorm
# cols -> kernel: 8, 2048: wave-per-row; 2056, 3000: MAXV 2 (two-row blocks, a
# partly filled second vector slot; 1100 rows over 256 two-row blocks is three
# trips of the two-buffer loop); 4104, 8192: MAXV 4 (one-row blocks, one row at
# a time; 530 rows over 512 blocks is two trips); 8200, 16384: MAXV 8.
LN_SHAPES = [(8, 1), (8, 7), (2048, 9), (2056, 67), (3000, 1100), (4104, 67), (8192, 530), (8200, 5), (16384, 67)]


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cols,rows", LN_SHAPES)
def test_layernorm_dispatch_edges(k, cols, rows, dtype, residual):
    check_layernorm(cols, rows, dtype, residual)


@pytest.mark.parametrize("cols", [12, 2052, 16392])
def test_layernorm_rejects_width(k, cols):
    """Widths that are no multiple of 8, and 16392 (> 8 vectors per thread)."""
    x = torch.randn(3, cols, device=DEV)
    w, b = torch.ones(cols, device=DEV), torch.zeros(cols, device=DEV)
    with pytest.raises(RuntimeError):
        k.layernorm_fwd(x, None, w, b, 1e-5, 0.0, False)
    with pytest.raises(RuntimeError):
        k.layernorm_bwd(x, x, torch.zeros(3, device=DEV), torch.ones(3, device=DEV), w, 0.0, 0, 0)


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("cols", [1024, 4096, 8192])
def test_layernorm_offset_inputs(k, cols, residual):
    """x = 100 + randn: fp32 F.layer_norm (CPU) is within 1.7e-5 of fp64 here, a
    one-pass E[x^2] - mean^2 variance is off by 5e-3; the fp32 tolerance (1e-4)
    sits between the two."""
    check_layernorm(cols, 33, torch.float32, residual, offset=100.0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cols,p", [(1600, 0.25), (4096, 0.1), (8192, 0.25)])
def test_layernorm_dropout_exact_mask(k, cols, p, dtype):
    """Forward and backward regenerate the same documented keep8 mask: y and z
    against the fp64 reference of res + x * keep / (1 - p); dx exactly 0 where
    dropped and dz / (1 - p) where kept."""
    rows, eps = 37, 1e-5
    x, res, w, b, dy = ln_inputs(rows, cols, dtype, True)
    y, z, mean, rstd, seed, offset = k.layernorm_fwd(x, res, w, b, eps, p, True)
    keep = keep8(rows * cols, p, seed, offset).view(rows, cols).to(DEV)
    assert abs(keep.float().mean().item() - (1 - p)) < 0.01
    ref = ln_reference(x, res, w, b, eps, dy, keep, p)
    assert_close(z, ref["z"], dtype, "z")
    assert_close(y, ref["y"], dtype, "y")
    assert_close(mean, ref["z"].mean(-1), torch.float32, "mean")
    assert_close(rstd, (ref["z"].var(-1, unbiased=False) + eps).rsqrt(), torch.float32, "rstd")
    dz, dx, dg, db = k.layernorm_bwd(dy, z, mean, rstd, w, p, seed, offset)
    assert _all_zero(dx[~keep])
    if dtype == torch.float32:
        assert_close(dz, ref["dres"], dtype, "dz")
        assert_close(dx, ref["dx"], dtype, "dx")
        assert_reduction(dg, ref["dw"], "dgamma")
        assert_reduction(db, ref["db"], "dbeta")
    else:
        s_dz, s_dg = ln_saved_z_slack(ref["z"], w, dy, eps)
        assert_close_slack(dz, ref["dres"], s_dz, "dz")
        assert_close_slack(dx, ref["dx"], s_dz / (1 - p), "dx")
        assert_close_slack(dg, ref["dw"], s_dg, "dgamma")
        assert_close(db, ref["db"], dtype, "dbeta")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cols,rows", [(1600, 300), (4096, 300), (8192, 70)])
def test_layernorm_main_grad_accumulation(k, cols, rows, dtype):
    """acc_gamma / acc_beta (fp32 main_grad) receive prefill + the fp64 column
    sums; nothing is returned for them."""
    x, _, w, b, dy = ln_inputs(rows, cols, dtype, False)
    ref = ln_reference(x, None, w, b, 1e-5, dy)
    _, _, mean, rstd, _, _ = k.layernorm_fwd(x, None, w, b, 1e-5, 0.0, False)
    pre_g = 1 + 3 * torch.randn(cols, device=DEV)
    pre_b = -2 + 3 * torch.randn(cols, device=DEV)
    acc_g, acc_b = pre_g.clone(), pre_b.clone()
    dz, dx, dg, db = k.layernorm_bwd(dy, x, mean, rstd, w, 0.0, 0, 0, acc_g, acc_b)
    assert dg is None and db is None and dx is None
    assert_close(dz, ref["dx"], dtype, "dz")
    assert_reduction(acc_g, pre_g.double() + ref["dw"], "main_grad gamma")
    assert_reduction(acc_b, pre_b.double() + ref["db"], "main_grad beta")


def test_layernorm_block_kernels_at_narrow_widths():
    """MIPIPE_LN_ROWS=0 (read once per process): one fresh child runs the sweep
    on ln_fwd_kernel / ln_bwd_kernel<T, 1, 2> at 8, 256, 1600 and 2048 columns."""
    env = dict(os.environ, MIPIPE_LN_ROWS="0")
    worker = os.path.join(ROOT, "tests", "helpers", "ln_block_worker.py")
    r = subprocess.run([sys.executable, worker], env=env, timeout=240, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True)
    assert r.returncode == 0, r.stdout[-4000:]


# ------------------------------------------------------------------ 2. bias + activation + dropout
_ACTS = {0: None, 1: "relu", 2: "gelu"}


def _bias_act_ref(x, b, act, dy, keep=None, p=0.0):
    from mipipe.ops.activation import bias_act_reference

    xd = x.double().requires_grad_()
    bd = b.double().requires_grad_()
    y = bias_act_reference(xd, bd, _ACTS[act], 0.0, True)
    if keep is not None:
        y = y * keep.double() / (1.0 - p)
    y.backward(dy.double())
    return y.detach(), xd.grad


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("cols", [8, 520])
@pytest.mark.parametrize("rows", [1, 5, 96, 1023])
def test_bias_act_row_tails_and_exact_mask(k, rows, cols, act, dtype):
    """Row counts that leave the last 4-row tile partly filled; p = 0 against
    fp64, p > 0 with the exact keep_rc mask in forward and backward."""
    x = torch.randn(rows, cols, device=DEV).to(dtype)
    b = torch.randn(cols, device=DEV).to(dtype)
    dy = torch.randn(rows, cols, device=DEV).to(dtype)
    for p in (0.0, 0.25, 0.1):
        y, seed, offset = k.bias_act_fwd(x, b, act, p)
        keep = keep_rc(rows, cols, p, seed, offset).to(DEV) if p > 0 else None
        ref_y, ref_dx = _bias_act_ref(x, b, act, dy, keep, p)
        tag = f"bias_act {rows}x{cols} act={act} {dtype} p={p}"
        assert_close(y, ref_y, dtype, tag + " y")
        saved = x if act == 2 else y
        dx, dbias = k.bias_act_bwd(dy, saved, b, act, p, seed, offset, True)
        assert_close(dx, ref_dx, dtype, tag + " dx")
        if keep is not None:
            assert _all_zero(y[~keep]), tag
            assert _all_zero(dx[~keep]), tag
        # dbias is the column sum of the dx the kernel wrote (its own input)
        if dtype == torch.float32:
            assert_reduction(dbias, dx.double().sum(0), tag + " dbias")
        else:
            assert_close(dbias, dx.double().sum(0), dtype, tag + " dbias")


@pytest.mark.parametrize("dtype", DTYPES)
def test_bias_act_saved_gradient_backward(k, dtype):
    """Backward code 3: dx = dy * saved * keep / (1 - p), the mask regenerated
    from the forward's (seed, offset)."""
    rows, cols, p = 5, 520, 0.25
    x = torch.randn(rows, cols, device=DEV).to(dtype)
    _, seed, offset = k.bias_act_fwd(x, None, 2, p)
    keep = keep_rc(rows, cols, p, seed, offset).to(DEV)
    dy = torch.randn(rows, cols, device=DEV).to(dtype)
    sg = torch.randn(rows, cols, device=DEV).to(dtype)
    dx, dbias = k.bias_act_bwd(dy, sg, None, 3, p, seed, offset, False)
    assert dbias is None
    assert _all_zero(dx[~keep])
    assert_close(dx, dy.double() * sg.double() * keep.double() / (1 - p), dtype, "dx")


# ------------------------------------------------------------------ 3. cross-entropy
def _ce_check(k, logits, t, dtype, what, base=None):
    """loss / lse / weights of cross_entropy_mean_fwd and the gradient of
    ops.cross_entropy against fp64; ``logits`` is a leaf, or a view of the leaf
    ``base``.  Returns the gradient w.r.t. logits."""
    from mipipe.ops import cross_entropy

    N, V = logits.shape
    ld = logits.detach().double().requires_grad_()
    ref = F.cross_entropy(ld, t, ignore_index=-100, reduction="sum")
    valid = (t != -100)
    count = max(int(valid.sum().item()), 1)
    ref = ref / count
    ref.backward()
    loss, lse, weight = k.cross_entropy_mean_fwd(logits.detach(), t, -100)
    ref_lse = torch.logsumexp(ld.detach(), dim=1)
    err = (lse.double() - ref_lse).abs()
    bound = 1e-4 + 2.0 ** -22 * ref_lse.abs()
    assert torch.isfinite(lse).all(), what
    assert (err <= bound).all(), f"{what}: lse off by {err.max().item():.3e}"
    assert abs(loss.item() - ref.item()) < 1e-3 * max(1, abs(ref.item())), (what, loss.item(), ref.item())
    assert torch.allclose(weight.double(), valid.double() / count, rtol=1e-6, atol=0), what
    out = cross_entropy(logits, t)
    assert abs(out.item() - ref.item()) < 1e-3 * max(1, abs(ref.item())), (what, out.item(), ref.item())
    out.backward()
    g = base.grad[:, :V] if base is not None else logits.grad
    atol = 1e-5 if dtype == torch.float32 else 2e-4
    assert torch.isfinite(g).all(), what
    assert torch.allclose(g.double(), ld.grad, atol=atol, rtol=2e-2), \
        f"{what}: gradient off by {(g.double() - ld.grad).abs().max().item():.3e}"
    if base is not None and base.shape[1] > V:
        assert base.grad[:, V:].abs().max().item() == 0.0, what
    return g


def _ce_layout(values, layout):
    """values [N, V] (already in the kernel's dtype) as a contiguous leaf
    ("contig": rows of V elements -- the scalar path unless a row is a multiple
    of 16 bytes), as a [:, :V] view of a leaf padded to a multiple of 8
    ("padded": vector body plus scalar tail), or as a view whose base address
    is off the 16-byte grid ("offset": the scalar path at any V).  Returns (logits, base)."""
    N, V = values.shape
    if layout == "contig":
        return values.clone().requires_grad_(), None
    vp = (V + 7) // 8 * 8
    if layout == "padded":
        base = torch.zeros(N, vp, device=DEV, dtype=values.dtype)
        base[:, :V] = values
        base.requires_grad_()
        return base[:, :V], base
    buf = torch.zeros(N, vp + 8, device=DEV, dtype=values.dtype)
    buf[:, 1:V + 1] = values
    return buf[:, 1:V + 1].detach().requires_grad_(), None


def _targets(N, V, finite_cols=None):
    cols = torch.arange(V, device=DEV) if finite_cols is None else finite_cols
    t = cols[torch.randint(0, cols.numel(), (N,), device=DEV)]
    t[0] = cols[-1]  # the last column: in the scalar tail when V % 8 != 0
    if N > 3:
        t[3] = -100
    return t


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["contig", "padded"])
@pytest.mark.parametrize("V", [3, 8, 9, 255, 257])
def test_cross_entropy_small_vocab(k, V, layout, dtype):
    """V < 8 (no vector body), V < 256 (threads that see no value), one vector
    chunk plus a tail, and one value more than the block's threads."""
    N = 33
    values = (3 * torch.randn(N, V, device=DEV)).to(dtype)
    logits, base = _ce_layout(values, layout)
    _ce_check(k, logits, _targets(N, V), dtype, f"V={V} {layout} {dtype}", base)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_entropy_mean_second_trip(k, dtype):
    """N = 1500 > the mean kernel's 1024 threads, ignored targets on both sides
    of row 1024: loss, every row weight and the gradient."""
    N, V = 1500, 40
    values = (3 * torch.randn(N, V, device=DEV)).to(dtype)
    t = _targets(N, V)
    t[[7, 1000, 1023, 1024, 1025, 1400, 1499]] = -100
    logits, _ = _ce_layout(values, "contig")
    g = _ce_check(k, logits, t, dtype, f"N=1500 {dtype}")
    assert _all_zero(g[t == -100])


@pytest.mark.parametrize("layout", ["contig", "padded"])
@pytest.mark.parametrize("dtype,c", [(torch.float32, 0.0), (torch.float32, 80.0), (torch.float32, 1e4),
                                     (torch.float32, -1e4), (torch.bfloat16, 0.0), (torch.bfloat16, 80.0),
                                     (torch.bfloat16, 3e4)])
def test_cross_entropy_large_logits(k, dtype, c, layout):
    """Rows of c + randn: exp(80) overflows a softmax that does not subtract the
    row maximum first."""
    N, V = 16, 1003
    values = (c + torch.randn(N, V, device=DEV)).to(dtype)
    logits, base = _ce_layout(values, layout)
    _ce_check(k, logits, _targets(N, V), dtype, f"c={c} {layout} {dtype}", base)


def _neg_inf_case(case):
    if case == "v16_first8":
        V, dead = 16, torch.arange(16, device=DEV) < 8
    elif case == "v4096_random30":
        V = 4096
        dead = torch.rand(V, device=DEV) < 0.3
        dead[:8] = True  # thread 0's first 16-byte chunk entirely masked, finite ones after it
        dead[-1] = False
    else:  # the first 2048 columns: every thread's first chunks are all -inf
        V, dead = 4096, torch.arange(4096, device=DEV) < 2048
    return V, dead


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["contig", "offset"])
@pytest.mark.parametrize("case", ["v16_first8", "v4096_random30", "v4096_first2048"])
def test_cross_entropy_neg_inf_logits(k, case, layout, dtype):
    """Masked (-inf) logits: F.cross_entropy gives a finite loss and zero
    gradient on those columns.  A thread whose first chunk (vector path,
    "contig") or first value (scalar path, "offset") was -inf evaluated
    exp(-inf - (-inf)) = NaN into its running sum, and a finite value after it
    carried the NaN into the row's lse (both V = 4096 cases; at V = 16 no thread
    sees a second chunk and the block combine drops the sum of a thread whose
    maximum is still -inf, so that case only pins the result)."""
    N = 8
    V, dead = _neg_inf_case(case)
    values = (3 * torch.randn(N, V, device=DEV)).to(dtype)
    values[:, dead] = float("-inf")
    logits, _ = _ce_layout(values, layout)
    t = _targets(N, V, torch.nonzero(~dead).flatten())
    g = _ce_check(k, logits, t, dtype, f"{case} {layout} {dtype}")
    assert _all_zero(g[:, dead])


@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_entropy_split_decoder_neg_inf_head(k, dtype):
    """The split decoder's merge of a head slice whose logits are all -inf
    (lse -inf) with a finite tail: the full-row loss, no NaN."""
    N, V, E = 8, 64, 8
    head = torch.full((N, 32), float("-inf"), device=DEV, dtype=dtype)
    tail = (3 * torch.randn(N, 32, device=DEV)).to(dtype)
    t = torch.randint(32, V, (N,), device=DEV)
    nslot = 8 if dtype == torch.bfloat16 else 4  # 4 fp32 words of statistic slots
    msg = torch.zeros(N, E + nslot, device=DEV, dtype=dtype)
    k.vsplit_head_fwd(head, t, torch.zeros(N, E, device=DEV, dtype=dtype), msg)
    loss, lse, weight = k.vsplit_tail_fwd(tail, t, 32, -100, msg[:, E:])
    ref = F.cross_entropy(torch.cat([head, tail], 1).double(), t)
    assert torch.isfinite(lse).all()
    assert abs(loss.item() - ref.item()) < 1e-3 * max(1, abs(ref.item()))


@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_entropy_all_ignored(k, dtype):
    """count = max(#valid, 1): an all-ignored batch gives loss 0, weights 0 and
    a zero gradient, not NaN."""
    from mipipe.ops import cross_entropy

    N, V = 12, 40
    logits = (3 * torch.randn(N, V, device=DEV)).to(dtype).requires_grad_()
    t = torch.full((N,), -100, device=DEV)
    loss, lse, weight = k.cross_entropy_mean_fwd(logits.detach(), t, -100)
    assert loss.item() == 0.0 and weight.abs().max().item() == 0.0 and torch.isfinite(lse).all()
    out = cross_entropy(logits, t)
    assert out.item() == 0.0
    out.backward()
    assert logits.grad.abs().max().item() == 0.0  # also rules out NaN


# ------------------------------------------------------------------ 4. Adam and sumsq
def _adam_ref_step(st, g, step, lr, b1, b2, eps, wd, adamw, max_norm, sumsq):
    """fp64 re-statement of FlatAdam._step_eager on st = {p, m, v}."""
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    g = g.double()
    if sumsq is not None and max_norm > 0:
        g = g * min(1.0, max_norm / (math.sqrt(sumsq) + 1e-6))
    if wd:
        if adamw:
            st["p"] = st["p"] * (1 - lr * wd)
        else:
            g = g + wd * st["p"]
    st["m"] = b1 * st["m"] + (1 - b1) * g
    st["v"] = b2 * st["v"] + (1 - b2) * g * g
    st["p"] = st["p"] - (lr / bc1) * st["m"] / (st["v"].sqrt() / math.sqrt(bc2) + eps)


_ADAM_SIZES = {3: [(3,)], 4: [(4,)], 1027: [(17, 5), (33,), (909,)], 4 * 1024 * 2 + 5: [(1031, 7), (980,)]}
_ADAM_HYPER = [(adamw, wd, mgn) for adamw in (False, True) for wd in (0.0, 0.1) for mgn in (None, 1e6, 0.5)]


def _zero_block(n):
    return n // 3, max(n // 3 + 1, 2 * n // 3)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_flat_adam_hyper_sizes(k, variant, dtype):
    """Every Adam kernel variant, fp32 and bf16 parameters, three steps: Adam /
    AdamW with and without decay; no clipping, a clip that does not bind
    (coef = 1) and one that does; flat sizes 3 and 4 (n < 4: the grid-stride
    kernel with no vector at all), 1027, and two 4096-element tiles plus a
    tail; a block of exactly zero gradients, which must not move its
    parameters when there is no decay.  fp32 master against fp64 (atol 1e-5);
    the bf16 model copy equals master.to(bfloat16) bit for bit."""
    from mipipe.optim import FlatAdam

    lr, (b1, b2), eps = 1e-2, (0.9, 0.999), 1e-8
    k.adam_set_variant(variant)
    try:
        for n, shapes in _ADAM_SIZES.items():
            for adamw, wd, mgn in _ADAM_HYPER:
                tag = f"variant {variant} {dtype} n={n} adamw={adamw} wd={wd} max_grad_norm={mgn}"
                gen = torch.Generator(device=DEV).manual_seed(n)
                ps = [torch.randn(s, device=DEV, generator=gen).to(dtype).requires_grad_() for s in shapes]
                opt = FlatAdam(ps, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, adamw=adamw, max_grad_norm=mgn)
                (grp,) = opt.groups
                assert grp.numel == n
                init = grp.master.clone()
                st = {"p": init.double(), "m": torch.zeros(n, device=DEV, dtype=torch.float64),
                      "v": torch.zeros(n, device=DEV, dtype=torch.float64)}
                z0, z1 = _zero_block(n)
                for step in range(1, 4):
                    g = torch.randn(n, device=DEV, generator=gen)
                    g[z0:z1] = 0.0
                    opt.zero_grad()
                    grp.main_grad.copy_(g)
                    opt.step()
                    sumsq = g.double().pow(2).sum().item() if mgn is not None else None
                    _adam_ref_step(st, g, step, lr, b1, b2, eps, wd, adamw, mgn or 0.0, sumsq)
                err = (grp.master.double() - st["p"]).abs().max().item()
                assert torch.isfinite(grp.master).all() and err <= 1e-5, f"{tag}: master off by {err:.3e}"
                if wd == 0.0:
                    assert torch.equal(grp.master[z0:z1], init[z0:z1]), f"{tag}: zero gradients moved parameters"
                if dtype == torch.bfloat16:
                    assert grp.model.dtype == torch.bfloat16 and grp.model is not grp.master
                    assert torch.equal(grp.model, grp.master.to(torch.bfloat16)), f"{tag}: bf16 model copy"
                    off = 0
                    for p in ps:  # the parameters are views of the model copy
                        assert torch.equal(p.detach().reshape(-1), grp.model[off:off + p.numel()]), tag
                        off += p.numel()
    finally:
        k.adam_set_variant(2)


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("mgn", [None, 0.5])
def test_flat_adamw_matches_torch_adamw(k, variant, mgn):
    """fp32 adamw=True against torch.optim.AdamW (clip_grad_norm_ first)."""
    from mipipe.optim import FlatAdam

    k.adam_set_variant(variant)
    try:
        ps = [torch.randn(s, device=DEV, requires_grad=True) for s in _ADAM_SIZES[1027]]
        qs = [p.detach().clone().requires_grad_() for p in ps]
        opt = FlatAdam(ps, lr=1e-2, weight_decay=0.1, adamw=True, max_grad_norm=mgn)
        ref = torch.optim.AdamW(qs, lr=1e-2, weight_decay=0.1)
        for _ in range(3):
            grads = [torch.randn_like(q) for q in qs]
            opt.zero_grad()
            for p, g in zip(ps, grads):
                p.grad = g.clone()
            opt.step()
            for q, g in zip(qs, grads):
                q.grad = g.clone()
            if mgn is not None:
                torch.nn.utils.clip_grad_norm_(qs, mgn)
            ref.step()
    finally:
        k.adam_set_variant(2)
    for p, q in zip(ps, qs):
        assert torch.allclose(p, q, atol=1e-5)


@pytest.fixture(scope="module")
def adam_large():
    """One case of n = 2 * 4,194,304 + 1203 elements, built once and never
    modified: in the grid-stride kernel (4096 blocks of 256 threads, two
    vectors per trip) the U = 2 loop, the single-vector loop (300 vectors) and
    the scalar tail (3 elements) all run.  The fp64 result is added by the
    first test that has the clip's fp32 sum of squares."""
    n = 8_389_811
    gen = torch.Generator(device=DEV).manual_seed(11)
    p = torch.randn(n, device=DEV, generator=gen)
    g = torch.randn(n, device=DEV, generator=gen)
    g[1000:3000] = 0.0
    # moments of a plausible earlier step (|m| = 0.3 sqrt(v)): the update stays below lr
    h = torch.randn(n, device=DEV, generator=gen)
    m, v = 0.3 * h, h * h
    hyper = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=0.01, adamw=False, max_norm=2000.0, step=2)
    return dict(p=p, g=g, m=m, v=v, hyper=hyper)


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_adam_step_large_flat_buffer(k, adam_large, variant):
    """k.adam_step on 8,389,811 elements with a bf16 model copy, one step
    against fp64 (atol 1e-6: the step moves a parameter by about lr, and with
    |p| < 8 the fp32 rounding of the parameter itself is below 2.4e-7)."""
    c = adam_large
    h = c["hyper"]
    sq = k.sumsq(c["g"])
    if "ref" not in c:
        st = {"p": c["p"].double(), "m": c["m"].double(), "v": c["v"].double()}
        _adam_ref_step(st, c["g"], h["step"], h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], h["adamw"], h["max_norm"],
                       float(sq.item()))  # the fp32 sum the kernel itself reads
        c["ref"] = st["p"]
        assert c["p"].abs().max().item() < 8
    master, m, v = c["p"].clone(), c["m"].clone(), c["v"].clone()
    model = torch.zeros(master.numel(), device=DEV, dtype=torch.bfloat16)
    k.adam_set_variant(variant)
    try:
        k.adam_step(master, model, c["g"], m, v, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"],
                    1 - h["b1"] ** h["step"], 1 - h["b2"] ** h["step"], sq, h["max_norm"], h["adamw"])
    finally:
        k.adam_set_variant(2)
    err = (master.double() - c["ref"]).abs()
    assert torch.isfinite(master).all()
    assert err.max().item() <= 1e-6, f"variant {variant}: off by {err.max().item():.3e} at {err.argmax().item()}"
    assert torch.equal(model, master.to(torch.bfloat16))
    assert not torch.equal(master, c["p"])


@pytest.mark.parametrize("n", [1, 3, 1023, 1_048_576 * 4 + 7])
def test_sumsq_sizes(k, n):
    """n < 4 (scalar tail only), n < 1024 (one partly filled block), and five
    trips of the 1024-block grid-stride loop plus a tail; values near 1e3."""
    g = 1e3 * torch.randn(n, device=DEV)
    ref = g.double().pow(2).sum()
    out = k.sumsq(g)
    assert out.shape == (1,) and abs(out.item() - ref.item()) <= 1e-4 * ref.item(), (out.item(), ref.item())


# ------------------------------------------------------------------ 5. embedding and column_sum
def _tokens(V, B, S):
    tok = torch.randint(0, V, (B, S), device=DEV)
    tok[0, :3] = 7  # repeats: atomic accumulation
    tok[1, 0] = 7
    tok[0, 3] = 0
    tok[1, 1] = V - 1
    return tok


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", [0.0, 0.25])
@pytest.mark.parametrize("E", [2056, 8192])
def test_embedding_wide_rows(k, E, p, dtype):
    """E / 8 > 256: the 256-thread blocks loop more than once over a row (E =
    8192 fills the backward's LDS row); p = 0 against F.embedding in fp64,
    p = 0.25 with the exact keep8 mask in the forward and the table gradient."""
    V, B, S = 64, 2, 8
    scale = math.sqrt(E)
    w = torch.randn(V, E, device=DEV).to(dtype)
    tok = _tokens(V, B, S)
    y, seed, offset = k.embedding_fwd(tok, w, None, scale, p)
    keep = keep8(B * S * E, p, seed, offset).view(B, S, E).to(DEV) if p > 0 else torch.ones(B, S, E, dtype=torch.bool,
                                                                                             device=DEV)
    mask = keep.double() / (1 - p)
    assert_close(y, F.embedding(tok, w.double()) * scale * mask, dtype, "embedding")
    assert _all_zero(y[~keep])
    dout = torch.randn(B, S, E, device=DEV).to(dtype)
    dw = torch.zeros(V, E, device=DEV)
    k.embedding_bwd(tok, dout, dw, scale, p, seed, offset)
    ref = torch.zeros(V, E, device=DEV, dtype=torch.float64)
    ref.index_add_(0, tok.reshape(-1), (dout.double() * mask * scale).reshape(-1, E))
    assert_reduction(dw, ref, "table gradient")
    untouched = torch.ones(V, dtype=torch.bool, device=DEV)
    untouched[tok.reshape(-1)] = False
    assert _all_zero(dw[untouched])


def test_embedding_rejects_rows_over_8192(k):
    tok = _tokens(64, 2, 8)
    with pytest.raises(RuntimeError):
        k.embedding_bwd(tok, torch.zeros(2, 8, 8200, device=DEV), torch.zeros(64, 8200, device=DEV), 1.0, 0.0, 0, 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,cols", [(1, 8), (31, 264), (300, 7)])
def test_column_sum_small_shapes(k, rows, cols, dtype):
    """One row, fewer rows than a part's 32 row lanes, and the scalar path
    (cols % 8 != 0); a fresh output and accumulate=True into fp32."""
    x = torch.randn(rows, cols, device=DEV).to(dtype)
    ref = x.double().sum(0)
    out = k.column_sum(x)
    assert out.dtype == dtype and out.shape == (cols,)
    if dtype == torch.float32:
        assert_reduction(out, ref, "column_sum")
    else:
        assert_close(out, ref, dtype, "column_sum")
    pre = 5 + torch.randn(cols, device=DEV)
    acc = pre.clone()
    ret = k.column_sum(x, acc, True)
    assert ret.data_ptr() == acc.data_ptr()
    assert_reduction(acc, pre.double() + ref, "column_sum accumulate")
