"""The QK-norm HIP kernels (csrc/kernels/qknorm.hip) on the GPU: forward, dx and
the two weight gradients against fp64, the V heads, in place against out of
place, an all-zero row, main_grad accumulation, the binding's refusals, the
eager path of an unsupported head dim, a checkpoint recompute and the
``qwen3_tiny`` model.  The kernels come from mipipe/_C.so: the tests fail if the
extension is missing.

The reference is fp64 math on the tensors as given (already rounded to the
kernel's dtype), written out here; the bounds are the project's own
(helpers/rowwise_cases.py): the kernels compute in fp32 and round once at the
store, and the backward reads x itself, so no extra term is needed."""
import copy
import warnings

import pytest
import torch

from helpers.rowwise_cases import assert_close, assert_reduction
from test_gpu_llama_kernels import _assert_model_close, _data, _gpu_step, _loss_fn

from mipipe import Pipe, checkpoint, ops
from mipipe.models import CONFIGS, build_lm_blocks
from mipipe.models.transformer import AttentionCore
from mipipe.optim import FlatAdam
from mipipe.parallel import PipelineEngine

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
EPS = 1e-6
B, S, POS0 = 2, 37, 5
HEADS = [(4, 4, 4), (6, 2, 2), (4, 1, 1)]


@pytest.fixture(scope="module")
def k():
    from mipipe._native_loader import kernels

    return kernels()


def qknorm_fp64(x, wq, wk, eps, cos, sin, n_q, n_k, pos0, dout):
    """fp64 ``{y, dx, dwq, dwk}`` of the tensors as given, every step written out (no autograd, no mipipe op)."""
    x, wq, wk, dout = x.double(), wq.double(), wk.double(), dout.double()
    Bb, Ss, heads, Dd = x.shape
    half = Dd // 2
    n = n_q + n_k
    w = torch.cat((wq.expand(n_q, Dd), wk.expand(n_k, Dd)), 0)
    qk = x[:, :, :n]
    rstd = 1.0 / torch.sqrt((qk * qk).sum(-1, keepdim=True) / Dd + eps)
    xhat = qk * rstd
    nrm = xhat * w
    g = dout[:, :, :n]
    if cos is not None:
        c = cos[pos0:pos0 + Ss].double().view(1, Ss, 1, half)
        s = sin[pos0:pos0 + Ss].double().view(1, Ss, 1, half)
        a, b = nrm[..., :half], nrm[..., half:]
        y_qk = torch.cat((a * c - b * s, b * c + a * s), -1)
        ga, gb = g[..., :half], g[..., half:]
        g = torch.cat((ga * c + gb * s, gb * c - ga * s), -1)
    else:
        y_qk = nrm
    gy = g * w
    cm = (gy * xhat).sum(-1, keepdim=True) / Dd
    dx_qk = rstd * (gy - xhat * cm)
    dw = (g * xhat).sum((0, 1))
    return {"y": torch.cat((y_qk, x[:, :, n:]), 2), "dx": torch.cat((dx_qk, dout[:, :, n:]), 2),
            "dwq": dw[:n_q].sum(0), "dwk": dw[n_q:].sum(0)}


def _inputs(b, s, heads, D, dtype, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed + 131 * D + heads)
    rn = lambda *sh: torch.randn(*sh, device=DEV, generator=g)  # noqa: E731
    x = rn(b, s, heads, D).to(dtype)
    dout = rn(b, s, heads, D).to(dtype)
    wq = (1 + 0.3 * rn(D)).to(dtype)
    wk = (1 + 0.3 * rn(D)).to(dtype)
    return x, wq, wk, dout


def _run(x, wq, wk, cos, sin, n_q, n_k, pos0, dout):
    xs, qs, ks = (t.clone().requires_grad_() for t in (x, wq, wk))
    y = ops.qk_norm_rope_heads(xs, qs, ks, EPS, cos, sin, n_q, n_k, pos0)
    assert y.data_ptr() != xs.data_ptr() and torch.equal(xs.detach(), x)
    y.backward(dout)
    return y.detach(), xs.grad, qs.grad, ks.grad


def _check_case(b, s, n_q, n_k, n_v, D, pos0, tables, dtype):
    x, wq, wk, dout = _inputs(b, s, n_q + n_k + n_v, D, dtype)
    cos, sin = ops.rope_tables(pos0 + s + 3, D, device=DEV) if tables else (None, None)
    ref = qknorm_fp64(x, wq, wk, EPS, cos, sin, n_q, n_k, pos0, dout)
    y, dx, dwq, dwk = _run(x, wq, wk, cos, sin, n_q, n_k, pos0, dout)
    tag = f"qknorm {b}x{s} heads {n_q}+{n_k}+{n_v} D{D} pos0={pos0} tables={tables} {dtype}"
    assert_close(y, ref["y"], dtype, tag + " y")
    assert_close(dx, ref["dx"], dtype, tag + " dx")
    for out, name in ((dwq, "dwq"), (dwk, "dwk")):
        assert out.dtype == dtype
        if dtype == torch.float32:
            assert_reduction(out, ref[name], f"{tag} {name}")
        else:
            assert_close(out, ref[name], dtype, f"{tag} {name}")
    # V: bit-identical, forward and backward
    n = n_q + n_k
    assert torch.equal(y[:, :, n:], x[:, :, n:]) and torch.equal(dx[:, :, n:], dout[:, :, n:])
    return x, wq, wk, cos, sin, y


# ------------------------------------------------------------------ 1. against fp64
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tables", [True, False])
@pytest.mark.parametrize("n_q,n_k,n_v", HEADS)
@pytest.mark.parametrize("D", [64, 128, 256])
def test_qknorm_against_fp64(k, D, n_q, n_k, n_v, tables, dtype):
    """B S (n_q + n_k) = 74 * {8, 8, 5} head rows of 4, 8 or 16 lanes: no multiple of the rows of a wave or of a
    block, with V vectors in the same waves."""
    _check_case(B, S, n_q, n_k, n_v, D, POS0, tables, dtype)


@pytest.mark.parametrize("D", [16, 32])
def test_qknorm_small_head_dims(k, D):
    """One and two lanes per row."""
    _check_case(B, S, 6, 2, 2, D, POS0, True, torch.bfloat16)
    _check_case(B, S, 4, 4, 4, D, 0, False, torch.float32)


@pytest.mark.parametrize("dtype", DTYPES)
def test_qknorm_grid_stride_runs_more_than_once(k, dtype):
    """8 * 512 tokens of 36 + 4 norm heads at D = 64: 163,840 head rows = 655,360 row items plus the V vectors,
    past the forward's 2048 * 256 and the backward's 1024 * 256 threads."""
    _check_case(8, 512, 36, 4, 4, 64, 3, True, dtype)


# ------------------------------------------------------------------ 2. in place
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tables", [True, False])
@pytest.mark.parametrize("D,n_q,n_k,n_v", [(64, 6, 2, 2), (128, 4, 4, 4)])
def test_qknorm_in_place_gives_the_same_bits(k, D, n_q, n_k, n_v, tables, dtype):
    x, wq, wk, _ = _inputs(B, S, n_q + n_k + n_v, D, dtype, seed=1)
    cos, sin = ops.rope_tables(POS0 + S, D, device=DEV) if tables else (None, None)
    out = ops.qk_norm_rope_heads(x, wq, wk, EPS, cos, sin, n_q, n_k, POS0)
    assert out.data_ptr() != x.data_ptr()
    # in the argument's own storage: the same bits, the V bytes as they were
    buf = x.clone()
    same = ops.qk_norm_rope_heads(buf, wq, wk, EPS, cos, sin, n_q, n_k, POS0, inplace=True)
    assert same.data_ptr() == buf.data_ptr() and torch.equal(same, out)
    assert torch.equal(buf[:, :, n_q + n_k:], x[:, :, n_q + n_k:])
    # the binding itself: out = x, no rstd without save_rstd
    buf2 = x.clone()
    y2, rstd = k.qk_norm_rope_fwd(buf2, wq, wk, EPS, cos, sin, buf2, n_q, n_k, POS0, False)
    assert rstd is None and y2.data_ptr() == buf2.data_ptr() and torch.equal(y2, out)
    y3, rstd = k.qk_norm_rope_fwd(x, wq, wk, EPS, cos, sin, None, n_q, n_k, POS0, True)
    assert torch.equal(y3, out) and rstd.shape == (B * S, n_q + n_k) and rstd.dtype == torch.float32
    ref_rstd = torch.rsqrt(x[:, :, :n_q + n_k].double().pow(2).mean(-1) + EPS).view(B * S, n_q + n_k)
    assert_close(rstd, ref_rstd, torch.float32, "rstd")
    # under autograd the op is out of place whatever inplace says: the backward needs x
    leaf = x.clone().requires_grad_()
    mid = leaf * 1
    out4 = ops.qk_norm_rope_heads(mid, wq, wk, EPS, cos, sin, n_q, n_k, POS0, inplace=True)
    assert out4.data_ptr() != mid.data_ptr() and torch.equal(out4, out) and torch.equal(mid.detach(), x)


def test_no_grad_forward_saves_nothing(k):
    x, wq, wk, _ = _inputs(B, S, 8, 64, torch.bfloat16, seed=2)
    wq.requires_grad_()
    cos, sin = ops.rope_tables(S, 64, device=DEV)
    torch.cuda.synchronize()
    with torch.no_grad():
        buf = x.clone()
        base = torch.cuda.memory_allocated()
        y = ops.qk_norm_rope_heads(buf, wq, wk, EPS, cos, sin, 4, 2, inplace=True)
        assert torch.cuda.memory_allocated() == base  # in place, no rstd
        assert y.grad_fn is None and not y.requires_grad


# ------------------------------------------------------------------ 3. a zero row
@pytest.mark.parametrize("dtype", DTYPES)
def test_qknorm_zero_rows(k, dtype):
    D, n_q, n_k, n_v = 64, 4, 2, 2
    x, wq, wk, dout = _inputs(B, S, n_q + n_k + n_v, D, dtype, seed=3)
    x[0, 3, 1] = 0   # a Q head row
    x[1, 30, 5] = 0  # a K head row
    cos, sin = ops.rope_tables(S, D, device=DEV)
    ref = qknorm_fp64(x, wq, wk, EPS, cos, sin, n_q, n_k, 0, dout)
    y, dx, dwq, dwk = _run(x, wq, wk, cos, sin, n_q, n_k, 0, dout)
    assert (y[0, 3, 1] == 0).all() and (y[1, 30, 5] == 0).all()
    for t in (y, dx, dwq, dwk):
        assert torch.isfinite(t).all()
    # dx of a zero row is rstd gy with rstd = eps^-1/2 = 1000: large, finite, and within the bound
    assert dx[0, 3, 1].abs().max().item() > 100
    assert_close(y, ref["y"], dtype, "zero rows y")
    assert_close(dx, ref["dx"], dtype, "zero rows dx")


# ------------------------------------------------------------------ 4. main_grad
@pytest.mark.parametrize("dtype", DTYPES)
def test_qknorm_main_grad_accumulation(k, dtype):
    """w.main_grad (fp32) on both weights: the first backward after _mg_fresh = True overwrites the stale 7.0s,
    the second accumulates; w.grad stays None; the same inputs give the same bits."""
    D, n_q, n_k, n_v = 128, 6, 2, 2
    x, wq, wk, dout = _inputs(B, S, n_q + n_k + n_v, D, dtype, seed=4)
    dout2 = torch.randn(dout.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5)).to(dtype)
    cos, sin = ops.rope_tables(POS0 + S, D, device=DEV)
    ref1 = qknorm_fp64(x, wq, wk, EPS, cos, sin, n_q, n_k, POS0, dout)
    ref2 = qknorm_fp64(x, wq, wk, EPS, cos, sin, n_q, n_k, POS0, dout2)

    def fresh():
        qs, ks = wq.clone().requires_grad_(), wk.clone().requires_grad_()
        for w in (qs, ks):
            w.main_grad = torch.full((D,), 7.0, device=DEV)
            w._mg_fresh = True
        return qs, ks

    def two_steps():
        qs, ks = fresh()
        xs = x.clone().requires_grad_()
        ops.qk_norm_rope_heads(xs, qs, ks, EPS, cos, sin, n_q, n_k, POS0).backward(dout)
        first = (qs.main_grad.clone(), ks.main_grad.clone())
        ops.qk_norm_rope_heads(x.clone().requires_grad_(), qs, ks, EPS, cos, sin, n_q, n_k, POS0).backward(dout2)
        assert qs.grad is None and ks.grad is None
        return first, (qs.main_grad.clone(), ks.main_grad.clone()), xs.grad

    first, second, dx = two_steps()
    assert_reduction(first[0], ref1["dwq"], "wq.main_grad after the first backward")
    assert_reduction(first[1], ref1["dwk"], "wk.main_grad after the first backward")
    assert_reduction(second[0], ref1["dwq"] + ref2["dwq"], "wq.main_grad after the second backward")
    assert_reduction(second[1], ref1["dwk"] + ref2["dwk"], "wk.main_grad after the second backward")
    first_b, second_b, dx_b = two_steps()
    assert torch.equal(dx, dx_b)
    for a, b in zip(first + second, first_b + second_b):
        assert torch.equal(a, b)
    # one weight with a main_grad, the other without: one accumulates, the other is returned in its dtype
    qs, _ = fresh()
    ks = wk.clone().requires_grad_()
    ops.qk_norm_rope_heads(x.clone().requires_grad_(), qs, ks, EPS, cos, sin, n_q, n_k, POS0).backward(dout)
    assert qs.grad is None and torch.equal(qs.main_grad, first[0])
    assert ks.grad is not None and ks.grad.dtype == dtype
    if dtype == torch.float32:
        assert_reduction(ks.grad, ref1["dwk"], "dwk beside an accumulated dwq")
    else:
        assert_close(ks.grad, ref1["dwk"], dtype, "dwk beside an accumulated dwq")
    # the binding itself: prefilled targets are added to, nothing is returned for them
    _, rstd = k.qk_norm_rope_fwd(x, wq, wk, EPS, cos, sin, None, n_q, n_k, POS0, True)
    pre_q, pre_k = 1 + 3 * torch.randn(D, device=DEV), 1 + 3 * torch.randn(D, device=DEV)
    acc_q, acc_k = pre_q.clone(), pre_k.clone()
    _, gq, gk = k.qk_norm_rope_bwd(dout, x, rstd, wq, wk, cos, sin, n_q, n_k, POS0, acc_q, acc_k)
    assert gq is None and gk is None
    assert_reduction(acc_q, pre_q.double() + ref1["dwq"], "acc_q")
    assert_reduction(acc_k, pre_k.double() + ref1["dwk"], "acc_k")


# ------------------------------------------------------------------ 5. refusals and the eager path
def test_qknorm_binding_refuses(k):
    D = 64
    x, wq, wk, dout = _inputs(1, 8, 8, D, torch.float32, seed=6)
    cos, sin = ops.rope_tables(8, D, device=DEV)
    assert k.qk_norm_rope_fwd(x, wq, wk, EPS, cos, sin, None, 4, 2)[0].shape == x.shape
    with pytest.raises(RuntimeError, match="contiguous"):
        k.qk_norm_rope_fwd(x.transpose(1, 2), wq, wk, EPS, cos, sin, None, 4, 2)
    with pytest.raises(RuntimeError, match="n_q \\+ n_k"):
        k.qk_norm_rope_fwd(x, wq, wk, EPS, cos, sin, None, 6, 3)
    with pytest.raises(RuntimeError, match="wq and wk"):
        k.qk_norm_rope_fwd(x, wq[:32].contiguous(), wk, EPS, cos, sin, None, 4, 2)
    with pytest.raises(RuntimeError, match="wq and wk"):
        k.qk_norm_rope_fwd(x, wq, torch.ones(128, device=DEV), EPS, cos, sin, None, 4, 2)
    with pytest.raises(RuntimeError, match="cos / sin"):  # tables end at position 8
        k.qk_norm_rope_fwd(x, wq, wk, EPS, cos, sin, None, 4, 2, 1)
    with pytest.raises(RuntimeError, match="cos / sin"):  # bf16 tables
        k.qk_norm_rope_fwd(x, wq, wk, EPS, cos.bfloat16(), sin.bfloat16(), None, 4, 2)
    with pytest.raises(RuntimeError, match="both cos and sin"):
        k.qk_norm_rope_fwd(x, wq, wk, EPS, cos, None, None, 4, 2)
    with pytest.raises(RuntimeError, match="same dtype"):
        k.qk_norm_rope_fwd(x, wq.bfloat16(), wk.bfloat16(), EPS, cos, sin, None, 4, 2)
    for bad in (24, 48, 96, 512):
        xb = torch.randn(1, 8, 8, bad, device=DEV)
        cb, sb = ops.rope_tables(8, bad, device=DEV)
        assert not k.qk_norm_rope_supported(bad)
        with pytest.raises(RuntimeError, match="head dim"):
            k.qk_norm_rope_fwd(xb, torch.ones(bad, device=DEV), torch.ones(bad, device=DEV), EPS, cb, sb, None, 4, 2)
    assert all(k.qk_norm_rope_supported(d) for d in (16, 32, 64, 128, 256))
    # the backward checks the same, and its own tensors
    _, rstd = k.qk_norm_rope_fwd(x, wq, wk, EPS, cos, sin, None, 4, 2)
    with pytest.raises(RuntimeError, match="rstd"):
        k.qk_norm_rope_bwd(dout, x, rstd[:, :5].contiguous(), wq, wk, cos, sin, 4, 2)
    with pytest.raises(RuntimeError, match="dout"):
        k.qk_norm_rope_bwd(dout[:, :4].contiguous(), x, rstd, wq, wk, cos, sin, 4, 2)
    with pytest.raises(RuntimeError, match="accumulation target"):
        k.qk_norm_rope_bwd(dout, x, rstd, wq, wk, cos, sin, 4, 2, 0, torch.zeros(D, device=DEV).bfloat16(), None)
    with pytest.raises(RuntimeError, match="cos / sin"):
        k.qk_norm_rope_bwd(dout, x, rstd, wq, wk, cos, sin, 4, 2, 1)
    # no tokens: shapes only
    y, r = k.qk_norm_rope_fwd(x[:, :0].contiguous(), wq, wk, EPS, cos, sin, None, 4, 2)
    assert y.shape == (1, 0, 8, D) and r.shape == (0, 6)


def test_unsupported_head_dim_runs_the_eager_reference_and_warns_once(k):
    Q = __import__("sys").modules["mipipe.ops.qknorm"]
    D, n_q, n_k, n_v = 48, 4, 2, 2
    x, wq, wk, dout = _inputs(B, 9, n_q + n_k + n_v, D, torch.float32, seed=7)
    cos, sin = ops.rope_tables(9, D, device=DEV)
    Q._noted.discard((tuple(x.shape), x.dtype))
    with pytest.warns(UserWarning, match="head dim 48 is not native"):
        y, dx, dwq, dwk = _run(x, wq, wk, cos, sin, n_q, n_k, 0, dout)
    ref = qknorm_fp64(x, wq, wk, EPS, cos, sin, n_q, n_k, 0, dout)
    assert_close(y, ref["y"], torch.float32, "eager y")
    assert_close(dx, ref["dx"], torch.float32, "eager dx")
    assert_reduction(dwq, ref["dwq"], "eager dwq")
    assert_reduction(dwk, ref["dwk"], "eager dwk")
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # once per shape
        y2 = ops.qk_norm_rope_heads(x, wq, wk, EPS, cos, sin, n_q, n_k)
        y3 = ops.qk_norm_rope_projection(x.view(B, 9, -1), wq, wk, EPS, cos, sin, n_q, n_kv_heads=n_k)
    assert torch.equal(y2, y) and torch.equal(y3, y)


# ------------------------------------------------------------------ 6. checkpoint recompute
@pytest.mark.parametrize("hkv", [2, 4])
def test_qk_norm_checkpoint_recompute_bit_exact(k, hkv):
    """The checkpoint's first forward runs under no_grad: the norm works in place in the projection's output and
    saves nothing; the recompute is out of place.  Output and gradients match the uncheckpointed run bit for bit."""
    Sq, E = 64, 256
    torch.manual_seed(0)
    core = AttentionCore(E, 4, 0.0, norm_first=True, causal=True, layer_norm_eps=1e-5, norm="rms", bias=False,
                         rope=True, n_kv_heads=hkv, qk_norm=True).to(DEV, torch.bfloat16).train()
    with torch.no_grad():
        core.q_norm_weight.add_(0.2 * torch.randn(64, device=DEV))
        core.k_norm_weight.add_(0.2 * torch.randn(64, device=DEV))
    g = torch.Generator(device=DEV).manual_seed(8)
    base = torch.randn(B, Sq, E, device=DEV, generator=g).to(torch.bfloat16)
    do = torch.randn(B, Sq, E, device=DEV, generator=g).to(torch.bfloat16)

    def run(ckpt):
        core.zero_grad()
        x = base.clone().requires_grad_()
        o = checkpoint(core, x) if ckpt else core(x)
        o.backward(do)
        torch.cuda.synchronize()
        return [o.detach(), x.grad] + [p.grad.clone() for p in core.parameters()]

    with_ckpt, without = run(True), run(False)
    assert len(with_ckpt) == 2 + 4  # in_proj, the block's norm, the two QK-norm weights
    for a, b in zip(with_ckpt, without):
        assert torch.equal(a, b)
    assert core.q_norm_weight.grad.abs().max().item() > 0 and core.k_norm_weight.grad.abs().max().item() > 0
    # the norm is really there
    core.eval()
    with torch.no_grad():
        o_on = core(base)
        core.qk_norm = False
        assert not torch.equal(core(base), o_on)


# ------------------------------------------------------------------ 7. the model
@pytest.fixture(scope="module")
def qwen3_reference():
    """qwen3_tiny's blocks (bf16-rounded weights, the norm weights moved off 1) and, on the CPU eager path in
    fp32, the loss and gradients of one step."""
    cfg = CONFIGS["qwen3_tiny"]
    torch.manual_seed(0)
    blocks = build_lm_blocks(cfg, dtype=torch.bfloat16)
    cores = [b.core for b in blocks if hasattr(b, "core")]
    assert len(cores) == 2 and all(c.qk_norm for c in cores)
    with torch.no_grad():
        for c in cores:
            c.q_norm_weight.add_(0.2 * torch.randn(c.head_dim))
            c.k_norm_weight.add_(0.2 * torch.randn(c.head_dim))
    ref = torch.nn.Sequential(*copy.deepcopy(blocks)).float().train()
    x, t = _data(cfg, 8)
    loss = _loss_fn(cfg)(ref(x), t)
    loss.backward()
    return blocks, float(loss.detach()), {n: p.grad for n, p in ref.named_parameters()}


def test_qwen3_tiny_bf16_matches_cpu_fp32(k, qwen3_reference):
    """test_llama_tiny_bf16_matches_cpu_fp32's comparison and bound (loss 2e-3 relative, each gradient 2e-2 of
    its max) on the QK-norm model."""
    cfg = CONFIGS["qwen3_tiny"]
    blocks, ref_loss, ref_grads = qwen3_reference
    model = torch.nn.Sequential(*copy.deepcopy(blocks)).to(DEV).train()
    x, t = _data(cfg, 8)
    loss, grads = _gpu_step(model, cfg, x, t)
    assert any(n.endswith("q_norm_weight") for n in grads) and any(n.endswith("k_norm_weight") for n in grads)
    _assert_model_close(loss, grads, ref_loss, ref_grads)


@pytest.mark.parametrize("ckpt", ["never", "except_last", "always"])
def test_qwen3_tiny_pipe_two_partitions(k, qwen3_reference, ckpt):
    cfg = CONFIGS["qwen3_tiny"]
    blocks, ref_loss, ref_grads = qwen3_reference
    blocks = copy.deepcopy(blocks)
    model = torch.nn.Sequential(*blocks).to(DEV).train()
    opt = FlatAdam(model.parameters(), lr=1e-3)
    pipe = Pipe(model, chunks=4, checkpoint=ckpt, balance=[3, len(blocks) - 3], copy_same_device=True)
    x, t = _data(cfg, 8)
    try:
        assert len(pipe.partitions) == 2
        opt.zero_grad()
        loss = _loss_fn(cfg)(pipe(x.to(DEV)).local_value(), t.to(DEV))
        loss.backward()
        opt.fold_grads()
        torch.cuda.synchronize()
    finally:
        pipe.close()
    _assert_model_close(float(loss.detach()), {n: p.main_grad for n, p in model.named_parameters()}, ref_loss,
                        ref_grads)


def test_qwen3_tiny_engine_step_flat_adam(k, qwen3_reference):
    cfg = CONFIGS["qwen3_tiny"]
    blocks, ref_loss, ref_grads = qwen3_reference
    model = torch.nn.Sequential(*copy.deepcopy(blocks)).to(DEV).train()
    opt = FlatAdam(model.parameters(), lr=1e-3)
    m, mb = 4, 2
    eng = PipelineEngine(model, chunks=m, checkpoint="except_last", act_shape=(mb, cfg.seq_len),
                         act_dtype=torch.bfloat16, loss_fn=_loss_fn(cfg), device=torch.device(DEV, 0))
    x, t = _data(cfg, m * mb)
    before = [p.detach().clone() for p in model.parameters()]
    opt.zero_grad()
    st = eng.step([c.to(DEV) for c in x.split(mb)], [c.to(DEV) for c in t.split(mb)])
    opt.fold_grads()
    torch.cuda.synchronize()
    _assert_model_close(float(st.loss), {n: p.main_grad.clone() for n, p in model.named_parameters()}, ref_loss,
                        ref_grads)
    opt.step()
    torch.cuda.synchronize()
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
    assert all(torch.isfinite(p.detach().float()).all() for p in model.parameters())
