"""Shared case code of tests/test_gpu_rowwise_edges.py and its LayerNorm worker
(tests/helpers/ln_block_worker.py): tolerance rules and the LayerNorm
forward/backward comparison against an fp64 reference.

Tolerances (fixed by reasoning about the number formats, never by what a
kernel returns):

* fp32 kernel against fp64: ``|err| <= 1e-4 + 1e-4 * |ref|`` (the project's fp32
  tolerance, ``_tol`` of test_gpu_kernels.py);
* bf16 output, reference computed from the bf16-rounded inputs:
  ``|err| <= 2**-8 * |ref| + 1e-4`` -- one full bf16 ulp (twice the half ulp a
  single round-to-nearest store can cost) plus the fp32 term;
* fp32 column reductions (dgamma / dbeta / main_grad / table gradients):
  ``max|err| / max|ref| < 1e-4``.
"""
import torch
import torch.nn.functional as F

DEV = "cuda"
FP32_TOL = (1e-4, 1e-4)  # (atol, rtol), test_gpu_kernels._tol(torch.float32)
BF16_REL = 2.0 ** -8
BF16_ABS = 1e-4
RED_REL = 1e-4


def excess(out, ref, dtype):
    """max over elements of |out - ref| - allowed(ref); <= 0 passes.  ``ref`` is fp64."""
    out = out.double()
    err = (out - ref).abs()
    if dtype == torch.bfloat16:
        allowed = BF16_REL * ref.abs() + BF16_ABS
    else:
        allowed = FP32_TOL[0] + FP32_TOL[1] * ref.abs()
    if err.numel() == 0:
        return 0.0
    bad = ~torch.isfinite(out)
    if bad.any():
        return float("inf")
    return (err - allowed).max().item()


def assert_close(out, ref, dtype, what):
    e = excess(out, ref, dtype)
    worst = (out.double() - ref).abs().max().item() if ref.numel() else 0.0
    assert e <= 0, f"{what}: max|err| {worst:.3e}, {e:.3e} over the {dtype} bound"


def red_err(out, ref):
    """max|err| / max|ref| of a reduction; ``ref`` fp64."""
    out = out.double()
    if not torch.isfinite(out).all():
        return float("inf")
    return ((out - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def assert_reduction(out, ref, what):
    r = red_err(out, ref)
    assert r < RED_REL, f"{what}: max|err| / max|ref| = {r:.3e} (bound {RED_REL:g})"


def ln_reference(x, res, w, b, eps, dy, keep=None, p=0.0):
    """fp64 LayerNorm(res + x * keep / (1 - p)) of the tensors as given (already
    rounded to the kernel's dtype), and its gradients for the output gradient dy."""
    xd = x.detach().double().requires_grad_()
    rd = res.detach().double().requires_grad_() if res is not None else None
    wd = w.detach().double().requires_grad_()
    bd = b.detach().double().requires_grad_()
    h = xd
    if keep is not None:
        h = h * keep.to(h.device).double() / (1.0 - p)
    z = h + rd if rd is not None else h
    y = F.layer_norm(z, (x.shape[-1],), wd, bd, eps)
    y.backward(dy.detach().double())
    return {"y": y.detach(), "z": z.detach(), "dx": xd.grad, "dres": rd.grad if rd is not None else None,
            "dw": wd.grad, "db": bd.grad}


def ln_saved_z_slack(z, w, dy, eps):
    """Extra error allowed in the bf16 backward WITH a residual, as (dz, dgamma).

    The forward normalises the fp32 sum z = res + x but saves it for the
    backward rounded to bf16 (half the bytes of an fp32 copy), so the backward
    sees xhat off by up to |dxh| = 2**-8 |z| rstd (half a bf16 ulp of z is at
    most 2**-8 |z|).  Propagated to first order through
        dz = rstd (gy - mean(gy) - xhat mean(gy xhat)),  dgamma = sum_rows dy xhat
    with gy = dy gamma, in fp64 from the inputs (never from a kernel's output):
        |d dz|     <= rstd (|dxh| |mean(gy xhat)| + |xhat| mean(|gy| |dxh|))
        |d dgamma| <= sum_rows |dy| |dxh|
    dbeta = sum_rows dy does not read z.  For scale: PyTorch's own bf16
    layer_norm of the rounded sum, measured on the CPU on these inputs, misses
    the unwidened bf16 bound by up to 1.4e-2 (dz) and 2.2 (dgamma, 1100 rows x
    3000), where this slack is at most 1.1e-2 and 3.1."""
    z, gy, dy = z.double(), dy.double() * w.double(), dy.double()
    mean = z.mean(-1, keepdim=True)
    rstd = (z.var(-1, unbiased=False, keepdim=True) + eps).rsqrt()
    xh = (z - mean) * rstd
    dxh = BF16_REL * z.abs() * rstd
    dz = rstd * (dxh * (gy * xh).mean(-1, keepdim=True).abs() + xh.abs() * (gy.abs() * dxh).mean(-1, keepdim=True))
    dg = (dy.abs() * dxh).sum(0)
    return dz, dg


def assert_close_slack(out, ref, slack, what):
    out = out.double()
    assert torch.isfinite(out).all(), f"{what}: non-finite values"
    over = ((out - ref).abs() - (BF16_REL * ref.abs() + BF16_ABS + slack)).max().item()
    assert over <= 0, f"{what}: {over:.3e} over the bf16 bound plus the saved-z slack"


def ln_inputs(rows, cols, dtype, residual, offset=0.0, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed + 7919 * cols + rows)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)  # noqa: E731
    x = (offset + rn(rows, cols)).to(dtype)
    res = rn(rows, cols).to(dtype) if residual else None
    w = (1 + 0.1 * rn(cols)).to(dtype)
    b = (0.1 * rn(cols)).to(dtype)
    dy = rn(rows, cols).to(dtype)
    return x, res, w, b, dy


def check_layernorm(cols, rows, dtype, residual, offset=0.0):
    """add_dropout_layer_norm (p = 0) forward and backward against fp64; raises
    AssertionError naming the first tensor outside its bound."""
    from mipipe.ops import add_dropout_layer_norm

    x, res, w, b, dy = ln_inputs(rows, cols, dtype, residual, offset)
    ref = ln_reference(x, res, w, b, 1e-5, dy)
    xs = x.clone().requires_grad_()
    rs = res.clone().requires_grad_() if residual else None
    ws, bs = w.clone().requires_grad_(), b.clone().requires_grad_()
    y = add_dropout_layer_norm(xs, rs, ws, bs, 1e-5, 0.0, True)
    tag = f"layernorm {rows}x{cols} {dtype} residual={residual}"
    assert_close(y, ref["y"], dtype, tag + " y")
    y.backward(dy)
    if dtype == torch.float32:
        assert_close(xs.grad, ref["dx"], dtype, tag + " dx")
        if residual:
            assert_close(rs.grad, ref["dres"], dtype, tag + " dresidual")
        assert_reduction(ws.grad, ref["dw"], tag + " dgamma")
        assert_reduction(bs.grad, ref["db"], tag + " dbeta")
    elif not residual:  # the backward reads x itself: no rounded copy in between
        assert_close(xs.grad, ref["dx"], dtype, tag + " dx")
        assert_close(ws.grad, ref["dw"], dtype, tag + " dgamma")
        assert_close(bs.grad, ref["db"], dtype, tag + " dbeta")
    else:
        s_dz, s_dg = ln_saved_z_slack(ref["z"], w, dy, 1e-5)
        assert_close_slack(xs.grad, ref["dx"], s_dz, tag + " dx")
        assert_close_slack(rs.grad, ref["dres"], s_dz, tag + " dresidual")
        assert_close_slack(ws.grad, ref["dw"], s_dg, tag + " dgamma")
        assert_close(bs.grad, ref["db"], dtype, tag + " dbeta")
