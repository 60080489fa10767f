"""The both-I-contiguous weight-gradient GEMM (dW = dY^T . X with dY and X read
as they lie in memory: ``gemm256_kernel<false, false, ...>``) through the
binding the deferred flush uses for that layout, ``linear_wgrad_segments``,
against ``dY.float().T @ X.float()``.

Every call here is K-segmented (``seg_k > 0``, one segment included), which
``use_big`` sends to the 256-row tile kernel whatever the shape, so the small
shapes below all run the kernel's main loop: one K-tile, the tile counts at
which the three-slot B rotation wraps and the two-buffer A parity flips (2, 3,
4, 7), both block widths, edge tiles, split-K, two segments, both epilogues
and the folded bias gradient.  Tolerances are those of the weight-gradient
tests in test_gpu_kernels.py (max error over max magnitude < 1e-3; bias
atol 1e-2, rtol 1e-4)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def k():
    from mipipe._native_loader import kernels

    return kernels()


def _inputs(seed, n_out, k_in, t, nseg):
    g = torch.Generator(device=DEV).manual_seed(seed)
    dys = [torch.randn(t, n_out, device=DEV, generator=g).to(torch.bfloat16) for _ in range(nseg)]
    xs = [torch.randn(t, k_in, device=DEV, generator=g).to(torch.bfloat16) for _ in range(nseg)]
    expect = sum(d.float().t() @ x.float() for d, x in zip(dys, xs))
    return dys, xs, expect


def _check_both_epilogues(k, dys, xs, expect, tag, bias=False):
    """First write (the store epilogue) over garbage, then accumulation into a
    non-zero main_grad; with ``bias`` the row-sum fold must be taken."""
    n_out, k_in = expect.shape
    for accumulate in (False, True):
        main = torch.randn(n_out, k_in, device=DEV)
        base = main.clone() if accumulate else torch.zeros_like(main)
        bg = torch.full((n_out,), 0.5, device=DEV) if bias else None
        fused = k.linear_wgrad_segments(dys, xs, main, accumulate, bg)
        err = ((main - base - expect).abs().max() / expect.abs().max()).item()
        assert err < 1e-3, (tag, accumulate, err)
        if bias:
            assert fused, tag  # >= 16 tile columns and no split-K: the fold is part of the GEMM
            ref = 0.5 + sum(d.float().sum(0) for d in dys)
            assert torch.allclose(bg, ref, atol=1e-2, rtol=1e-4), (tag, accumulate, (bg - ref).abs().max().item())
        else:
            assert not fused, tag


@pytest.mark.parametrize("ktiles", [1, 2, 3, 4, 7])
def test_wgrad_ii_k_tiles(k, ktiles):
    """One 256 x 256 tile, 1-7 K-tiles of 64 tokens: no rotation, then the B
    slots wrapping (3, 4), both A parities, and an odd tail."""
    assert k.gemm_supported(256, 256, 64 * ktiles)
    dys, xs, expect = _inputs(100 + ktiles, 256, 256, 64 * ktiles, 1)
    _check_both_epilogues(k, dys, xs, expect, ktiles)


@pytest.mark.parametrize("width", [256, 128])
def test_wgrad_ii_edge_tiles_both_widths(k, width):
    """A partial tile in N_out and in K_in (256 + 64 each, so 2 x 2 or 2 x 3
    blocks), two segments of three K-tiles, at both block widths."""
    k.gemm_set_width(width)
    try:
        dys, xs, expect = _inputs(200 + width, 320, 320, 192, 2)
        _check_both_epilogues(k, dys, xs, expect, width)
    finally:
        k.gemm_set_width(0)


@pytest.mark.parametrize("width,k_in", [(256, 4096), (128, 2048)])
def test_wgrad_ii_bias_fold(k, width, k_in):
    """The bias gradient (row sums of the A tiles) folded into the GEMM: 16
    tile columns at each width, an edge tile row, two segments."""
    k.gemm_set_width(width)
    try:
        dys, xs, expect = _inputs(300 + width, 320, k_in, 128, 2)
        _check_both_epilogues(k, dys, xs, expect, (width, k_in), bias=True)
    finally:
        k.gemm_set_width(0)


def test_wgrad_ii_split_k_and_determinism(k):
    """K = 2 x 4096 tokens on a one-tile grid: the split-K rule cuts the 128
    K-tiles over several blocks (all but the first start mid-way, half of them
    in the second segment) and a reduction adds their fp32 partials in a fixed order -- so
    the same call twice gives identical bits (as the kernel before this loop
    did: the partials are never added atomically)."""
    dys, xs, expect = _inputs(400, 256, 256, 4096, 2)
    _check_both_epilogues(k, dys, xs, expect, "split-k")
    outs = []
    for _ in range(2):
        main = torch.full((256, 256), 0.25, device=DEV)
        k.linear_wgrad_segments(dys, xs, main, True)
        outs.append(main)
    assert torch.equal(outs[0], outs[1])


def test_wgrad_ii_deterministic_plain(k):
    """No split-K (three K-tiles per segment): the same call twice, identical bits."""
    dys, xs, _ = _inputs(500, 320, 320, 192, 2)
    outs = []
    for _ in range(2):
        main = torch.empty(320, 320, device=DEV)
        k.linear_wgrad_segments(dys, xs, main, False)
        outs.append(main)
    assert torch.equal(outs[0], outs[1])
