"""K-segmented weight-gradient GEMMs: the segment bookkeeping of the 256-row
kernel's K loop (one MI355X).

The loop tracks (segment, local k) of the tile it stages next incrementally
and switches operand pointers at a segment boundary; each wave group stages a
different tile ahead.  These tests pin the results at the shapes where that
can go wrong -- a boundary at every tile, boundaries odd against the 2-buffer
and 3-slot rotations, kMaxSegs segments, a single K-tile, split-K blocks that
start in the middle of a segment -- bit for bit against the same GEMM over the
concatenated operands, which has no boundary to cross."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def k():
    from mipipe._native_loader import kernels

    return kernels()


@functools.lru_cache(maxsize=None)
def _operands(N, Kin, T, nseg):
    """dY_i [T, N], x_i [T, Kin], x_i^T, their concatenations along T and the fp32
    product -- made once per shape and shared (never written to)."""
    g = torch.Generator(device=DEV).manual_seed(1000 * N + 10 * Kin + T + nseg)
    dys = [torch.randn(T, N, device=DEV, generator=g).to(torch.bfloat16) for _ in range(nseg)]
    xs = [torch.randn(T, Kin, device=DEV, generator=g).to(torch.bfloat16) for _ in range(nseg)]
    xts = [x.t().contiguous() for x in xs]
    dy_cat, x_cat = torch.cat(dys, 0), torch.cat(xs, 0)
    expect = dy_cat.float().t() @ x_cat.float()
    return dys, xs, xts, dy_cat, x_cat, x_cat.t().contiguous(), expect


# (N, Kin, T, nseg)
SEGMENT_CASES = [
    (256, 256, 64, 5),    # one tile; every K-tile is its own segment: both look-aheads cross a boundary every tile
    (520, 264, 64, 16),   # edge tiles, kMaxSegs segments
    (264, 136, 128, 3),   # two tiles per segment
    (256, 512, 192, 4),   # three tiles per segment: odd against the 2-buffer and the 3-slot rotation
    (256, 256, 64, 1),    # nk = 1: no look-ahead at all
]


@pytest.mark.parametrize("width", [128, 256])
@pytest.mark.parametrize("N,Kin,T,nseg", SEGMENT_CASES)
def test_segments_equal_concatenated(k, N, Kin, T, nseg, width):
    """main_grad of the segmented GEMM == main_grad of the unsegmented GEMM over the
    concatenated operands, bit for bit: same kernel, same block width, same
    split-K setting, same accumulation order -- only the operand addresses
    differ.  Both entries, storing and accumulating.

    The unsegmented run of the [T, N] / [T, Kin] layout is linear_wgrad on the
    concatenation; the x^T entry has no unsegmented twin, so its reference is
    the same entry with ONE segment spanning the whole K (no boundary inside).
    That one-segment form is checked for the plain entry as well."""
    dys, xs, xts, dy_cat, x_cat, xt_cat, _ = _operands(N, Kin, T, nseg)
    init = torch.randn(N, Kin, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    k.gemm_set_width(width)
    try:
        for accumulate in (False, True):
            seg = init.clone()
            k.linear_wgrad_segments(dys, xs, seg, accumulate)
            one = init.clone()
            k.linear_wgrad_segments([dy_cat], [x_cat], one, accumulate)
            assert torch.equal(seg, one), ("segments vs one segment", accumulate, (seg - one).abs().max().item())
            cat = init.clone()
            k.linear_wgrad(dy_cat, x_cat, cat, accumulate)
            assert torch.equal(seg, cat), ("segments vs linear_wgrad", accumulate, (seg - cat).abs().max().item())

            seg_t = init.clone()
            k.linear_wgrad_xt_segments(dys, xts, seg_t, accumulate)
            one_t = init.clone()
            k.linear_wgrad_xt_segments([dy_cat], [xt_cat], one_t, accumulate)
            assert torch.equal(seg_t, one_t), ("x^T segments vs one segment", accumulate,
                                               (seg_t - one_t).abs().max().item())
    finally:
        k.gemm_set_width(0)


# (256, 256, 192, 8) is 24 K-tiles of 3 per segment.  The host takes split-K only
# from K = 8192 and 16 K-tiles per block, so that shape runs unsplit whatever
# gemm_set_splitk says; (256, 256, 704, 12) -- 132 K-tiles of 11 per segment --
# is the smallest odd-tiles-per-segment shape that does split 5 and 7 ways:
# blocks then start at tiles 26, 52, 79, 105 and 18, 37, 56, 75, 94, 113, none
# a multiple of 11.
@pytest.mark.parametrize("splits", [5, 7])
@pytest.mark.parametrize("N,Kin,T,nseg", [(256, 256, 192, 8), (256, 256, 704, 12)])
def test_split_k_starts_mid_segment(k, N, Kin, T, nseg, splits):
    """A split-K block that starts inside a segment (the one division left in
    the kernel): against fp32 within the 1e-3 relative bound of
    test_wgrad_split_k, both entries, storing and accumulating."""
    dys, xs, xts, _, _, _, expect = _operands(N, Kin, T, nseg)
    scale = expect.abs().max()
    k.gemm_set_splitk(splits)
    try:
        for accumulate in (False, True):
            for xt in (False, True):
                main = torch.randn(N, Kin, device=DEV)
                base = main.clone() if accumulate else torch.zeros_like(main)
                if xt:
                    k.linear_wgrad_xt_segments(dys, xts, main, accumulate)
                else:
                    k.linear_wgrad_segments(dys, xs, main, accumulate)
                err = ((main - base - expect).abs().max() / scale).item()
                assert err < 1e-3, (splits, accumulate, xt, err)
    finally:
        k.gemm_set_splitk(1)


def test_rowsum_fold(k):
    """The A-side bias fold (16 tile columns: the smallest fold shape of
    test_wgrad_segments_fused_bias, at T = 64 so every tile crosses a segment),
    to that test's tolerances."""
    N, Kin, T, nseg = 520, 4096, 64, 3
    dys, xs, _, _, _, _, expect = _operands(N, Kin, T, nseg)
    main = torch.zeros(N, Kin, device=DEV)
    bias = torch.full((N,), 0.5, device=DEV)
    assert k.linear_wgrad_segments(dys, xs, main, True, bias)
    assert ((main - expect).abs().max() / expect.abs().max()).item() < 1e-3
    ref = 0.5 + sum(d.float().sum(0) for d in dys)
    assert torch.allclose(bias, ref, atol=1e-2, rtol=1e-4), (bias - ref).abs().max()


@pytest.mark.parametrize("N,Kin", [(600, 256), (264, 2048)])
def test_colsum_fold(k, N, Kin):
    """The B-side bias fold of the x^T entry, to the same tolerances: one tile
    row -> 128-column slices, several K-rows per lane (the smallest fold shape
    of test_wgrad_xt_segments, at T = 64), and 8 tile rows -> 16-column slices,
    one K-row per lane (the form the wide layers take)."""
    T, nseg = 64, 3
    dys, _, xts, _, _, _, expect = _operands(N, Kin, T, nseg)
    for accumulate in (False, True):
        main = torch.randn(N, Kin, device=DEV)
        base = main.clone() if accumulate else torch.zeros_like(main)
        bias = torch.full((N,), 0.5, device=DEV)
        assert k.linear_wgrad_xt_segments(dys, xts, main, accumulate, bias)
        assert ((main - base - expect).abs().max() / expect.abs().max()).item() < 1e-3
        ref = 0.5 + sum(d.float().sum(0) for d in dys)
        assert torch.allclose(bias, ref, atol=1e-2, rtol=1e-4), (bias - ref).abs().max()
