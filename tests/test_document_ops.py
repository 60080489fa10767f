"""Document-masked attention (packed sequences) on the CPU: the bounds helpers of
``utils.data``, the eager ops with ``doc_bounds`` against an fp64 attention
whose mask is built here from ``arange`` comparisons, the errors, ``None`` as
the old code path, a causal model under ``ops.use_documents``, two gloo
ranks through ``PipelineEngine.step(..., doc_bounds=...)`` and the training
example's ``--doc-eos``.  The HIP kernels
behind the same keyword are tested in test_gpu_document_kernels.py.

The CPU attention path (``ops.attention_reference``) computes in fp32 whatever
it is given, so the comparisons with the fp64 oracle are at the project's fp32
bound (``helpers.rowwise_cases.FP32_TOL``)."""
import math

import pytest
import torch

from helpers import documents_engine
from helpers.rowwise_cases import FP32_TOL

from mipipe import checkpoint, ops
from mipipe.models import build_lm_blocks
from mipipe.models.transformer import AttentionCore
from mipipe.utils.data import document_bounds, document_bounds_from_lengths, mask_boundary_targets

B, S, D = 2, 24, 16
LENGTHS = [[1, 7, 1, 9, 6], [10, 14]]  # one-token documents, another packing per row


# ------------------------------------------------------------------ 1. the bounds helpers
def _tokens(rows, eos=0):
    """Rows of document lengths -> tokens: every document ends in an EOS except one cut by the row's end."""
    out = []
    for lengths, cut in rows:
        row = []
        for n in lengths:
            row += [5] * (n - 1) + [eos]
        if cut:
            row[-1] = 5
        out.append(row)
    return torch.tensor(out)


def test_document_bounds_edges_and_lengths():
    # EOS at position 0 (a one-token first document), adjacent EOS tokens, EOS at S - 1
    t = _tokens([([1, 3, 1, 1, 2], False), ([8], False)])
    assert t[0].tolist() == [0, 5, 5, 0, 0, 0, 5, 0] and t[1, -1] == 0
    b = document_bounds(t, 0)
    assert b.dtype == torch.int32 and b.shape == (2, 2, 8) and b.is_contiguous()
    assert b[0, 0].tolist() == [0, 1, 1, 1, 4, 5, 6, 6]
    assert b[0, 1].tolist() == [1, 4, 4, 4, 5, 6, 8, 8]
    assert torch.equal(b, document_bounds_from_lengths([[1, 3, 1, 1, 2], [8]], 8))
    ops.check_doc_bounds(b)
    # no EOS: one document; a last document cut by the row
    t = _tokens([([8], True), ([3, 5], True)])
    b = document_bounds(t, 0)
    assert torch.equal(b, document_bounds_from_lengths([[8], [3, 5]], 8))
    ops.check_doc_bounds(b)
    assert torch.equal(document_bounds_from_lengths([3, 5], 8), b[1:])  # a flat list is one row
    with pytest.raises(ValueError):
        document_bounds_from_lengths([3, 4], 8)


def test_document_bounds_of_a_split_batch_is_the_split_of_the_bounds():
    g = torch.Generator().manual_seed(0)
    tok = torch.randint(0, 6, (6, 40), generator=g)
    whole = document_bounds(tok, 3)
    ops.check_doc_bounds(whole)
    assert int(whole[:, 0].max()) > 0
    for part, ref in zip(tok.split(2), whole.split(2)):
        assert torch.equal(document_bounds(part, 3), ref)


def test_check_doc_bounds_rejects_broken_contracts():
    good = document_bounds_from_lengths(LENGTHS, S)
    ops.check_doc_bounds(good)
    bad = good.clone()
    bad[0, 0, 3] = 0  # start: 0 1 1 0 ... is not monotone
    with pytest.raises(ValueError, match="non-decreasing|constant"):
        ops.check_doc_bounds(bad)
    bad = good.clone()
    bad[1, 0, 2] = 5  # start[i] > i
    with pytest.raises(ValueError):
        ops.check_doc_bounds(bad)
    bad = good.clone()
    bad[1, 1, -1] = S + 1
    with pytest.raises(ValueError):
        ops.check_doc_bounds(bad)
    with pytest.raises(ValueError, match="int32"):
        ops.check_doc_bounds(good.long())


def test_mask_boundary_targets():
    tok = torch.tensor([[5, 0, 7, 7, 0, 0, 2, 9]])
    tgt = torch.tensor([[0, 7, 7, 0, 0, 2, 9, 4]])
    out = mask_boundary_targets(tgt, tok, 0, -100)
    assert out.tolist() == [[0, -100, 7, 0, -100, -100, 9, 4]] and tgt[0, 1] == 7  # not in place
    assert mask_boundary_targets(tgt.reshape(-1), tok, 0).tolist() == out.reshape(-1).tolist()
    logits = torch.randn(8, 10)
    ref = torch.nn.functional.cross_entropy(logits[out[0] != -100], out[0][out[0] != -100])
    assert torch.allclose(ops.cross_entropy(logits, out.reshape(-1)), ref, atol=1e-6)


# ------------------------------------------------------------------ 2. the eager ops against fp64
def document_attention_fp64(q, k, v, bounds, window=None, softcap=None):
    """``[B, H, S, D]`` fp64 attention where query i sees the keys start[b, i] <= j <= i (and j > i - window)."""
    n = q.shape[-2]
    i = torch.arange(n)[None, :, None]
    j = torch.arange(n)[None, None, :]
    keep = (j <= i) & (j >= bounds[:, 0].long()[:, :, None])
    if window is not None:
        keep &= j > i - window
    s = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(q.shape[-1])
    if softcap is not None:
        s = softcap * torch.tanh(s / softcap)
    s = s.masked_fill(~keep[:, None], float("-inf"))
    return torch.matmul(torch.softmax(s, dim=-1), v)


def _close(out, ref, what):
    allowed = FP32_TOL[0] + FP32_TOL[1] * ref.abs()
    over = ((out.double() - ref).abs() - allowed).max().item()
    assert over <= 0, f"{what}: {over:.3e} over the fp32 bound"


def _inputs(h, hkv, seed=0):
    g = torch.Generator().manual_seed(seed + 10 * h + hkv)
    qkv = torch.randn(B, S, h + 2 * hkv, D, generator=g)
    do = torch.randn(B, S, h, D, generator=g)
    return qkv, do


def _oracle(qkv, do, h, hkv, bounds, window=None, softcap=None):
    """(o [B, S, H, D], dqkv) of the fp64 attention on repeated K/V heads (autograd sums each group)."""
    x = qkv.double().requires_grad_()
    q, k, v = (t.transpose(1, 2) for t in (x[:, :, :h], x[:, :, h:h + hkv], x[:, :, h + hkv:]))
    rep = h // hkv
    o = document_attention_fp64(q, k.repeat_interleave(rep, 1), v.repeat_interleave(rep, 1), bounds, window, softcap)
    o.backward(do.double().transpose(1, 2))
    return o.detach().transpose(1, 2), x.grad


@pytest.mark.parametrize("window,softcap", [(None, None), (5, None), (None, 50.0), (5, 50.0)])
@pytest.mark.parametrize("h,hkv", [(4, 4), (6, 2), (4, 1)])
def test_document_ops_against_fp64(h, hkv, window, softcap):
    qkv, do = _inputs(h, hkv)
    bounds = document_bounds_from_lengths(LENGTHS, S)
    ref_o, ref_d = _oracle(qkv, do, h, hkv, bounds, window, softcap)
    tag = f"H{h}/{hkv} W{window} cap{softcap}"
    kw = dict(causal=True, window=window, softcap=softcap, doc_bounds=bounds)

    x = qkv.clone().requires_grad_()
    o = ops.attention_gqa_packed(x, hkv, **kw)
    o.backward(do)
    _close(o, ref_o, tag + " attention_gqa_packed o")
    _close(x.grad, ref_d, tag + " attention_gqa_packed dqkv")

    leaves = [t.transpose(1, 2).clone().requires_grad_() for t in (qkv[:, :, :h], qkv[:, :, h:h + hkv],
                                                                    qkv[:, :, h + hkv:])]
    o = ops.attention(*leaves, **kw)
    o.backward(do.transpose(1, 2))
    _close(o.transpose(1, 2), ref_o, tag + " attention o")
    for t, lo, hi, name in ((leaves[0], 0, h, "dq"), (leaves[1], h, h + hkv, "dk"), (leaves[2], h + hkv, None, "dv")):
        _close(t.grad.transpose(1, 2), ref_d[:, :, lo:hi], f"{tag} attention {name}")

    if hkv == h:
        x5 = qkv.view(B, S, 3, h, D).clone().requires_grad_()
        o = ops.attention_packed(x5, **kw)
        o.backward(do)
        _close(o, ref_o, tag + " attention_packed o")
        _close(x5.grad.view_as(ref_d), ref_d, tag + " attention_packed dqkv")
        rl = [t.transpose(1, 2).clone().requires_grad_() for t in x5.detach().unbind(2)]
        o = ops.attention_reference(*rl, True, 0.0, window=window, softcap=softcap, doc_bounds=bounds)
        o.backward(do.transpose(1, 2))
        _close(o.transpose(1, 2), ref_o, tag + " attention_reference o")
        for t, which in zip(rl, range(3)):
            _close(t.grad.transpose(1, 2), ref_d.view(B, S, 3, h, D)[:, :, which], f"{tag} attention_reference d{which}")

    # each document's rows equal causal attention run on that document alone
    full = ops.attention_gqa_packed(qkv, hkv, **kw)
    for b, lengths in enumerate(LENGTHS):
        at = 0
        for n in lengths:
            alone = ops.attention_gqa_packed(qkv[b:b + 1, at:at + n], hkv, causal=True, window=window, softcap=softcap)
            _close(full[b:b + 1, at:at + n], alone.double(), f"{tag} document [{at}, {at + n}) of row {b} alone")
            at += n


# ------------------------------------------------------------------ 3. errors, and None
def test_bad_bounds_raise():
    qkv, _ = _inputs(4, 4)
    q5 = qkv.view(B, S, 3, 4, D)
    q, k, v = (t.transpose(1, 2) for t in q5.unbind(2))
    good = document_bounds_from_lengths(LENGTHS, S)
    for bounds, causal in ((good, False), (good[:, :, :-1], True), (good[:, 0], True), (good[:1], True),
                           (good.long(), True), (good.float(), True)):
        for call in (lambda **kw: ops.attention_packed(q5, **kw),
                     lambda **kw: ops.attention_gqa_packed(qkv, 4, **kw),
                     lambda **kw: ops.attention_gqa_packed(qkv[:, :, :8], 2, **kw),
                     lambda **kw: ops.attention(q, k, v, **kw),
                     lambda **kw: ops.attention_reference(q, k, v, kw["causal"], 0.0, doc_bounds=kw["doc_bounds"])):
            with pytest.raises(ValueError, match="doc_bounds"):
                call(causal=causal, doc_bounds=bounds)


@pytest.mark.parametrize("causal", [False, True])
def test_no_bounds_is_the_call_without_the_keyword(causal):
    qkv, _ = _inputs(4, 2, seed=3)
    q5 = _inputs(4, 4, seed=3)[0].view(B, S, 3, 4, D)
    q, k, v = (t.transpose(1, 2) for t in q5.unbind(2))
    assert torch.equal(ops.attention_gqa_packed(qkv, 2, causal=causal, doc_bounds=None),
                       ops.attention_gqa_packed(qkv, 2, causal=causal))
    assert torch.equal(ops.attention_packed(q5, causal=causal, doc_bounds=None), ops.attention_packed(q5, causal=causal))
    assert torch.equal(ops.attention(q, k, v, causal=causal, doc_bounds=None), ops.attention(q, k, v, causal=causal))
    assert torch.equal(ops.attention_reference(q, k, v, causal, 0.0, doc_bounds=None),
                       ops.attention_reference(q, k, v, causal, 0.0))


def test_use_documents_is_a_thread_local_context():
    import threading

    good = document_bounds_from_lengths(LENGTHS, S)
    assert ops.current_documents() is None
    seen = []
    with ops.use_documents(good):
        assert ops.current_documents() is good
        with ops.use_documents(None):
            assert ops.current_documents() is None
        assert ops.current_documents() is good
        t = threading.Thread(target=lambda: seen.append(ops.current_documents()))
        t.start()
        t.join()
    assert ops.current_documents() is None and seen == [None]
    with pytest.raises(RuntimeError, match="boom"):
        with ops.use_documents(good):
            raise RuntimeError("boom")
    assert ops.current_documents() is None


# ------------------------------------------------------------------ 4. a model under use_documents
def _model_run(model, x, bounds):
    model.zero_grad()
    leaf = x.clone().requires_grad_()
    with ops.use_documents(bounds):
        y = model(leaf)
    (y * torch.linspace(-1, 1, y.numel()).view_as(y)).sum().backward()
    return y.detach(), leaf.grad


def test_model_documents_do_not_see_each_other():
    """Outputs and input gradients of one document's tokens do not change when another document's tokens do.
    (Everything else in the blocks is per token; only attention mixes positions.)"""
    cfg = documents_engine.documents_cfg(window=None)
    torch.manual_seed(0)
    blocks = [b for b in build_lm_blocks(cfg) if hasattr(b, "core")]
    assert len(blocks) == cfg.num_layers and all(b.core.causal for b in blocks)
    model = torch.nn.Sequential(*blocks).train()
    n, seq = 2, cfg.seq_len
    lengths = [[5, 1, 10], [7, 9]]
    bounds = document_bounds_from_lengths(lengths, seq)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(n, seq, cfg.d_model, generator=g)
    y0, g0 = _model_run(model, x, bounds)
    x1 = x.clone()
    x1[0, 6:] = torch.randn(seq - 6, cfg.d_model, generator=g)  # row 0: the last document's tokens
    x1[1, :7] = torch.randn(7, cfg.d_model, generator=g)        # row 1: the first document's
    y1, g1 = _model_run(model, x1, bounds)
    assert torch.equal(y1[0, :6], y0[0, :6]) and torch.equal(g1[0, :6], g0[0, :6])
    assert torch.equal(y1[1, 7:], y0[1, 7:]) and torch.equal(g1[1, 7:], g0[1, 7:])
    assert not torch.equal(y1[0, 6:], y0[0, 6:])
    # without the bounds the later document does see the earlier one
    ya, _ = _model_run(model, x, None)
    yb, _ = _model_run(model, x1, None)
    assert not torch.equal(yb[1, 7:], ya[1, 7:])
    # the checkpoint's recompute runs under the bounds its forward ran under
    leaf = x.clone().requires_grad_()
    model.zero_grad()
    with ops.use_documents(bounds):
        y = checkpoint(model, leaf)
    (y * torch.linspace(-1, 1, y.numel()).view_as(y)).sum().backward()
    assert torch.equal(y.detach(), y0) and torch.equal(leaf.grad, g0)


def test_core_checks_the_context():
    kw = dict(norm_first=True, layer_norm_eps=1e-5)
    x = torch.randn(B, S, 32)
    good = document_bounds_from_lengths(LENGTHS, S)
    core = AttentionCore(32, 4, 0.0, causal=False, **kw)
    core(x)
    with ops.use_documents(good):
        with pytest.raises(ValueError, match="not causal"):
            core(x)
    causal = AttentionCore(32, 4, 0.0, causal=True, **kw)
    with ops.use_documents(good[:1]):
        with pytest.raises(ValueError, match="do not match"):
            causal(x)
    with ops.use_documents(good):
        masked = causal(x)
    assert masked.shape == (B, S, 32) and not torch.equal(masked, causal(x))  # the bounds reached the op


# ------------------------------------------------------------------ 5. the engine
def test_engine_step_takes_one_bounds_tensor_per_micro_batch():
    from mipipe.parallel import PipelineEngine

    cfg = documents_engine.documents_cfg()
    torch.manual_seed(0)
    model = torch.nn.Sequential(*build_lm_blocks(cfg)).train()
    eng = PipelineEngine(model, chunks=documents_engine.M, checkpoint="never",
                         act_shape=(documents_engine.MB, cfg.seq_len), act_dtype=torch.float32,
                         loss_fn=documents_engine.engine_cases._loss_fn(cfg), device=torch.device("cpu"))
    inputs, targets, bounds = documents_engine.packed_data(cfg)
    with pytest.raises(ValueError, match="doc_bounds"):
        eng.step(inputs, targets, doc_bounds=bounds[:-1])
    with_docs = float(eng.step(inputs, targets, doc_bounds=bounds).loss)
    ref_loss, _ = documents_engine.unpipelined_reference()
    assert abs(with_docs - ref_loss) < 1e-5 * abs(ref_loss)
    plain = float(eng.step(inputs, targets).loss)
    assert plain == float(eng.step(inputs, targets, doc_bounds=None).loss) and plain != with_docs


def test_train_engine_example_doc_eos():
    """examples/train_engine.py --doc-eos: two gloo ranks train on packed batches (bounds on every rank,
    boundary targets masked); the flag changes the losses."""
    from test_train_engine_example import _run

    packed = _run(2, "--config", "llama_tiny", "--steps", "2", "--doc-eos", "1")
    plain = _run(2, "--config", "llama_tiny", "--steps", "2")
    assert sorted(packed) == sorted(plain) == [0, 1]
    assert all(math.isfinite(float(packed[i][0])) for i in packed) and packed[0] != plain[0]


def test_documents_engine_two_gloo_ranks():
    """Loss and gradients of two ranks equal the unpipelined model under ``use_documents``;
    ``checkpoint="always"`` so every micro-batch's recompute enters the context too."""
    documents_engine.run_documents_engine_case(2, "always")
