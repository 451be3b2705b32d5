"""GPU tests for the fwd+g ("saved-g") path: one kernel emits loss + g slab
+ scalar partials, backward is pure GEMMs.  Verifies it against both the
recompute kernels and the fp32 PyTorch reference."""

import functools
import math
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from distributed_sigmoid_loss_amd import ops
from distributed_sigmoid_loss_amd.losses.functional import (
    sigmoid_contrastive_loss,
    _torch_loss,
    _torch_bwd,
)


def make_inputs(b, n, d, seed=0):
    g = torch.Generator().manual_seed(seed)
    zi = F.normalize(torch.randn(b, d, generator=g), dim=-1)
    zt = F.normalize(torch.randn(n, d, generator=g), dim=-1)
    tp = torch.tensor(math.log(10.0))
    bs = torch.tensor(-10.0)
    return (zi.cuda().bfloat16(), zt.cuda().bfloat16(),
            tp.cuda(), bs.cuda())


def ref_g_and_scalars(zi, zt, tp, bs, diag):
    """fp32 reference of what the fwd+g kernel emits."""
    zi32, zt32 = zi.float(), zt.float()
    t = tp.float().exp()
    dot = zi32 @ zt32.T
    z = dot * t + bs.float()
    lab = -torch.ones_like(z)
    if diag is not None:
        i = torch.arange(zi.shape[0], device=z.device)
        j = i + diag
        m = (j >= 0) & (j < zt.shape[0])
        lab[i[m], j[m]] = 1.0
    loss = F.softplus(-lab * z).sum()
    g = -lab * torch.sigmoid(-lab * z)
    return loss, g, (g * dot).sum(), g.sum()


@pytest.mark.parametrize("b,n,diag", [
    (256, 256, 0),
    (256, 512, 256),
    (300, 260, None),      # ragged edge blocks
    (1024, 2048, 1024),
])
def test_fwdg_matches_reference(b, n, diag):
    d = 768 if b % 8 == 0 else 256
    zi, zt, tp, bs = make_inputs(b, n, d, seed=b + n)
    buf, g, gt = ops.siglip_fwd_g(zi, zt, tp, bs, diag)
    out3 = ops.reduce_out3(buf)
    r_loss, r_g, r_gdot, r_gsum = ref_g_and_scalars(zi, zt, tp, bs, diag)
    torch.cuda.synchronize()
    assert gt is None
    assert torch.allclose(out3[0].cpu(), r_loss.cpu(), rtol=2e-2, atol=1e-2)
    assert torch.allclose(g.float().cpu(), r_g.cpu(), rtol=5e-2, atol=5e-3), \
        (g.float().cpu() - r_g.cpu()).abs().max()
    assert torch.allclose(out3[1].cpu(), r_gdot.cpu(), rtol=2e-2, atol=1e-2)
    assert torch.allclose(out3[2].cpu(), r_gsum.cpu(), rtol=2e-2, atol=1e-2)


def test_fwdg_slab_offset_write():
    """Ring-style assembly: two chunks written at column offsets into one
    (b, 2n) slab must equal the single-call (b, 2n) result."""
    b, n, d = 256, 256, 768
    zi, zt, tp, bs = make_inputs(b, 2 * n, d, seed=3)
    # one call over the full width
    buf_full, g_full, _ = ops.siglip_fwd_g(zi, zt, tp, bs, 64)
    # two chunked calls into a shared slab + shared scalar buffer
    g_slab = torch.empty((b, 2 * n), device="cuda", dtype=torch.bfloat16)
    buf = ops._out_buf("cuda")
    ops.siglip_fwd_g(zi, zt[:n], tp, bs, 64, g_slab=g_slab, col0=0,
                     out3=buf)
    ops.siglip_fwd_g(zi, zt[n:], tp, bs, 64 - n, g_slab=g_slab, col0=n,
                     out3=buf)
    torch.cuda.synchronize()
    assert torch.allclose(ops.reduce_out3(buf), ops.reduce_out3(buf_full),
                          rtol=1e-3, atol=1e-3)
    assert torch.equal(g_slab, g_full)


def test_bwd_from_g_matches_recompute():
    """Full autograd: saved-g backward == recompute backward (bit-comparable
    tolerances; same quantized math, different schedule)."""
    b, n, d = 512, 1024, 768
    results = {}
    for mode in ("1", "0"):
        os.environ["SIGLIP_SAVE_G"] = mode
        try:
            zi, zt, tp, bs = make_inputs(b, n, d, seed=9)
            zi = zi.clone().requires_grad_(True)
            zt = zt.clone().requires_grad_(True)
            tp = tp.clone().requires_grad_(True)
            bs = bs.clone().requires_grad_(True)
            loss = sigmoid_contrastive_loss(zi, zt, tp, bs, diag_offset=0)
            loss.backward()
            torch.cuda.synchronize()
            results[mode] = (loss.detach(), zi.grad, zt.grad, tp.grad,
                             bs.grad)
        finally:
            os.environ.pop("SIGLIP_SAVE_G", None)
    for a, b_ in zip(results["1"], results["0"]):
        assert torch.allclose(a.float(), b_.float(), rtol=2e-2, atol=1e-3)


@pytest.mark.parametrize("quant", ["fp8", "mixed"])
def test_fwdg_quant_matches_recompute(quant):
    """fp8/mixed saved-g path vs the recompute path through full autograd.
    Pins the per-tensor policy — this test compares the two backward
    MECHANICS, and the recompute path is per-tensor by design."""
    b, n, d = 512, 512, 768
    results = {}
    os.environ["SIGLIP_FP8_ROWWISE"] = "0"
    for mode in ("1", "0"):
        os.environ["SIGLIP_SAVE_G"] = mode
        try:
            zi, zt, tp, bs = make_inputs(b, n, d, seed=4)
            zi = zi.clone().requires_grad_(True)
            zt = zt.clone().requires_grad_(True)
            tp = tp.clone().requires_grad_(True)
            bs = bs.clone().requires_grad_(True)
            loss = sigmoid_contrastive_loss(zi, zt, tp, bs, diag_offset=0,
                                            quant=quant)
            loss.backward()
            torch.cuda.synchronize()
            results[mode] = (loss.detach(), zi.grad, zt.grad, tp.grad,
                             bs.grad)
        finally:
            os.environ.pop("SIGLIP_SAVE_G", None)
    os.environ.pop("SIGLIP_FP8_ROWWISE", None)
    for a, b_ in zip(results["1"], results["0"]):
        assert torch.allclose(a.float(), b_.float(), rtol=5e-2, atol=5e-3), \
            (a.float() - b_.float()).abs().max()


@pytest.mark.parametrize("quant", ["fp8", "mixed"])
def test_fwdg_quant_vs_fp32(quant):
    """fp8/mixed saved-g autograd against the fp32 reference (quantization
    tolerances)."""
    b, n, d = 256, 256, 768
    zi, zt, tp, bs = make_inputs(b, n, d, seed=13)
    zi = zi.clone().requires_grad_(True)
    zt = zt.clone().requires_grad_(True)
    tp = tp.clone().requires_grad_(True)
    bs = bs.clone().requires_grad_(True)
    loss = sigmoid_contrastive_loss(zi, zt, tp, bs, diag_offset=0,
                                    quant=quant)
    loss.backward()

    zi2 = zi.detach().float().clone().requires_grad_(True)
    zt2 = zt.detach().float().clone().requires_grad_(True)
    tp2 = tp.detach().float().clone().requires_grad_(True)
    bs2 = bs.detach().float().clone().requires_grad_(True)
    ref = _torch_loss(zi2, zt2, tp2, bs2, 0, col_chunk=None)
    ref.backward()
    torch.cuda.synchronize()

    # Embedding grads pass through the e4m3 grad GEMMs in BOTH policies
    # (mixed differs only in the logits precision), so both get fp8-class
    # tolerances on grads; mixed's loss is bf16-exact.
    rtol, atol = 1e-1, 2e-2
    assert torch.allclose(loss.float(), ref, rtol=5e-2)
    assert torch.allclose(zi.grad.float(), zi2.grad, rtol=rtol, atol=atol)
    assert torch.allclose(zt.grad.float(), zt2.grad, rtol=rtol, atol=atol)
    assert torch.allclose(tp.grad.float(), tp2.grad, rtol=rtol, atol=atol)


def test_rowwise_fp8_vs_fp32_reference():
    """Row-wise fp8 full autograd against the fp32 reference at fp8-class
    tolerances (unit-norm rows)."""
    b, n, d = 512, 512, 768
    os.environ["SIGLIP_FP8_ROWWISE"] = "1"
    try:
        zi, zt, tp, bs = make_inputs(b, n, d, seed=55)
        zi = zi.clone().requires_grad_(True)
        zt = zt.clone().requires_grad_(True)
        tp = tp.clone().requires_grad_(True)
        bs = bs.clone().requires_grad_(True)
        loss = sigmoid_contrastive_loss(zi, zt, tp, bs, diag_offset=0,
                                        quant="fp8")
        loss.backward()
        torch.cuda.synchronize()
    finally:
        os.environ.pop("SIGLIP_FP8_ROWWISE", None)

    zi2 = zi.detach().float().clone().requires_grad_(True)
    zt2 = zt.detach().float().clone().requires_grad_(True)
    tp2 = tp.detach().float().clone().requires_grad_(True)
    bs2 = bs.detach().float().clone().requires_grad_(True)
    ref = _torch_loss(zi2, zt2, tp2, bs2, 0, col_chunk=None)
    ref.backward()
    torch.cuda.synchronize()

    def rel_l2(a, r):
        return float((a.float() - r).norm() / r.norm().clamp(min=1e-12))

    assert torch.allclose(loss.float(), ref, rtol=5e-2)
    assert rel_l2(zi.grad, zi2.grad) < 0.12
    assert rel_l2(zt.grad, zt2.grad) < 0.12
    assert torch.allclose(bs.grad.float(), bs2.grad, rtol=1e-1, atol=1e-2)


def test_rowwise_quant_keeps_per_row_precision():
    """The feature's claim, measured directly: with row norms spanning
    2^-6..2^6, per-tensor e4m3 destroys small rows' relative precision
    while row-wise pow2 scales keep EVERY row at e4m3 precision."""
    b, d = 512, 768
    g = torch.Generator().manual_seed(99)
    # 2^24 spread: beyond e4m3's ~2^17.8 dynamic range, so a single tensor
    # scale must underflow the small rows; row-wise scales keep them exact.
    mag = torch.exp2(torch.randint(-12, 13, (b, 1), generator=g).float())
    x = (F.normalize(torch.randn(b, d, generator=g), dim=-1) * mag)
    x = x.cuda().bfloat16()

    q_r, e8, ratio, s_ref = ops._quant_fp8_rowwise(x)
    # reconstruct: q · 2^(e8-127) per row
    rec_r = q_r.float() * torch.exp2(e8.float() - 127.0).unsqueeze(1)
    qc_t = ops.quantize_fp8_pair(x, x)
    q_t, s_t = qc_t.zi_q, qc_t.si
    rec_t = q_t.float() * s_t
    torch.cuda.synchronize()

    xf = x.float()
    norms = xf.norm(dim=1).clamp(min=1e-12)
    err_r = ((rec_r - xf).norm(dim=1) / norms)
    err_t = ((rec_t - xf).norm(dim=1) / norms)
    # every row stays at e4m3 precision under row-wise scales
    assert err_r.max().item() < 0.05, err_r.max()
    # per-tensor loses the small rows (sanity that the comparison is real)
    assert err_t.max().item() > 0.2, err_t.max()


@pytest.mark.parametrize("b,d", [(256, 768), (1000, 120), (7, 8)])
def test_fused_quant_matches_torch(b, d):
    """Fused amax+cast quantization kernels vs the torch composite."""
    g = torch.Generator().manual_seed(b + d)
    x = (torch.randn(b, d, generator=g) * 2.5).cuda().bfloat16()
    q, s = ops._quant_fp8(x)
    # torch composite reference
    amax = x.detach().abs().amax().float().clamp_(min=2.0 ** -20)
    s_ref = amax / 448.0
    q_ref = (x.float() / s_ref).to(torch.float8_e4m3fn)
    torch.cuda.synchronize()
    assert torch.allclose(s.cpu(), s_ref.cpu(), rtol=1e-6)
    # identical scale => elementwise cast should agree except for ties
    diff = (q.float() - q_ref.float()).abs()
    denom = q_ref.float().abs().clamp(min=1.0)
    assert (diff / denom).max().item() < 0.07, (diff / denom).max()


def test_fp8_wire_simulated_roundtrip_gpu():
    """The fp8 ring's wire math on one GPU: quantize a chunk, 'transmit' its
    uint8 view + scale, reconstruct the receiver's qcache, and compute —
    must match computing directly from the sender's quantization."""
    b, n, d = 512, 512, 768
    zi, zt, tp, bs = make_inputs(b, n, d, seed=31)
    zi_q, si = ops._quant_fp8(zi)
    zt_q, st = ops._quant_fp8(zt)
    # "wire": uint8 payload + (1,) fp32 scale, as parallel.ring ships them
    wire_q = zt_q.view(torch.uint8).contiguous().clone()
    wire_s = st.reshape(1).float().clone()
    rq = wire_q.view(torch.float8_e4m3fn)
    rs = wire_s.reshape(())
    assert torch.equal(rq, zt_q) and torch.equal(rs, st.reshape(()))

    direct = ops.siglip_fwd_g(zi, zt, tp, bs, None, quant="fp8",
                              qcache=ops.QuantCache(zi_q, zt_q, si, st))
    via_wire = ops.siglip_fwd_g(zi, (rq.to(torch.float32) * rs).to(zt.dtype),
                                tp, bs, None, quant="fp8",
                                qcache=ops.QuantCache(zi_q, rq, si, rs))
    torch.cuda.synchronize()
    assert torch.equal(ops.reduce_out3(direct[0]), ops.reduce_out3(via_wire[0]))
    assert torch.equal(direct[1], via_wire[1])          # g slabs bitwise
    assert torch.equal(direct[2], via_wire[2])          # gt slabs bitwise


def test_banded_savedg_matches_recompute():
    """Column-banded saved-g (the huge-batch regime, forced small here via
    env) == recompute backward == fp32 reference."""
    b, n, d = 512, 1024, 768
    outs = {}
    for mode, env in (("banded", {"SIGLIP_SAVE_G_MAX_BYTES": "1000",
                                  "SIGLIP_BANDED_STEP": "256"}),
                      ("recompute", {"SIGLIP_SAVE_G": "0"})):
        for k, v in env.items():
            os.environ[k] = v
        try:
            zi, zt, tp, bs = make_inputs(b, n, d, seed=77)
            zi = zi.clone().requires_grad_(True)
            zt = zt.clone().requires_grad_(True)
            tp = tp.clone().requires_grad_(True)
            bs = bs.clone().requires_grad_(True)
            loss = sigmoid_contrastive_loss(zi, zt, tp, bs, diag_offset=256)
            loss.backward()
            torch.cuda.synchronize()
            outs[mode] = (loss.detach(), zi.grad, zt.grad, tp.grad, bs.grad)
        finally:
            for k in env:
                os.environ.pop(k, None)
    for a, b_ in zip(outs["banded"], outs["recompute"]):
        assert torch.allclose(a.float(), b_.float(), rtol=2e-2, atol=1e-3), \
            (a.float() - b_.float()).abs().max()


@pytest.mark.parametrize("n", [768, 700])
def test_banded_grads_three_bands(n):
    """The banded backward through ops.grad_gemms at three 256-column bands
    — last one full (768) and ragged (700, 188 columns) — against the
    recompute path, at test_banded_savedg_matches_recompute's tolerances."""
    b, d = 512, 256
    outs = {}
    for mode, env in (("banded", {"SIGLIP_SAVE_G_MAX_BYTES": "1000",
                                  "SIGLIP_BANDED_STEP": "256"}),
                      ("recompute", {"SIGLIP_SAVE_G": "0"})):
        for k, v in env.items():
            os.environ[k] = v
        try:
            zi, zt, tp, bs = make_inputs(b, n, d, seed=78)
            zi = zi.clone().requires_grad_(True)
            zt = zt.clone().requires_grad_(True)
            tp = tp.clone().requires_grad_(True)
            bs = bs.clone().requires_grad_(True)
            loss = sigmoid_contrastive_loss(zi, zt, tp, bs, diag_offset=100)
            loss.backward()
            torch.cuda.synchronize()
            outs[mode] = (loss.detach(), zi.grad, zt.grad, tp.grad, bs.grad)
        finally:
            for k in env:
                os.environ.pop(k, None)
    for a, b_ in zip(outs["banded"], outs["recompute"]):
        assert torch.allclose(a.float(), b_.float(), rtol=2e-2, atol=1e-3), \
            (a.float() - b_.float()).abs().max()


@pytest.mark.parametrize("b", [256, 260])   # interior tiles / ragged edge
def test_fp8_ring_recompute_single_gpu(b):
    """The ring Function's fp8 RECOMPUTE backward (SIGLIP_SAVE_G=0), which
    hands each chunk's forward quantization to chunk_loss_bwd, at W=1
    against the plain fused loss under the same env: the same kernels on the
    same quantized inputs, at the fp8 saved-g-vs-recompute bound."""
    from distributed_sigmoid_loss_amd.losses.sigmoid_loss import (
        _RingAllGatherLoss)
    d = 128
    results = {}
    os.environ["SIGLIP_SAVE_G"] = "0"
    try:
        for mode in ("ring", "plain"):
            zi, zt, tp, bs = make_inputs(b, b, d, seed=21)
            zi = zi.clone().requires_grad_(True)
            zt = zt.clone().requires_grad_(True)
            tp = tp.clone().requires_grad_(True)
            bs = bs.clone().requires_grad_(True)
            if mode == "ring":
                # (group, col_chunk, impl, quant, want_grad, bidir); no
                # process group, so W=1
                loss = _RingAllGatherLoss.apply(zi, zt, tp, bs, None, None,
                                                "auto", "fp8", True, False)
            else:
                loss = sigmoid_contrastive_loss(zi, zt, tp, bs,
                                                diag_offset=0, quant="fp8")
            loss.backward()
            torch.cuda.synchronize()
            results[mode] = (loss.detach(), zi.grad, zt.grad, tp.grad,
                             bs.grad)
    finally:
        os.environ.pop("SIGLIP_SAVE_G", None)
    for a, b_ in zip(results["ring"], results["plain"]):
        assert torch.allclose(a.float(), b_.float(), rtol=5e-2, atol=5e-3), \
            (a.float() - b_.float()).abs().max()


# ---------------------------------------------------------------------------
# The ring's chunk accumulator (_RingChunks) and wire formats driven directly
# on one GPU, no process group: W=3, rank=1 (the positive diagonal sits in the
# middle block), chunks added in bidirectional arrival order (own, right,
# left).  The oracle is the plain fused loss over the concatenated text on the
# same device in the same regime.
#
# Inputs follow tests/test_gpu_tile_exact.py's informative regime,
# t' = log(1.5 / std(dot)) and bias = -0.5, so the negatives carry weight: a
# dropped or misplaced chunk moves every output by tens of percent.  For fp8
# the three text chunks are scaled by distinct factors in [2/3, 3/2]: their
# per-tensor scales differ by 1.5x steps, and a mispaired scale is visible.
# ---------------------------------------------------------------------------

RING_W, RING_RANK, RING_D = 3, 1, 128
RING_ORDER = (1, 2, 0)
RING_FACTORS = {"fp8": (2.0 / 3.0, 1.0, 1.5)}
RING_NAMES = ("loss", "dzimg", "dtxt_flat", "dt_prime", "dbias")


@functools.lru_cache(maxsize=None)
def _ring_case(b, scaled):
    """Inputs plus the float64 reference (loss, grads, informative fraction),
    computed once per key from the bf16 values and never modified."""
    gen = torch.Generator().manual_seed(7000 + b)
    factors = RING_FACTORS["fp8"] if scaled else (1.0,) * RING_W
    zi = F.normalize(torch.randn(b, RING_D, generator=gen), dim=-1)
    chunks = [F.normalize(torch.randn(b, RING_D, generator=gen), dim=-1) * f
              for f in factors]
    zi = zi.cuda().bfloat16()
    chunks = tuple(c.cuda().bfloat16() for c in chunks)
    zi64 = zi.double().requires_grad_(True)
    zt64 = torch.cat(chunks).double().requires_grad_(True)
    dot = (zi64 @ zt64.T).detach()
    tp64 = torch.tensor(math.log(1.5 / float(dot.std())), device="cuda",
                        dtype=torch.float64, requires_grad=True)
    bs64 = torch.tensor(-0.5, device="cuda", dtype=torch.float64,
                        requires_grad=True)
    diag = RING_RANK * b
    loss = _torch_loss(zi64, zt64, tp64, bs64, diag, col_chunk=None)
    loss.backward()
    lab = -torch.ones_like(dot)
    i = torch.arange(b, device="cuda")
    lab[i, i + diag] = 1.0
    g = torch.sigmoid(-lab * (dot * tp64.detach().exp() + bs64.detach()))
    informative = float(((g >= 0.05) & (g <= 0.95)).double().mean())
    ref = (loss.detach(), zi64.grad, zt64.grad, tp64.grad, bs64.grad)
    return (zi, chunks, tp64.detach().float(), bs64.detach().float(), ref,
            informative)


def _ring_run(b, quant, want_grad=True):
    """Drive wire + accumulator as _RingAllGatherLoss does → (acc, outputs)."""
    from distributed_sigmoid_loss_amd.losses.sigmoid_loss import (
        _Fp8Wire, _PlainWire, _RingChunks)
    zi, chunks, tp, bs, _, _ = _ring_case(b, quant == "fp8")
    wire = _Fp8Wire(zi) if quant == "fp8" else _PlainWire()
    payloads = [wire.pack(c) for c in chunks]     # each owner's quantization
    acc = _RingChunks(zi, tp, bs, RING_W, RING_RANK, b, quant, None, "auto",
                      want_grad)
    for src in RING_ORDER:
        if src == RING_RANK:
            acc.add(src, chunks[src], wire.qcache(payloads[src]), 0)
        else:
            acc.add(src, *wire.unpack(payloads[src]), None)
    loss = acc.loss()
    if not want_grad:
        torch.cuda.synchronize()
        return acc, (loss,)
    # backward sees only what a Function would have saved
    back = _RingChunks.from_tensors(acc.tensors(), **acc.meta())
    fired = []
    grads = back.grads(torch.ones((), device="cuda"), fired.append)
    torch.cuda.synchronize()
    assert len(fired) == 1 and fired[0] is grads[1]
    return acc, (loss,) + tuple(grads)


def _plain_run(b, quant):
    zi, chunks, tp, bs, _, _ = _ring_case(b, quant == "fp8")
    zi, zt, tp, bs = (t.clone().requires_grad_(True)
                      for t in (zi, torch.cat(chunks), tp, bs))
    loss = sigmoid_contrastive_loss(zi, zt, tp, bs,
                                    diag_offset=RING_RANK * b, quant=quant)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), zi.grad, zt.grad, tp.grad, bs.grad


def _err(a, b_, ref):
    """‖a − b‖ / ‖ref‖ in float64 (|·| for scalars)."""
    return float((a.double() - b_.double()).norm() / ref.double().norm())


def _set_regime(monkeypatch, save_g):
    monkeypatch.delenv("SIGLIP_FP8_ROWWISE", raising=False)
    if save_g:
        monkeypatch.delenv("SIGLIP_SAVE_G", raising=False)
    else:
        monkeypatch.setenv("SIGLIP_SAVE_G", "0")


@pytest.mark.parametrize("save_g", [True, False], ids=["savedg", "recompute"])
@pytest.mark.parametrize("quant", ["bf16", "mixed"])
@pytest.mark.parametrize("b", [256, 260])   # interior tiles / ragged edge
def test_ring_chunks_match_plain(b, quant, save_g, monkeypatch):
    """bf16/mixed: the accumulator launches the plain path's kernels on the
    same bits (test_fwdg_slab_offset_write: the chunked slab is torch.equal to
    the single-call one) and makes the same GEMM calls.  Scalars come out of
    atomics, so they get that test's tolerance; the gradient tensors must
    agree to one bf16 unit roundoff normwise (2^-8) — exact equality is
    expected, anything larger is a bug."""
    _set_regime(monkeypatch, save_g)
    *_, ref, informative = _ring_case(b, False)
    assert informative >= 0.9, informative
    acc, ring = _ring_run(b, quant)
    assert acc.regime == ("slab" if save_g else "concat_recompute")
    plain = _plain_run(b, quant)
    for name, r, p in zip(RING_NAMES, ring, plain):
        print(f"{name}: ring-vs-plain {_err(r, p, p):.3e}")
    for name, r, p in zip(RING_NAMES, ring, plain):
        if name in ("dzimg", "dtxt_flat"):
            assert _err(r, p, p) <= 2.0 ** -8, name
        else:
            assert torch.allclose(r.float(), p.float(), rtol=1e-3,
                                  atol=1e-3), name


@pytest.mark.parametrize("save_g", [True, False], ids=["savedg", "recompute"])
@pytest.mark.parametrize("b", [256, 260])   # 260: the dequantize-GEMM route
def test_ring_chunks_fp8_match_plain(b, save_g, monkeypatch):
    """fp8: the ring quantizes each text chunk with its owner's scale, the
    plain path the whole block with one, so the two are independently rounded
    results.  Per output, q = ‖plain − ref64‖/‖ref64‖ is the quantization
    floor of code the ring does not touch; two results each within about q of
    exact are within 2q of each other (triangle inequality), so the bound is
    ‖ring − plain‖/‖ref64‖ <= 2q.  A dropped chunk (~50 %) or a scale
    mispaired by >= 1.5x is far above it."""
    _set_regime(monkeypatch, save_g)
    *_, ref, informative = _ring_case(b, True)
    assert informative >= 0.9, informative
    acc, ring = _ring_run(b, "fp8")
    assert acc.regime == ("chunk_slabs" if save_g else "chunk_recompute")
    plain = _plain_run(b, "fp8")
    figures = [(name, _err(p, f, f), _err(r, p, f))
               for name, r, p, f in zip(RING_NAMES, ring, plain, ref)]
    for name, q, e in figures:
        print(f"{name}: q {q:.3e}  ring-vs-plain {e:.3e}")
    for name, q, e in figures:
        assert e <= 2 * q, (name, q, e)


def test_ring_chunks_no_grad_takes_scalar_forward(monkeypatch):
    """want_grad=False: no slab is allocated or kept, every chunk runs the
    scalar-only forward kernel, and the loss equals the saved-g loss."""
    _set_regime(monkeypatch, True)
    b = 260
    *_, informative = _ring_case(b, False)
    assert informative >= 0.9, informative
    acc, (loss,) = _ring_run(b, "bf16", want_grad=False)
    assert acc.regime == "concat_recompute"
    assert acc.g is None and acc.out3 is None
    assert set(acc.tensors()) == {"zimg", "t_prime", "bias", "chunks.0",
                                  "chunks.1", "chunks.2"}
    acc_g, ring_g = _ring_run(b, "bf16")
    assert acc_g.regime == "slab"
    assert torch.allclose(loss, ring_g[0], rtol=1e-3, atol=1e-3)


def test_inference_skips_slab():
    """Under no_grad the plain forward kernel runs (no g allocation) — the
    loss is identical either way."""
    b, n, d = 256, 256, 768
    zi, zt, tp, bs = make_inputs(b, n, d, seed=2)
    with torch.no_grad():
        l1 = sigmoid_contrastive_loss(zi, zt, tp, bs, diag_offset=0)
    zi_g = zi.clone().requires_grad_(True)
    l2 = sigmoid_contrastive_loss(zi_g, zt, tp, bs, diag_offset=0)
    torch.cuda.synchronize()
    assert torch.allclose(l1, l2.detach(), rtol=1e-3, atol=1e-3)
