"""Sigmoid contrastive loss with sample-ID labels.

``sigmoid_contrastive_loss`` decides what a positive pair is by position:
row ``i`` matches column ``i + diag_offset`` and everything else is a
negative.  Real image–text batches break that rule — repeated captions and
images in a web-scale batch, several captions per image, padding rows of a
fixed-shape batch — and the sigmoid loss has no normaliser to dilute a false
negative: it is a flatly wrong label with full weight.  Here two int64 id
vectors say which pairs match.

One contract for every implementation.  With ``s_ij = <zimg_i, ztxt_j>`` and
``z_ij = t·s_ij + bias``, ``t = exp(t_prime)``, a pair is

- **masked** where ``img_ids[i] < 0`` or ``txt_ids[j] < 0``: a negative id
  switches off a whole row or column (padding, filtered samples);
- ``duplicates="positive"`` (default): **positive** where the ids are equal,
  negative otherwise — any number of positives per row or column, or none;
- ``duplicates="ignore"``: the positive is ``j == i + diag_offset`` (none if
  ``None``), whatever the ids of that pair; a pair with equal ids off that
  diagonal is masked (false-negative removal with the position as the only
  positive); everything else is negative.

With ``l = ±1``:

    total = Σ_{not masked} softplus(−l_ij·z_ij)
    g_ij  = −l_ij·σ(−l_ij·z_ij)                    (0 where masked)
    dzimg = t·g@ztxt   dztxt = t·gᵀ@zimg   dt' = t·Σ g_ij·s_ij   dbias = Σ g_ij

``total`` is in sum form and the caller normalises.  With ``img_ids =
arange(b) + diag``, ``txt_ids = arange(n)`` and ``"positive"`` this is exactly
``sigmoid_contrastive_loss(diag_offset=diag)``.  Ids are compared as 64-bit
values.

On GPU (bf16) the fused kernel ``ops.sigmoid_ids`` evaluates the grid tile by
tile, never building the logits, in one of two regimes:

- *saved-g* — gradients wanted, ``col_chunk is None`` and the bf16 g slab
  below 2³² bytes: the forward emits the loss partials and the dL/dlogit slab
  in one pass; the backward is the two gradient GEMMs (``ops.grad_gemms``)
  plus the scalar gradients from the saved partials.
- *band recompute* — otherwise: the forward runs the loss-only kernel per
  column chunk; the backward re-runs the kernel per band through
  ``ops.band_grad_gemms``.

``quant="mixed"`` (GPU path only) keeps all of that — exact bf16 logits, the
same loss, ``dt'`` and ``dbias`` bit for bit — and runs the two gradient GEMMs
in fp8: ``ops.sigmoid_ids_e4m3`` writes dL/dlogit as an e4m3 slab pair (``g``
and ``gᵀ``, ``448·g``; together the bytes of the bf16 slab), the embeddings
are quantised per tensor (``ops.quantize_fp8_pair``) and ``ops.grad_gemms``
takes the hipBLASLt fp8 route where every GEMM dimension is 16-aligned, the
dequantise route otherwise.  Only ``dzimg`` and ``dztxt`` carry fp8 error.

``quant="fp8"`` (GPU path only) runs the logits on e4m3 operands as well: the
embeddings are quantised once per step (``ops.quantize_fp8_pair``; the cache
travels to the backward), ``ops.sigmoid_ids_fp8`` reads the e4m3 pair on the
MX-scaled MFMA with unit block scales — the per-tensor scales are added to
``t'`` on the device, ``t' + log s_img + log s_txt`` — and writes the same
e4m3 slab pair, or nothing in the loss-only form the band regime and
forwards without gradients use.  The backward is the ``mixed`` one, straight
through the quantisation; ``dt' = exp(t' + log s_img + log s_txt)·Σ g·s`` with
``s`` the raw e4m3 dot.  Loss, ``dt'`` and ``dbias`` are those of the
quantised embeddings, not the bf16 path's bits.

``quant="mxfp8"`` (GPU path only, ``d % 32 == 0``) is the ``fp8`` policy with
OCP MX block scales instead of one scale per tensor: ``ops.quantize_mx`` gives
each operand e4m3 elements and one e8m0 scale per 32 consecutive elements of
a row (one pass, once per step), and ``ops.sigmoid_ids_mx`` hands the scales
to the MX-scaled MFMA, so ``s`` is the true dot of the dequantised values and
``t'`` is passed unchanged.  A block's scale is set by its own maximum, so
rows or blocks of very different magnitude keep e4m3's precision where one
per-tensor scale would flush the small ones; on unit-norm rows the logits are
as accurate as ``fp8``'s, not more (``profiles/README.md``).  Regimes as for ``fp8`` (bands slice the
text elements, scales and ids by rows); the backward is the ``mixed`` one
unchanged — a per-tensor ``ops.quantize_fp8_pair`` of the bf16 embeddings
for the two gradient GEMMs — and ``dt' = exp(t')·Σ g·s``, straight through.

Not built: ids under ``fp8`` / ``mixed`` / ``mxfp8`` in
``DistributedSigmoidLoss``, and MX operands for the gradient GEMMs.

Per-tile partials are summed in fp64 on the device; nothing syncs with the
host.  Elsewhere a differentiable torch composite with the same contract runs
(fp32 compute, fp64 for fp64 inputs) — the CPU path and the tests' reference.
"""

from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from .. import ops

_DUPLICATES = ("positive", "ignore")
_QUANTS = ("bf16", "mixed", "fp8", "mxfp8")


def pair_classes(img_ids: torch.Tensor, txt_ids: torch.Tensor,
                 duplicates: str = "positive",
                 diag_offset: Optional[int] = None, col0: int = 0):
    """``(positive, masked)`` boolean ``(b, c)`` matrices of the pair grid of
    ``img_ids (b,)`` × ``txt_ids (c,)``; ``col0`` is the column of the full
    grid at which this block starts (``diag_offset`` refers to the full
    grid).  The contract of the module docstring, spelled out densely — what
    the torch path evaluates chunk by chunk."""
    if duplicates not in _DUPLICATES:
        raise ValueError(f"unknown duplicates {duplicates!r}")
    b, c = img_ids.shape[0], txt_ids.shape[0]
    eq = img_ids[:, None] == txt_ids[None, :]
    masked = (img_ids < 0)[:, None] | (txt_ids < 0)[None, :]
    if duplicates == "positive":
        return eq, masked
    diag = torch.zeros((b, c), dtype=torch.bool, device=img_ids.device)
    if diag_offset is not None:
        rows = torch.arange(b, device=img_ids.device)
        cols = rows + (int(diag_offset) - col0)
        ok = (cols >= 0) & (cols < c)
        diag[rows[ok], cols[ok]] = True
    return diag, masked | (eq & ~diag)


def _torch_loss_ids(zimg, ztxt, t_prime, bias, img_ids, txt_ids, duplicates,
                    diag_offset, col_chunk):
    """Differentiable composite, chunked over columns: holds ``O(b ·
    col_chunk)`` logits at a time."""
    n = ztxt.shape[0]
    cdt = torch.float64 if zimg.dtype == torch.float64 else torch.float32
    dev = zimg.device
    zi = zimg.to(cdt)
    t = t_prime.to(device=dev, dtype=cdt).exp()
    bs = bias.to(device=dev, dtype=cdt)
    step = int(col_chunk) if col_chunk and col_chunk > 0 else n
    total = None
    for j0 in range(0, n, step):
        j1 = min(j0 + step, n)
        logits = zi @ ztxt[j0:j1].to(cdt).T * t + bs
        pos, masked = pair_classes(img_ids, txt_ids[j0:j1], duplicates,
                                   diag_offset, j0)
        term = -F.logsigmoid(torch.where(pos, logits, -logits))
        part = term.masked_fill(masked, 0.0).sum()
        total = part if total is None else total + part
    return total


class _FusedIdLoss(torch.autograd.Function):
    """GPU path: ``ops.sigmoid_ids`` (``mixed``: ``ops.sigmoid_ids_e4m3``;
    ``fp8``: ``ops.sigmoid_ids_fp8`` on the quantised pair; ``mxfp8``:
    ``ops.sigmoid_ids_mx`` on the MX pair) plus the library gradient GEMMs, in the saved-g or the band-recompute regime (module
    docstring)."""

    @staticmethod
    def forward(ctx, zimg, ztxt, t_prime, bias, img_ids, txt_ids, duplicates,
                diag_offset, col_chunk, want_grad, quant):
        zimg, ztxt = zimg.contiguous(), ztxt.contiguous()
        b, n = zimg.shape[0], ztxt.shape[0]
        fp8 = quant == "fp8"
        zi_k, zt_k, tp_k, qts = zimg, ztxt, t_prime, ()
        if fp8:
            # One quantisation per step; the kernel reads the e4m3 pair with
            # unit scales and the per-tensor scales ride on the temperature.
            ops._validate(zimg, ztxt, "fp8")
            qc = ops.quantize_fp8_pair(zimg, ztxt)
            zi_k, zt_k, qts = qc.zi_q, qc.zt_q, qc.tensors()
            tp_k = (ops._prep_scalar(t_prime, zimg.device) + qc.si.log()
                    + qc.st.log())
        mx = quant == "mxfp8"
        if mx:
            # One MX quantisation per step; the block scales are applied in
            # the kernel's dot, so t' goes in unchanged.
            ops._validate(zimg, ztxt, "bf16")
            if zimg.shape[1] % 32 != 0:
                raise RuntimeError(
                    f"emb dim must be a multiple of 32 for mxfp8 (got "
                    f"{zimg.shape[1]})")
            zi_q, zi_e8 = ops.quantize_mx(zimg)
            zt_q, zt_e8 = ops.quantize_mx(ztxt)
        # want_grad comes from the caller (grad mode is off in here).
        save_g = want_grad and col_chunk is None and b * n * 2 < 2 ** 32
        if save_g and mx:
            partials, *slabs = ops.sigmoid_ids_mx(
                zi_q, zi_e8, zt_q, zt_e8, t_prime, bias, img_ids, txt_ids,
                duplicates, diag_offset)
        elif save_g:
            emit = {"bf16": ops.sigmoid_ids, "mixed": ops.sigmoid_ids_e4m3,
                    "fp8": ops.sigmoid_ids_fp8}[quant]
            # (partials, g) or, mixed and fp8, (partials, g8, gt8)
            partials, *slabs = emit(zi_k, zt_k, tp_k, bias, img_ids, txt_ids,
                                    duplicates, diag_offset)
        if save_g:
            sums = partials.double().sum(dim=0)
            ctx.save_for_backward(zimg, ztxt, t_prime, bias, img_ids,
                                  txt_ids, *qts, sums, *slabs)
            loss = sums[0]
        else:
            step = min(n, int(col_chunk) if col_chunk and col_chunk > 0
                       else ops.banded_col_step(b))
            loss_only = ops.sigmoid_ids_fp8 if fp8 else ops.sigmoid_ids
            loss = torch.zeros((), device=zimg.device, dtype=torch.float64)
            if mx:
                qts = (zi_q, zi_e8, zt_q, zt_e8)   # the bands' recompute
            for j0, j1, diag_j in ops.col_bands(n, step, diag_offset):
                labels = (bias, img_ids, txt_ids[j0:j1], duplicates, diag_j)
                if mx:
                    partials = ops.sigmoid_ids_mx(
                        zi_q, zi_e8, zt_q[j0:j1], zt_e8[j0:j1], t_prime,
                        *labels, want_g=False)[0]
                else:
                    partials = loss_only(zi_k, zt_k[j0:j1], tp_k, *labels,
                                         want_g=False)[0]
                # the same reduction as saved-g: one block gives the same bits
                loss = loss + partials.double().sum(dim=0)[0]
            ctx.save_for_backward(zimg, ztxt, t_prime, bias, img_ids,
                                  txt_ids, *qts)
            ctx.step = step
        ctx.save_g, ctx.quant, ctx.n_q = save_g, quant, len(qts)
        ctx.duplicates, ctx.diag_offset = duplicates, diag_offset
        return loss.float()

    @staticmethod
    def backward(ctx, grad_output):
        zimg, ztxt, t_prime, bias, img_ids, txt_ids = ctx.saved_tensors[:6]
        rest = ctx.saved_tensors[6 + ctx.n_q:]
        n, dev = ztxt.shape[0], zimg.device
        fp8, fp8_gemms = ctx.quant == "fp8", ctx.quant != "bf16"
        mx = ctx.quant == "mxfp8"
        go = ops._go_scalar(grad_output, dev)
        t = ops._prep_scalar(t_prime, dev).exp()
        # mixed, mxfp8: one per-tensor quantisation of the embeddings for both
        # GEMMs; fp8: the forward's.
        qc = None
        if fp8:
            qc = ops.QuantCache.from_tensors(ctx.saved_tensors[6:6 + ctx.n_q])
        elif fp8_gemms:
            qc = ops.quantize_fp8_pair(zimg, ztxt)
        # The kernel's t' and what multiplies its Σ g·s in dt': under fp8 the
        # dot is of e4m3 values, so the per-tensor scales come back in here
        # (the forward's expression, for the forward's bits).
        tp_k, t_k = t_prime, t
        if fp8:
            tp_k = (ops._prep_scalar(t_prime, dev) + qc.si.log()
                    + qc.st.log())
            t_k = tp_k.exp()
        if ctx.save_g:
            sums, g, *gt = rest
            # bf16_scale=True: the products stay bf16 (see ops.grad_gemms).
            # The GEMMs see the true temperature and, off the fp8 route, the
            # bf16 embeddings: straight-through w.r.t. the quantisation.
            dzimg, dztxt = ops.grad_gemms(
                ops.GBand(g, gt[0] if gt else None, ztxt, qc), zimg, n,
                go * t, bf16_scale=True)
        else:
            parts = []

            def emit(j0, j1, diag_j, g, gt):
                labels = (bias, img_ids, txt_ids[j0:j1], ctx.duplicates,
                          diag_j)
                if fp8:
                    partials = ops.sigmoid_ids_fp8(
                        qc.zi_q, qc.zt_q[j0:j1], tp_k, *labels, g=g, gt=gt)[0]
                elif mx:
                    zi_q, zi_e8, zt_q, zt_e8 = ctx.saved_tensors[6:10]
                    partials = ops.sigmoid_ids_mx(
                        zi_q, zi_e8, zt_q[j0:j1], zt_e8[j0:j1], tp_k, *labels,
                        g=g, gt=gt)[0]
                elif fp8_gemms:
                    partials = ops.sigmoid_ids_e4m3(
                        zimg, ztxt[j0:j1], tp_k, *labels, g=g, gt=gt)[0]
                else:
                    partials = ops.sigmoid_ids(
                        zimg, ztxt[j0:j1], tp_k, *labels, g=g)[0]
                parts.append(partials.double().sum(dim=0))

            # bf16_scale stays False, also when one band covers the block.
            dzimg, dztxt = ops.band_grad_gemms(
                zimg, ztxt, ctx.step, emit, go * t,
                diag_offset=ctx.diag_offset,
                g_dtype=torch.float8_e4m3fn if fp8_gemms else torch.bfloat16,
                with_gt=fp8_gemms, qc=qc)
            sums = torch.stack(parts).sum(dim=0)
        dt = sums[1] * (go * t_k).double()
        db = sums[2] * go.double()
        return (dzimg, dztxt,
                dt.to(device=t_prime.device,
                      dtype=t_prime.dtype).reshape(t_prime.shape),
                db.to(device=bias.device, dtype=bias.dtype).reshape(bias.shape),
                None, None, None, None, None, None, None)


def _ids_vector(name: str, ids, length: int, device) -> torch.Tensor:
    if (not isinstance(ids, torch.Tensor) or ids.dim() != 1
            or ids.shape[0] != length or ids.is_floating_point()
            or ids.is_complex() or ids.dtype == torch.bool):
        raise ValueError(
            f"{name} must be an integer tensor of shape ({length},) (got "
            f"{getattr(ids, 'dtype', type(ids))} "
            f"{tuple(getattr(ids, 'shape', ()))})")
    return ids.detach().to(device=device, dtype=torch.int64).contiguous()


def sigmoid_contrastive_loss_ids(zimg: torch.Tensor, ztxt: torch.Tensor,
                                 t_prime: torch.Tensor, bias: torch.Tensor,
                                 img_ids: torch.Tensor, txt_ids: torch.Tensor,
                                 duplicates: str = "positive",
                                 diag_offset: Optional[int] = None,
                                 col_chunk: Optional[int] = None,
                                 impl: str = "auto",
                                 quant: str = "bf16") -> torch.Tensor:
    """Sum of per-pair sigmoid cross-entropy over the ``(b, n)`` block with
    the labels taken from sample ids (see the module docstring).
    Differentiable in ``zimg``, ``ztxt``, ``t_prime`` and ``bias``.

    Args:
        zimg: ``(b, d)`` image embeddings (L2-normalized by the caller).
        ztxt: ``(n, d)`` text embeddings.
        t_prime: scalar; the temperature is ``exp(t_prime)``.
        bias: scalar additive logit bias.
        img_ids, txt_ids: integer ``(b,)`` / ``(n,)`` sample ids (int64 on
            the embeddings' device is used as is); a negative id masks the
            whole row / column.
        duplicates: ``"positive"`` — equal ids are positives; ``"ignore"`` —
            the positive is ``j == i + diag_offset`` and other pairs with
            equal ids count for nothing.
        diag_offset: column of row 0's positional positive, used only with
            ``"ignore"``; ``None``: no positional positive.
        col_chunk: columns per kernel pass, bounding the workspace to
            ``O(b · col_chunk)``; ``None``: the whole block (saved-g when
            gradients are wanted and the slab stays below 2³² bytes).
        impl: ``auto`` (``hip`` on GPU for bf16, ``torch`` elsewhere) |
            ``hip`` (bf16 on GPU, ``d % 8 == 0``; raises without the built
            extension or for other dtypes) | ``torch``.
        quant: ``"bf16"`` | ``"mixed"`` — exact bf16 logits, e4m3 dL/dlogit
            slabs and fp8 gradient GEMMs on the ``hip`` path (module
            docstring); it has no effect on the ``torch`` path, which has no
            fp8 GEMM.  ``"fp8"`` — e4m3 logit operands as well, ``hip`` path
            only (``d % 16 == 0``); with the ``torch`` path, which has no
            e4m3 logits, it raises ``ValueError``.  ``"mxfp8"`` — the same
            with OCP MX block scales, one e8m0 scale per 32 elements, applied
            in the kernel (``d % 32 == 0``); ``hip`` path only, ``ValueError``
            with the ``torch`` path.

    Returns a 0-d tensor; the caller normalises.
    """
    if zimg.dim() != 2 or ztxt.dim() != 2 or zimg.shape[1] != ztxt.shape[1]:
        raise ValueError(
            f"shape mismatch: zimg {tuple(zimg.shape)} ztxt {tuple(ztxt.shape)}")
    if duplicates not in _DUPLICATES:
        raise ValueError(f"unknown duplicates {duplicates!r}")
    if quant not in _QUANTS:
        raise ValueError(f"unknown quant {quant!r}")
    if impl == "auto":
        impl = ("hip" if zimg.is_cuda and zimg.dtype == torch.bfloat16
                and ztxt.dtype == torch.bfloat16 else "torch")
    if impl not in ("hip", "torch"):
        raise ValueError(f"unknown impl {impl!r}")
    if quant in ("fp8", "mxfp8") and impl == "torch":
        # no e4m3 logits here, and bf16-policy values would be a silent lie
        raise ValueError(
            f"quant={quant!r} needs the hip path (bf16 embeddings on a GPU); "
            "the torch path has no e4m3 logits")
    img_ids = _ids_vector("img_ids", img_ids, zimg.shape[0], zimg.device)
    txt_ids = _ids_vector("txt_ids", txt_ids, ztxt.shape[0], zimg.device)
    if duplicates != "ignore":
        diag_offset = None
    if impl == "torch":
        return _torch_loss_ids(zimg, ztxt, t_prime, bias, img_ids, txt_ids,
                               duplicates, diag_offset, col_chunk)
    want_grad = torch.is_grad_enabled() and any(
        t.requires_grad for t in (zimg, ztxt, t_prime, bias))
    return _FusedIdLoss.apply(zimg, ztxt, t_prime, bias, img_ids, txt_ids,
                              duplicates, diag_offset, col_chunk, want_grad,
                              quant)
