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
    """GPU path: ``ops.sigmoid_ids`` plus the library gradient GEMMs, in the
    saved-g or the band-recompute regime (module docstring)."""

    @staticmethod
    def forward(ctx, zimg, ztxt, t_prime, bias, img_ids, txt_ids, duplicates,
                diag_offset, col_chunk, want_grad):
        zimg, ztxt = zimg.contiguous(), ztxt.contiguous()
        b, n = zimg.shape[0], ztxt.shape[0]
        # want_grad comes from the caller (grad mode is off in here).
        save_g = want_grad and col_chunk is None and b * n * 2 < 2 ** 32
        if save_g:
            partials, g = ops.sigmoid_ids(
                zimg, ztxt, t_prime, bias, img_ids, txt_ids, duplicates,
                diag_offset)
            sums = partials.double().sum(dim=0)
            ctx.save_for_backward(zimg, ztxt, t_prime, bias, img_ids,
                                  txt_ids, sums, g)
            loss = sums[0]
        else:
            step = min(n, int(col_chunk) if col_chunk and col_chunk > 0
                       else ops.banded_col_step(b))
            loss = torch.zeros((), device=zimg.device, dtype=torch.float64)
            for j0, j1, diag_j in ops.col_bands(n, step, diag_offset):
                partials, _ = ops.sigmoid_ids(
                    zimg, ztxt[j0:j1], t_prime, bias, img_ids,
                    txt_ids[j0:j1], duplicates, diag_j, want_g=False)
                # the same reduction as saved-g: one block gives the same bits
                loss = loss + partials.double().sum(dim=0)[0]
            ctx.save_for_backward(zimg, ztxt, t_prime, bias, img_ids,
                                  txt_ids)
            ctx.step = step
        ctx.save_g = save_g
        ctx.duplicates, ctx.diag_offset = duplicates, diag_offset
        return loss.float()

    @staticmethod
    def backward(ctx, grad_output):
        zimg, ztxt, t_prime, bias, img_ids, txt_ids = ctx.saved_tensors[:6]
        n, dev = ztxt.shape[0], zimg.device
        go = ops._go_scalar(grad_output, dev)
        t = ops._prep_scalar(t_prime, dev).exp()
        if ctx.save_g:
            sums, g = ctx.saved_tensors[6:]
            # bf16_scale=True: the products stay bf16 (see ops.grad_gemms).
            dzimg, dztxt = ops.grad_gemms(ops.GBand(g, None, ztxt), zimg, n,
                                          go * t, bf16_scale=True)
        else:
            parts = []

            def emit(j0, j1, diag_j, g, gt):
                partials, _ = ops.sigmoid_ids(
                    zimg, ztxt[j0:j1], t_prime, bias, img_ids,
                    txt_ids[j0:j1], ctx.duplicates, diag_j, g=g)
                parts.append(partials.double().sum(dim=0))

            # bf16_scale stays False, also when one band covers the block.
            dzimg, dztxt = ops.band_grad_gemms(
                zimg, ztxt, ctx.step, emit, go * t,
                diag_offset=ctx.diag_offset)
            sums = torch.stack(parts).sum(dim=0)
        dt = sums[1] * (go * t).double()
        db = sums[2] * go.double()
        return (dzimg, dztxt,
                dt.to(device=t_prime.device,
                      dtype=t_prime.dtype).reshape(t_prime.shape),
                db.to(device=bias.device, dtype=bias.dtype).reshape(bias.shape),
                None, None, None, None, None, None)


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
                                 impl: str = "auto") -> torch.Tensor:
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

    Returns a 0-d tensor; the caller normalises.
    """
    if zimg.dim() != 2 or ztxt.dim() != 2 or zimg.shape[1] != ztxt.shape[1]:
        raise ValueError(
            f"shape mismatch: zimg {tuple(zimg.shape)} ztxt {tuple(ztxt.shape)}")
    if duplicates not in _DUPLICATES:
        raise ValueError(f"unknown duplicates {duplicates!r}")
    if impl == "auto":
        impl = ("hip" if zimg.is_cuda and zimg.dtype == torch.bfloat16
                and ztxt.dtype == torch.bfloat16 else "torch")
    if impl not in ("hip", "torch"):
        raise ValueError(f"unknown impl {impl!r}")
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
                              duplicates, diag_offset, col_chunk, want_grad)
