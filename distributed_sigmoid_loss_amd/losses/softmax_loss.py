"""Softmax (InfoNCE / CLIP) contrastive loss over the image×text pair grid.

The baseline the sigmoid loss is defined against, with the same contract as
``sigmoid_contrastive_loss``: a ``(b, n)`` block ``zimg (b, d)`` × ``ztxt
(n, d)`` whose logits never reach memory on the GPU path.

    z_ij      = t · <zimg_i, ztxt_j>,   t = exp(t_prime)      (no bias: it
                                                 cancels in a softmax)
    row_lse_i = log Σ_j exp(z_ij)       col_lse_j = log Σ_i exp(z_ij)
    total     = Σ_{i with a positive} (row_lse_i − z_{i,pos})
              + Σ_{j with a positive} (col_lse_j − z_{pos,j})

The positive of row ``i`` is column ``i + diag_offset``, the positive of
column ``j`` is row ``j − diag_offset``; a row or column whose positive lies
outside the block contributes nothing.  ``total`` is in sum form — the
caller normalises (``total / (2 b)`` is the symmetric CLIP loss).

Backward, with upstream weights ``row_w (b,)`` and ``col_w (n,)`` (zero
where there is no positive):

    g_ij  = row_w_i·exp(z_ij − row_lse_i) + col_w_j·exp(z_ij − col_lse_j)
            − [j == i + diag_offset]·(row_w_i + col_w_j)
    dzimg = t · g @ ztxt     dztxt = t · gᵀ @ zimg     dt' = t · Σ g_ij·s_ij

with ``s = z / t``.  Forward keeps the inputs and the two LSE vectors —
``O(b + n)``; backward recomputes the logits tile by tile and emits ``g`` as
a bf16 slab (whole, or per column band) for the two gradient GEMMs.

On GPU both passes are HIP kernels (``ops.pair_lse``, ``ops.softmax_g``);
elsewhere a row-chunked torch composite with the same contract runs (fp32
compute, fp64 for fp64 inputs) — the CPU path and the tests' reference.

Distributed (``group``): the one-grid form.  This rank holds ``b`` image
rows and all ``n = W·b`` text columns (``diag_offset = rank·b``).  Row LSEs
are complete locally; column LSEs are all-gathered and folded, identical on
every rank.  A rank's ``total`` counts its rows and the columns whose
positive row it holds.  In backward the ranks' ``grad_output`` scalars are
all-gathered: ``row_w = go_rank`` and ``col_w_j = go_owner(j)``, because
``col_lse_j`` belongs to its owner's loss — the exact gradient of
``Σ_q go_q·loss_q`` for unequal ``go_q`` too.

Sample-ID labels (``softmax_contrastive_loss_ids``): the positives come from
two int64 id vectors, as in ``losses/id_labels.py`` — any number per row or
column, pairs that count for nothing, padding rows outside every normaliser.
The contract stands above its code below; on GPU it runs on
``ops.pair_lse_ids`` and ``ops.softmax_g_ids``, which add each row's and
column's positive-logit sum and positive count to the LSE pass.
"""

from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn
import torch.distributed as dist

from .. import ops
from ..parallel.collectives import all_gather_with_grad
from .id_labels import _DUPLICATES, _ids_vector, pair_classes
from .retrieval import (
    _TORCH_ROW_CHUNK,
    _compute_dtype,
    _positive_rows,
    positive_scores,
)


def _torch_pair_lse(zimg, ztxt, t_prime, rows=True, cols=True,
                    row_chunk=_TORCH_ROW_CHUNK):
    """``ops.pair_lse`` as a row-chunked torch composite: holds
    ``O(row_chunk · n)`` logits at a time."""
    b, n = zimg.shape[0], ztxt.shape[0]
    dev, cdt = zimg.device, _compute_dtype(zimg)
    t = t_prime.detach().to(device=dev, dtype=cdt).exp()
    zt = ztxt.detach().to(cdt)
    row_lse = torch.empty(b, device=dev, dtype=cdt) if rows else None
    col_lse = (torch.full((n,), -math.inf, device=dev, dtype=cdt)
               if cols else None)
    for r0 in range(0, b, row_chunk):
        r1 = min(b, r0 + row_chunk)
        z = (zimg[r0:r1].detach().to(cdt) @ zt.T) * t
        if rows:
            row_lse[r0:r1] = torch.logsumexp(z, dim=1)
        if cols:
            col_lse = torch.logaddexp(col_lse, torch.logsumexp(z, dim=0))
    return row_lse, col_lse


def _torch_softmax_g(zimg, ztxt, t_prime, row_lse, row_w, col_lse, col_w,
                     diag_offset, g=None, row_chunk=_TORCH_ROW_CHUNK):
    """``ops.softmax_g`` as a row-chunked torch composite; ``g`` is in the
    compute dtype and ``gs_partials`` has one entry."""
    b, n = zimg.shape[0], ztxt.shape[0]
    dev, cdt = zimg.device, _compute_dtype(zimg)
    t = t_prime.detach().to(device=dev, dtype=cdt).exp()
    zt = ztxt.detach().to(cdt)
    if g is None:
        g = torch.empty((b, n), device=dev, dtype=cdt)
    gs = torch.zeros((), device=dev, dtype=torch.float64)
    cols = torch.arange(n, device=dev)
    for r0 in range(0, b, row_chunk):
        r1 = min(b, r0 + row_chunk)
        s = zimg[r0:r1].detach().to(cdt) @ zt.T
        z = s * t
        gv = torch.zeros_like(z)
        w = torch.zeros_like(z)
        if row_lse is not None:
            gv += row_w[r0:r1, None] * torch.exp(z - row_lse[r0:r1, None])
            w += row_w[r0:r1, None]
        if col_lse is not None:
            gv += col_w[None, :] * torch.exp(z - col_lse[None, :])
            w += col_w[None, :]
        if diag_offset is not None:
            pos = torch.arange(r0, r1, device=dev) + int(diag_offset)
            gv -= w * (cols[None, :] == pos[:, None])
        g[r0:r1] = gv
        gs += (gv * s).double().sum()
    return g, gs.reshape(1)


def _is_distributed(group) -> bool:
    return (group is not None and dist.is_available()
            and dist.is_initialized() and dist.get_world_size(group) > 1)


def _fwd_step(col_chunk, n: int) -> int:
    """Columns per forward pass (and per torch-path backward band)."""
    return int(col_chunk) if col_chunk and col_chunk > 0 else n


def _owner_go(go, b: int, group):
    """Under a group column j's term is part of the loss of the rank that
    holds row j − diag_offset, i.e. rank j // b: the ranks' ``grad_output``
    scalars, gathered, as an ``(n,)`` vector."""
    go_all = torch.empty(dist.get_world_size(group), device=go.device,
                         dtype=go.dtype)
    dist.all_gather_into_tensor(go_all, go.reshape(1), group=group)
    return go_all.repeat_interleave(b)


def _backward(hip, zimg, ztxt, t_prime, t, col_chunk, diag_offset, g_band,
              gs_parts, n_inputs):
    """What the two Functions' backwards share.  ``g_band(j0, j1, diag_j, g,
    gt)`` returns dL/dlogit of columns ``j0:j1`` — written into ``g`` where
    one is handed (the hip path) — and appends the band's ``Σ g·s`` partials
    to ``gs_parts``.  Returns the ``n_inputs`` gradients: dzimg, dztxt, dt'
    and ``None`` for the rest."""
    b, n = zimg.shape[0], ztxt.shape[0]
    if hip:
        # The upstream gradient lives in the weights: the scale is t alone.
        dzimg, dztxt = ops.band_grad_gemms(
            zimg, ztxt, ops.g_band_step(b, n, col_chunk), g_band, t,
            diag_offset=diag_offset)
    else:
        cdt = t.dtype
        zi = zimg.to(cdt)
        dzimg = torch.zeros((b, zimg.shape[1]), device=t.device, dtype=cdt)
        dztxt = torch.empty((n, zimg.shape[1]), device=t.device, dtype=cdt)
        for j0, j1, diag_j in ops.col_bands(n, _fwd_step(col_chunk, n),
                                            diag_offset):
            g = g_band(j0, j1, diag_j, None, None)
            dzimg += g @ ztxt[j0:j1].to(cdt)
            dztxt[j0:j1] = g.T @ zi
        dzimg, dztxt = (dzimg * t).to(zimg.dtype), (dztxt * t).to(ztxt.dtype)
    dt = t.double() * torch.cat(gs_parts).double().sum()
    return (dzimg, dztxt,
            dt.to(device=t_prime.device,
                  dtype=t_prime.dtype).reshape(t_prime.shape)
            ) + (None,) * (n_inputs - 3)


def _check_block(zimg, ztxt, impl: str, group, hip_auto: bool,
                 duplicates: str = "positive"):
    """What the public functions check alike → ``(impl, group, world,
    rank)``: the shapes, ``duplicates``, ``impl`` resolved (``auto`` is
    ``hip`` given ``hip_auto``), ``group`` as ``None`` unless it spans several
    ranks."""
    if zimg.dim() != 2 or ztxt.dim() != 2 or zimg.shape[1] != ztxt.shape[1]:
        raise ValueError(
            f"shape mismatch: zimg {tuple(zimg.shape)} ztxt {tuple(ztxt.shape)}")
    if duplicates not in _DUPLICATES:
        raise ValueError(f"unknown duplicates {duplicates!r}")
    if impl == "auto":
        impl = "hip" if hip_auto else "torch"
    if impl not in ("hip", "torch"):
        raise ValueError(f"unknown impl {impl!r}")
    if not _is_distributed(group):
        return impl, None, 1, 0
    return impl, group, dist.get_world_size(group), dist.get_rank(group)


class _SoftmaxLoss(torch.autograd.Function):
    """Both implementations: ``hip`` runs the fused kernels and the library
    gradient GEMMs, ``torch`` the composites above; the chunking, the
    collectives and the weights are shared."""

    @staticmethod
    def forward(ctx, zimg, ztxt, t_prime, diag_offset, col_chunk, impl,
                group):
        hip = impl == "hip"
        lse_fn = ops.pair_lse if hip else _torch_pair_lse
        zimg, ztxt = zimg.contiguous(), ztxt.contiguous()
        b, n = zimg.shape[0], ztxt.shape[0]
        row_lse, col_parts = None, []
        for j0, j1, _ in ops.col_bands(n, _fwd_step(col_chunk, n)):
            rl, cl = lse_fn(zimg, ztxt[j0:j1], t_prime)
            row_lse = rl if row_lse is None else torch.logaddexp(row_lse, rl)
            col_parts.append(cl)
        col_lse = col_parts[0] if len(col_parts) == 1 else torch.cat(col_parts)
        if group is not None:
            # This rank's rows are a share of every column: gather the
            # shares and fold them in rank order, the same on every rank.
            shares = torch.empty(dist.get_world_size(group) * n,
                                 device=col_lse.device, dtype=col_lse.dtype)
            dist.all_gather_into_tensor(shares, col_lse.contiguous(),
                                        group=group)
            col_lse = torch.logsumexp(shares.view(-1, n), dim=0)
        rows, cols = _positive_rows(b, n, diag_offset, zimg.device)
        t = t_prime.detach().to(device=zimg.device, dtype=row_lse.dtype).exp()
        z_pos = positive_scores(zimg, ztxt, diag_offset)[rows] * t
        total = (row_lse[rows].double() + col_lse[cols].double()
                 - 2.0 * z_pos.double()).sum().to(row_lse.dtype)
        ctx.save_for_backward(zimg, ztxt, t_prime, row_lse, col_lse)
        ctx.diag_offset, ctx.col_chunk = diag_offset, col_chunk
        ctx.hip, ctx.group = hip, group
        return total

    @staticmethod
    def backward(ctx, grad_output):
        zimg, ztxt, t_prime, row_lse, col_lse = ctx.saved_tensors
        b, n = zimg.shape[0], ztxt.shape[0]
        dev, cdt = zimg.device, row_lse.dtype
        go = ops._go_scalar(grad_output, dev, cdt)
        rows, cols = _positive_rows(b, n, ctx.diag_offset, dev)
        row_w = torch.zeros(b, device=dev, dtype=cdt)
        row_w[rows] = go
        if ctx.group is not None:
            col_w = _owner_go(go, b, ctx.group)
        else:
            col_w = torch.zeros(n, device=dev, dtype=cdt)
            col_w[cols] = go
        t = t_prime.detach().to(device=dev, dtype=cdt).exp()
        g_fn = ops.softmax_g if ctx.hip else _torch_softmax_g
        gs_parts = []

        def g_band(j0, j1, diag_j, g, gt):
            g, gs = g_fn(zimg, ztxt[j0:j1], t_prime, row_lse, row_w,
                         col_lse[j0:j1].contiguous(),
                         col_w[j0:j1].contiguous(), diag_j, g=g)
            gs_parts.append(gs)
            return g

        return _backward(ctx.hip, zimg, ztxt, t_prime, t, ctx.col_chunk,
                         ctx.diag_offset, g_band, gs_parts, 7)


def softmax_contrastive_loss(zimg: torch.Tensor, ztxt: torch.Tensor,
                             t_prime: torch.Tensor,
                             diag_offset: Optional[int] = 0,
                             col_chunk: Optional[int] = None,
                             impl: str = "auto", group=None) -> torch.Tensor:
    """Sum-form softmax contrastive loss of the ``(b, n)`` block: the
    cross-entropy of every row that has a positive plus that of every column
    that has one (see the module docstring).  Differentiable in ``zimg``,
    ``ztxt`` and ``t_prime``.

    Args:
        zimg: ``(b, d)`` image embeddings (L2-normalized by the caller).
        ztxt: ``(n, d)`` text embeddings.
        t_prime: scalar; the temperature is ``exp(t_prime)``.
        diag_offset: column of row 0's positive; ``None``: no positives.
        col_chunk: columns per kernel pass (forward LSE and backward g
            band), bounding the workspace to ``O(b · col_chunk)``; ``None``:
            the whole block, banded in backward only when the bf16 g slab
            would reach 2³² bytes.
        impl: ``auto`` (``hip`` on GPU, ``torch`` elsewhere) | ``hip`` (bf16,
            ``d % 8 == 0``; raises without the built extension) | ``torch``.
        group: a process group of ``W > 1`` ranks for the one-grid
            distributed form (``n == W·b``, ``diag_offset == rank·b``);
            ``None``: this block alone.

    Returns a 0-d tensor; the caller normalises.
    """
    impl, group, world, rank = _check_block(zimg, ztxt, impl, group,
                                            zimg.is_cuda)
    b = zimg.shape[0]
    if group is not None and (ztxt.shape[0] != world * b
                              or diag_offset != rank * b):
        raise ValueError(
            f"the distributed form needs n == W·b and diag_offset == "
            f"rank·b (got b={b}, n={ztxt.shape[0]}, W={world}, "
            f"rank={rank}, diag_offset={diag_offset})")
    return _SoftmaxLoss.apply(zimg, ztxt, t_prime, diag_offset, col_chunk,
                              impl, group)


# ---------------------------------------------------------------------------
# Sample-ID labels: multi-positive InfoNCE
# ---------------------------------------------------------------------------
#
# Pair classes are those of ``id_labels.pair_classes`` (masked where an id is
# negative; ``"positive"``: equal ids are positives; ``"ignore"``: the
# position is the positive and other equal-id pairs are masked); a masked pair
# is never a positive.  With P_i the unmasked positives of row i and Q_j those
# of column j:
#
#     row_lse_i = log Σ_{j not masked} exp(z_ij)   (−inf: fully masked row)
#     total = Σ_{i: |P_i|>0} (row_lse_i − (1/|P_i|)·Σ_{p∈P_i} z_ip)
#           + Σ_{j: |Q_j|>0} (col_lse_j − (1/|Q_j|)·Σ_{q∈Q_j} z_qj)
#     g_ij = 0 where masked, otherwise
#            row_w_i·exp(z_ij − row_lse_i) + col_w_j·exp(z_ij − col_lse_j)
#            − [positive]·(row_pw_i + col_pw_j)
#     row_w_i = upstream weight if |P_i| > 0 else 0,  row_pw_i = row_w_i/|P_i|
#
# — the mean over positives of −log softmax in both directions.  A masked
# pair is out of both normalisers; an unmasked row without a positive has no
# term of its own but still sits in the column normalisers.


def _torch_pair_lse_ids(zimg, ztxt, t_prime, img_ids, txt_ids,
                        duplicates="positive", diag_offset=None, rows=True,
                        cols=True, row_chunk=_TORCH_ROW_CHUNK):
    """``ops.pair_lse_ids`` as a row-chunked torch composite: holds
    ``O(row_chunk · n)`` logits at a time."""
    b, n = zimg.shape[0], ztxt.shape[0]
    dev, cdt = zimg.device, _compute_dtype(zimg)
    t = t_prime.detach().to(device=dev, dtype=cdt).exp()
    zt = ztxt.detach().to(cdt)
    row_lse = torch.empty(b, device=dev, dtype=cdt)
    row_pos = torch.empty(b, device=dev, dtype=cdt)
    row_cnt = torch.empty(b, device=dev, dtype=torch.int32)
    col_lse = torch.full((n,), -math.inf, device=dev, dtype=cdt)
    col_pos = torch.zeros(n, device=dev, dtype=cdt)
    col_cnt = torch.zeros(n, device=dev, dtype=torch.int32)
    for r0 in range(0, b, row_chunk):
        r1 = min(b, r0 + row_chunk)
        z = (zimg[r0:r1].detach().to(cdt) @ zt.T) * t
        pos, masked = pair_classes(
            img_ids[r0:r1], txt_ids, duplicates,
            None if diag_offset is None else int(diag_offset) + r0)
        pos = pos & ~masked
        zm = z.masked_fill(masked, -math.inf)
        zp = torch.where(pos, z, torch.zeros_like(z))
        row_lse[r0:r1] = torch.logsumexp(zm, dim=1)
        row_pos[r0:r1] = zp.sum(dim=1)
        row_cnt[r0:r1] = pos.sum(dim=1)
        col_lse = torch.logaddexp(col_lse, torch.logsumexp(zm, dim=0))
        col_pos += zp.sum(dim=0)
        col_cnt += pos.sum(dim=0).to(torch.int32)
    return ((row_lse, row_pos, row_cnt) if rows else (None,) * 3) + (
        (col_lse, col_pos, col_cnt) if cols else (None,) * 3)


def _torch_softmax_g_ids(zimg, ztxt, t_prime, img_ids, txt_ids, duplicates,
                         diag_offset, row_lse, row_w, row_pw, col_lse, col_w,
                         col_pw, g=None, row_chunk=_TORCH_ROW_CHUNK):
    """``ops.softmax_g_ids`` as a row-chunked torch composite; ``g`` is in
    the compute dtype and ``gs_partials`` has one entry."""
    b, n = zimg.shape[0], ztxt.shape[0]
    dev, cdt = zimg.device, _compute_dtype(zimg)
    t = t_prime.detach().to(device=dev, dtype=cdt).exp()
    zt = ztxt.detach().to(cdt)
    if g is None:
        g = torch.empty((b, n), device=dev, dtype=cdt)
    gs = torch.zeros((), device=dev, dtype=torch.float64)
    for r0 in range(0, b, row_chunk):
        r1 = min(b, r0 + row_chunk)
        s = zimg[r0:r1].detach().to(cdt) @ zt.T
        z = s * t
        pos, masked = pair_classes(
            img_ids[r0:r1], txt_ids, duplicates,
            None if diag_offset is None else int(diag_offset) + r0)
        gv = torch.zeros_like(z)
        pw = torch.zeros_like(z)
        if row_lse is not None:
            gv += row_w[r0:r1, None] * torch.exp(z - row_lse[r0:r1, None])
            pw += row_pw[r0:r1, None]
        if col_lse is not None:
            gv += col_w[None, :] * torch.exp(z - col_lse[None, :])
            pw += col_pw[None, :]
        gv -= pw * pos
        # A select: a fully masked row or column has lse = −inf and gv is
        # 0 · inf there.
        gv = torch.where(masked, torch.zeros_like(gv), gv)
        g[r0:r1] = gv
        gs += (gv * s).double().sum()
    return g, gs.reshape(1)


def _mean_positive_terms(lse, pos, cnt):
    """``lse − pos / cnt`` where there is a positive, 0 elsewhere (fp64)."""
    has = cnt > 0
    mean = pos.double() / cnt.clamp(min=1).double()
    return torch.where(has, lse.double() - mean, torch.zeros_like(mean))


def _id_weights(go, cnt, dtype):
    """``(w, pw)`` of one side: the upstream weight where there is a positive
    (0 elsewhere) and that weight over the number of positives."""
    w = torch.where(cnt > 0, go.to(dtype), torch.zeros((), device=cnt.device,
                                                       dtype=dtype))
    return w.contiguous(), (w / cnt.clamp(min=1).to(dtype)).contiguous()


class _SoftmaxIdLoss(torch.autograd.Function):
    """Both implementations of the sample-ID softmax loss, in the shape of
    :class:`_SoftmaxLoss`: ``hip`` runs the fused kernels and the library
    gradient GEMMs, ``torch`` the composites above; the chunking, the
    collectives and the weights are shared."""

    @staticmethod
    def forward(ctx, zimg, ztxt, t_prime, img_ids, txt_ids, duplicates,
                diag_offset, col_chunk, impl, group):
        hip = impl == "hip"
        lse_fn = ops.pair_lse_ids if hip else _torch_pair_lse_ids
        zimg, ztxt = zimg.contiguous(), ztxt.contiguous()
        b, n = zimg.shape[0], ztxt.shape[0]
        row_lse = row_pos = row_cnt = None
        col_parts = []
        for j0, j1, diag_j in ops.col_bands(n, _fwd_step(col_chunk, n),
                                            diag_offset):
            rl, rp, rc, cl, cp, cc = lse_fn(
                zimg, ztxt[j0:j1], t_prime, img_ids, txt_ids[j0:j1],
                duplicates, diag_j)
            if row_lse is None:
                row_lse, row_pos, row_cnt = rl, rp, rc
            else:
                row_lse = torch.logaddexp(row_lse, rl)
                row_pos, row_cnt = row_pos + rp, row_cnt + rc
            col_parts.append((cl, cp, cc))
        col_lse, col_pos, col_cnt = (
            col_parts[0] if len(col_parts) == 1
            else tuple(torch.cat(v) for v in zip(*col_parts)))
        own = slice(0, n)
        if group is not None:
            # This rank's rows are a share of every column: gather the
            # shares, fold the LSEs and add the sums and counts in rank
            # order, the same on every rank.
            world, rank = dist.get_world_size(group), dist.get_rank(group)
            mine = torch.cat((col_lse, col_pos))
            shares = torch.empty(world * 2 * n, device=mine.device,
                                 dtype=mine.dtype)
            dist.all_gather_into_tensor(shares, mine, group=group)
            shares = shares.view(world, 2, n)
            cnts = torch.empty(world * n, device=col_cnt.device,
                               dtype=col_cnt.dtype)
            dist.all_gather_into_tensor(cnts, col_cnt.contiguous(),
                                        group=group)
            cnts = cnts.view(world, n)
            col_lse = torch.logsumexp(shares[:, 0], dim=0)
            col_pos, col_cnt = shares[0, 1], cnts[0]
            for q in range(1, world):
                col_pos, col_cnt = col_pos + shares[q, 1], col_cnt + cnts[q]
            # Column j belongs to the loss of rank j // b, its text's owner.
            own = slice(rank * b, (rank + 1) * b)
        total = (_mean_positive_terms(row_lse, row_pos, row_cnt).sum()
                 + _mean_positive_terms(col_lse[own], col_pos[own],
                                        col_cnt[own]).sum()).to(row_lse.dtype)
        ctx.save_for_backward(zimg, ztxt, t_prime, img_ids, txt_ids, row_lse,
                              row_cnt, col_lse.contiguous(),
                              col_cnt.contiguous())
        ctx.duplicates, ctx.diag_offset = duplicates, diag_offset
        ctx.col_chunk, ctx.hip, ctx.group = col_chunk, hip, group
        return total

    @staticmethod
    def backward(ctx, grad_output):
        (zimg, ztxt, t_prime, img_ids, txt_ids, row_lse, row_cnt, col_lse,
         col_cnt) = ctx.saved_tensors
        b = zimg.shape[0]
        dev, cdt = zimg.device, row_lse.dtype
        go = ops._go_scalar(grad_output, dev, cdt)
        col_go = go if ctx.group is None else _owner_go(go, b, ctx.group)
        row_w, row_pw = _id_weights(go, row_cnt, cdt)
        col_w, col_pw = _id_weights(col_go, col_cnt, cdt)
        t = t_prime.detach().to(device=dev, dtype=cdt).exp()
        g_fn = ops.softmax_g_ids if ctx.hip else _torch_softmax_g_ids
        gs_parts = []

        def g_band(j0, j1, diag_j, g, gt):
            g, gs = g_fn(
                zimg, ztxt[j0:j1], t_prime, img_ids, txt_ids[j0:j1],
                ctx.duplicates, diag_j, row_lse, row_w, row_pw,
                col_lse[j0:j1].contiguous(), col_w[j0:j1].contiguous(),
                col_pw[j0:j1].contiguous(), g=g)
            gs_parts.append(gs)
            return g

        return _backward(ctx.hip, zimg, ztxt, t_prime, t, ctx.col_chunk,
                         ctx.diag_offset, g_band, gs_parts, 10)


def softmax_contrastive_loss_ids(zimg: torch.Tensor, ztxt: torch.Tensor,
                                 t_prime: torch.Tensor,
                                 img_ids: torch.Tensor, txt_ids: torch.Tensor,
                                 duplicates: str = "positive",
                                 diag_offset: Optional[int] = None,
                                 col_chunk: Optional[int] = None,
                                 impl: str = "auto",
                                 group=None) -> torch.Tensor:
    """Sum-form softmax contrastive loss of the ``(b, n)`` block with the
    labels taken from sample ids: for every row and every column that has a
    positive, the mean over its positives of ``−log softmax`` (multi-positive
    InfoNCE — the SupCon "outside" form, UniCL's bidirectional loss).
    Differentiable in ``zimg``, ``ztxt`` and ``t_prime``.

    A pair is masked where ``img_ids[i] < 0`` or ``txt_ids[j] < 0`` and is
    then out of both normalisers; ``duplicates="positive"`` makes a pair
    positive where the ids are equal; ``"ignore"`` keeps ``j == i +
    diag_offset`` as the only positive and masks every other pair with equal
    ids (false-negative removal).  A row or column without a positive adds no
    term of its own but stays in the normalisers of the other direction.  With
    ``img_ids = arange(b) + diag``, ``txt_ids = arange(n)`` and
    ``"positive"`` this is ``softmax_contrastive_loss(diag_offset=diag)``.

    Args:
        zimg: ``(b, d)`` image embeddings (L2-normalized by the caller).
        ztxt: ``(n, d)`` text embeddings.
        t_prime: scalar; the temperature is ``exp(t_prime)``.
        img_ids, txt_ids: integer ``(b,)`` / ``(n,)`` sample ids, compared as
            64-bit values; a negative id masks the whole row / column.
        duplicates: ``"positive"`` | ``"ignore"``.
        diag_offset: column of row 0's positional positive, used only with
            ``"ignore"``; ``None``: no positional positive.
        col_chunk: columns per kernel pass (forward and backward g band),
            bounding the workspace to ``O(b · col_chunk)``; ``None``: the
            whole block, banded in backward only when the bf16 g slab would
            reach 2³² bytes.
        impl: ``auto`` (``hip`` on GPU for bf16, ``torch`` elsewhere) |
            ``hip`` (bf16 on GPU, ``d % 8 == 0``; raises without the built
            extension) | ``torch``.
        group: a process group of ``W > 1`` ranks for the one-grid
            distributed form (``n == W·b``; with ``"ignore"``,
            ``diag_offset == rank·b``): column ``j`` counts for the loss of
            rank ``j // b``; ``None``: this block alone.

    Returns a 0-d tensor; the caller normalises.
    """
    impl, group, world, rank = _check_block(
        zimg, ztxt, impl, group,
        zimg.is_cuda and zimg.dtype == torch.bfloat16
        and ztxt.dtype == torch.bfloat16, duplicates)
    b = zimg.shape[0]
    img_ids = _ids_vector("img_ids", img_ids, b, zimg.device)
    txt_ids = _ids_vector("txt_ids", txt_ids, ztxt.shape[0], zimg.device)
    if duplicates != "ignore":
        diag_offset = None
    if group is not None and (ztxt.shape[0] != world * b
                              or (duplicates == "ignore"
                                  and diag_offset != rank * b)):
        raise ValueError(
            f"the distributed form needs n == W·b and, with "
            f"duplicates='ignore', diag_offset == rank·b (got b={b}, "
            f"n={ztxt.shape[0]}, W={world}, rank={rank}, "
            f"diag_offset={diag_offset})")
    return _SoftmaxIdLoss.apply(zimg, ztxt, t_prime, img_ids, txt_ids,
                                duplicates, diag_offset, col_chunk, impl,
                                group)


class DistributedSoftmaxLoss(nn.Module):
    """All-rank softmax (CLIP) contrastive loss with a module-owned,
    learnable ``t_prime`` (init ``log(1 / init_temperature)``; the forward
    clamps it at ``log(max_logit_scale)``, as CLIP does).

    ``forward`` takes the *local* image and text shards ``(b, d)``,
    all-gathers the text shard (``all_gather_with_grad``: reduce-scatter in
    backward), evaluates the ``(b, W·b)`` grid with ``diag_offset = rank·b``
    and returns ``total / (2·gpu_batch_size)``.  At ``W = 1`` that is the
    symmetric CLIP loss ``(CE(z) + CE(zᵀ)) / 2``; under DDP gradient
    averaging ``W`` ranks reproduce the single-rank gradients of the global
    batch.

    Sample-ID labels: ``forward(..., image_ids=, text_ids=)`` (both or
    neither) takes the positives from the ids of the local shards instead of
    the position — several captions per image, repeated samples
    (``duplicates="positive"``), false-negative removal with the position as
    the only positive (``"ignore"``), padding rows (a negative id); see
    :func:`softmax_contrastive_loss_ids`.  The text ids are all-gathered
    along with the text shard; the result is still divided by
    ``2·gpu_batch_size``, not by the number of active rows.
    """

    def __init__(self, gpu_batch_size: int, col_chunk: Optional[int] = None,
                 impl: str = "auto", init_temperature: float = 0.07,
                 max_logit_scale: float = 100.0):
        super().__init__()
        self.t_prime = nn.Parameter(
            torch.tensor(math.log(1.0 / init_temperature)))
        self.gpu_batch_size = gpu_batch_size
        self.col_chunk = col_chunk
        self.impl = impl
        self.max_logit_scale = max_logit_scale

    def _gather_text(self, text_embeddings, group):
        """What both label forms start with → ``(world, rank, t', all text
        shards, the group to reduce over or None at one rank)``."""
        world, rank = 1, 0
        if dist.is_available() and dist.is_initialized():
            world, rank = dist.get_world_size(group), dist.get_rank(group)
        t_prime = self.t_prime.clamp(max=math.log(self.max_logit_scale))
        all_txt = all_gather_with_grad(text_embeddings, group=group)
        if world > 1 and group is None:
            group = dist.group.WORLD
        return world, rank, t_prime, all_txt, group if world > 1 else None

    def _forward_ids(self, image_embeddings, text_embeddings, group,
                     image_ids, text_ids, duplicates):
        b_txt = text_embeddings.shape[0]
        text_ids = _ids_vector("text_ids", text_ids, b_txt,
                               text_embeddings.device)
        world, rank, t_prime, all_txt, group = self._gather_text(
            text_embeddings, group)
        all_ids = text_ids
        if group is not None:
            all_ids = torch.empty(world * b_txt, device=text_ids.device,
                                  dtype=torch.int64)
            dist.all_gather_into_tensor(all_ids, text_ids, group=group)
        total = softmax_contrastive_loss_ids(
            image_embeddings, all_txt, t_prime, image_ids, all_ids,
            duplicates=duplicates, diag_offset=rank * b_txt,
            col_chunk=self.col_chunk, impl=self.impl, group=group)
        return total / (2 * self.gpu_batch_size)

    def forward(self, image_embeddings: torch.Tensor,
                text_embeddings: torch.Tensor, group=None,
                image_ids: Optional[torch.Tensor] = None,
                text_ids: Optional[torch.Tensor] = None,
                duplicates: str = "positive") -> torch.Tensor:
        if (image_ids is None) != (text_ids is None):
            raise ValueError(
                "image_ids and text_ids must be given together")
        if image_ids is not None:
            return self._forward_ids(image_embeddings, text_embeddings,
                                     group, image_ids, text_ids, duplicates)
        _, rank, t_prime, all_txt, group = self._gather_text(
            text_embeddings, group)
        total = softmax_contrastive_loss(
            image_embeddings, all_txt, t_prime,
            diag_offset=rank * text_embeddings.shape[0],
            col_chunk=self.col_chunk, impl=self.impl, group=group)
        return total / (2 * self.gpu_batch_size)
