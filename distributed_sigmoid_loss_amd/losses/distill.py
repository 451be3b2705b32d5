"""Sigmoid distillation loss: soft targets from a teacher dual encoder.

Every other loss of the package takes hard labels.  The usual recipe for
training a small image–text model with a sigmoid loss is distillation from a
larger dual encoder: the teacher's own pair grid is the soft target of every
student pair, usually mixed with the hard positional label.  The teacher
embeddings come per sample — ``timg (b, d_T)``, ``ttxt (n, d_T)`` — so the
target grid is a second ``(b, n)`` matrix of dot products, and like the
student's it is never built here.

One contract for every implementation.  With ``t = exp(t_prime)`` and
``t_T = exp(teacher_t_prime)``:

    s_ij = <zimg_i, ztxt_j>          z_ij = t·s_ij + bias
    p_ij = σ(t_T·<timg_i, ttxt_j> + teacher_bias)
    q_ij = alpha·p_ij + (1 − alpha)·[j == i + diag_offset]
    total = Σ_ij softplus(z_ij) − q_ij·z_ij
    g_ij  = σ(z_ij) − q_ij
    dzimg = t·g@ztxt   dztxt = t·gᵀ@zimg   dt' = t·Σ g_ij·s_ij   dbias = Σ g_ij

``total`` is the binary cross-entropy of ``σ(z)`` against the target ``q`` in
sum form; the caller normalises.  It is linear in the target, so the mixed
objective costs one student pass, not two.  ``alpha = 0`` is
``sigmoid_contrastive_loss(diag_offset=…)``; ``alpha = 1`` is pure
distillation, minimal where the student's pair probabilities equal the
teacher's; ``diag_offset=None`` leaves out the hard positive.  The teacher
side gets no gradient: its embeddings and scalars are detached.

On GPU (all four embeddings bf16) the fused kernel ``ops.sigmoid_distill``
runs the teacher's and the student's K loops back to back on each 128×128
tile and keeps the targets in registers, in the two regimes of the sample-ID
loss:

- *saved-g* — gradients wanted, ``col_chunk is None`` and the bf16 g slab
  below 2³² bytes: the forward emits the loss partials and the dL/dlogit slab
  in one pass; the backward is the two gradient GEMMs (``ops.grad_gemms``)
  plus the scalar gradients from the saved partials.
- *band recompute* — otherwise: the forward runs the loss-only kernel per
  column band (``ztxt`` and ``ttxt`` sliced by the same rows); the backward
  re-runs the kernel per band through ``ops.band_grad_gemms``.

Per-tile partials are summed in fp64 on the device; nothing syncs with the
host.  Elsewhere a differentiable torch composite with the same contract runs
(fp32 compute, fp64 for fp64 inputs) — the CPU path and the tests' reference.

The softmax / KL form (``softmax_distillation_loss``) pulls the student's row
and column softmax over the batch towards the teacher's — the affinity
mimicking of TinyCLIP, CLIP-KD's contrastive relational distillation — mixed
with the hard InfoNCE label; its contract stands above its code below.

MXFP8 teacher (``teacher_quant="mxfp8"``, both losses and both modules).  The
teacher gets no gradient and enters no gradient GEMM, so it may be read — and
stored — as OCP MXFP8: e4m3 elements with one power-of-two scale per 32
consecutive elements (``ops.quantize_mx``; ``d_T % 32 == 0``).  ``timg`` and
``ttxt`` are then each a tensor, quantised once per call, or a stored ``(q,
e8)`` pair, of which no bf16 copy is made on the ``hip`` path: the kernels run
the teacher's K loop on the MX-scaled MFMA (``ops.sigmoid_distill_mx``,
``ops.pair_distill_stats_mx``, ``ops.softmax_distill_g_mx``), a band slices
``q`` and ``e8`` by the rows of ``ztxt``, and the modules gather the teacher
text shard as two ``uint8`` tensors, half the bytes.  The contract above holds
with the dequantised teacher ``q·2^(code − 127)`` in place of the tensor;
``impl="torch"`` dequantises and runs the composites.

Not built: sample-ID masks with soft targets, quantised operands for the
student pair, the ring strategy, teacher LSEs cached across steps.
"""

from __future__ import annotations

import math
from typing import Optional

import torch
import torch.distributed as dist
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..parallel.collectives import all_gather_with_grad
from .retrieval import (
    _TORCH_ROW_CHUNK,
    _compute_dtype,
    _positive_rows,
    positive_scores,
)
from .softmax_loss import _backward, _check_block, _fwd_step, _owner_go


def _torch_distill(zimg, ztxt, t_prime, bias, timg, ttxt, teacher_t_prime,
                   teacher_bias, alpha, diag_offset, col_chunk):
    """Differentiable composite, chunked over columns: holds ``O(b ·
    col_chunk)`` logits and targets at a time."""
    b, n = zimg.shape[0], ztxt.shape[0]
    cdt = torch.float64 if zimg.dtype == torch.float64 else torch.float32
    dev = zimg.device
    zi, ti = zimg.to(cdt), timg.detach().to(cdt)
    t = t_prime.to(device=dev, dtype=cdt).exp()
    bs = bias.to(device=dev, dtype=cdt)
    tt = torch.as_tensor(teacher_t_prime, dtype=cdt,
                         device=dev).detach().exp()
    bt = torch.as_tensor(teacher_bias, dtype=cdt, device=dev).detach()
    rows = torch.arange(b, device=dev)
    step = int(col_chunk) if col_chunk and col_chunk > 0 else n
    total = None
    for j0 in range(0, n, step):
        j1 = min(j0 + step, n)
        logits = zi @ ztxt[j0:j1].to(cdt).T * t + bs
        q = alpha * torch.sigmoid(ti @ ttxt[j0:j1].detach().to(cdt).T * tt
                                  + bt)
        if diag_offset is not None:
            cols = rows + (int(diag_offset) - j0)
            ok = (cols >= 0) & (cols < j1 - j0)
            q[rows[ok], cols[ok]] += 1.0 - alpha
        # softplus(z) − q·z, evaluated without cancellation
        part = F.binary_cross_entropy_with_logits(logits, q, reduction="sum")
        total = part if total is None else total + part
    return total


TEACHER_QUANTS = ("bf16", "mxfp8")


def _is_pair(x) -> bool:
    return isinstance(x, (tuple, list))


def _dequant_mx(q: torch.Tensor, e8: torch.Tensor, dtype) -> torch.Tensor:
    """``q·2^(code − 127)`` of a ``quantize_mx`` pair: exact in fp32 and
    fp64."""
    blocks = q.shape[1] // 32
    scale = torch.exp2(e8[:, :blocks].to(dtype) - 127.0)
    return (q.float().to(dtype).view(q.shape[0], blocks, 32)
            * scale[:, :, None]).reshape(q.shape)


def _teacher_operands(timg, ttxt, teacher_quant: str, hip: bool, cdt):
    """The teacher pair as the implementation reads it.  ``bf16``: the two
    tensors.  ``mxfp8``: each of ``timg`` / ``ttxt`` is a tensor, quantised
    here with ``ops.quantize_mx``, or a ``(q, e8)`` pair as it returns one;
    ``hip`` gets ``(timg_q, timg_e8, ttxt_q, ttxt_e8)`` — no bf16 copy of a
    stored pair is made — and ``torch`` the dequantised pair in ``cdt``."""
    if teacher_quant not in TEACHER_QUANTS:
        raise ValueError(f"unknown teacher_quant {teacher_quant!r}")
    if teacher_quant == "bf16":
        if _is_pair(timg) or _is_pair(ttxt):
            raise ValueError(
                "a (q, e8) teacher pair needs teacher_quant='mxfp8'")
        return timg.detach(), ttxt.detach()
    out = _as_mx_pair("timg", timg) + _as_mx_pair("ttxt", ttxt)
    if hip:
        return out
    return _dequant_mx(out[0], out[1], cdt), _dequant_mx(out[2], out[3], cdt)


def _as_mx_pair(what: str, x):
    """A teacher operand under ``teacher_quant="mxfp8"`` as its ``(q, e8)``
    pair: a stored pair as it is, a tensor quantised here."""
    if _is_pair(x) and len(x) != 2:
        raise ValueError(f"{what} must be a tensor or a (q, e8) pair")
    shape = tuple(_first(x).shape)
    if len(shape) != 2 or shape[1] < 32 or shape[1] % 32:
        raise ValueError(
            f"teacher_quant='mxfp8' needs d_T % 32 == 0 (got {what} {shape})")
    q, e8 = x if _is_pair(x) else ops.quantize_mx(x.detach())
    return q.detach(), e8.detach()


def _gather_teacher_text(ttxt, teacher_quant: str, world: int, group):
    """The module's plain all-gather of the local teacher text shard.  Under
    ``mxfp8`` the shard is quantised first — rows quantise independently, so
    the gathered pair is byte for byte the quantised gather — and travels as
    two ``uint8`` tensors, half the bytes of the bf16 gather."""
    if teacher_quant not in TEACHER_QUANTS:
        raise ValueError(f"unknown teacher_quant {teacher_quant!r}")

    def gather(shard):
        shard = shard.contiguous()
        if world == 1:
            return shard
        out = shard.new_empty((world * shard.shape[0], shard.shape[1]))
        dist.all_gather_into_tensor(out, shard, group=group)
        return out

    if teacher_quant == "bf16":
        if _is_pair(ttxt):
            raise ValueError(
                "a (q, e8) teacher pair needs teacher_quant='mxfp8'")
        return gather(ttxt.detach())
    q, e8 = _as_mx_pair("ttxt", ttxt)
    return gather(q.view(torch.uint8)).view(q.dtype), gather(e8)


def _teacher_text_rows(teacher, j0: int, j1: int):
    """``teacher`` (two bf16 tensors, or the four of an MXFP8 pair) with the
    text side cut to rows ``j0:j1``; row slices stay contiguous."""
    half = len(teacher) // 2
    return teacher[:half] + tuple(x[j0:j1] for x in teacher[half:])


class _FusedDistillLoss(torch.autograd.Function):
    """GPU path: ``ops.sigmoid_distill`` (``ops.sigmoid_distill_mx`` for an
    MXFP8 teacher) plus the library gradient GEMMs, in the saved-g or the
    band-recompute regime (module docstring)."""

    @staticmethod
    def forward(ctx, zimg, ztxt, t_prime, bias, teacher, teacher_t_prime,
                teacher_bias, alpha, diag_offset, col_chunk, want_grad):
        zimg, ztxt = zimg.contiguous(), ztxt.contiguous()
        teacher = tuple(x.contiguous() for x in teacher)
        op = ops.sigmoid_distill if len(teacher) == 2 else ops.sigmoid_distill_mx
        b, n = zimg.shape[0], ztxt.shape[0]
        # want_grad comes from the caller (grad mode is off in here).
        save_g = want_grad and col_chunk is None and b * n * 2 < 2 ** 32
        if save_g:
            partials, g = op(zimg, ztxt, t_prime, bias, *teacher,
                             teacher_t_prime, teacher_bias, alpha, diag_offset)
            sums = partials.double().sum(dim=0)
            ctx.save_for_backward(zimg, ztxt, t_prime, bias, sums, g)
            loss = sums[0]
        else:
            step = min(n, int(col_chunk) if col_chunk and col_chunk > 0
                       else ops.banded_col_step(b))
            loss = torch.zeros((), device=zimg.device, dtype=torch.float64)
            for j0, j1, diag_j in ops.col_bands(n, step, diag_offset):
                partials = op(
                    zimg, ztxt[j0:j1], t_prime, bias,
                    *_teacher_text_rows(teacher, j0, j1), teacher_t_prime,
                    teacher_bias, alpha, diag_j, want_g=False)[0]
                # the same reduction as saved-g: one block gives the same bits
                loss = loss + partials.double().sum(dim=0)[0]
            ctx.save_for_backward(zimg, ztxt, t_prime, bias, teacher_t_prime,
                                  teacher_bias, *teacher)
            ctx.step = step
        ctx.save_g, ctx.alpha, ctx.diag_offset = save_g, alpha, diag_offset
        ctx.op = op
        return loss.float()

    @staticmethod
    def backward(ctx, grad_output):
        zimg, ztxt, t_prime, bias, *rest = ctx.saved_tensors
        n, dev = ztxt.shape[0], zimg.device
        go = ops._go_scalar(grad_output, dev)
        t = ops._prep_scalar(t_prime, dev).exp()
        if ctx.save_g:
            sums, g = rest
            # bf16_scale=True: the products stay bf16 (see ops.grad_gemms).
            dzimg, dztxt = ops.grad_gemms(ops.GBand(g, None, ztxt, None),
                                          zimg, n, go * t, bf16_scale=True)
        else:
            teacher_t_prime, teacher_bias, *teacher = rest
            teacher = tuple(teacher)
            parts = []

            def emit(j0, j1, diag_j, g, gt):
                partials = ctx.op(
                    zimg, ztxt[j0:j1], t_prime, bias,
                    *_teacher_text_rows(teacher, j0, j1), teacher_t_prime,
                    teacher_bias, ctx.alpha, diag_j, g=g)[0]
                parts.append(partials.double().sum(dim=0))

            # bf16_scale stays False, also when one band covers the block.
            # fp32_bands: with soft targets g takes both signs along a row,
            # the bands' partial dzimg sums cancel, and a bf16 partial would
            # be rounded at its own size, not at the element's.
            dzimg, dztxt = ops.band_grad_gemms(
                zimg, ztxt, ctx.step, emit, go * t,
                diag_offset=ctx.diag_offset, fp32_bands=True)
            sums = torch.stack(parts).sum(dim=0)
        dt = sums[1] * (go * t).double()
        db = sums[2] * go.double()
        return (dzimg, dztxt,
                dt.to(device=t_prime.device,
                      dtype=t_prime.dtype).reshape(t_prime.shape),
                db.to(device=bias.device, dtype=bias.dtype).reshape(bias.shape),
                None, None, None, None, None, None, None)


def sigmoid_distillation_loss(zimg: torch.Tensor, ztxt: torch.Tensor,
                              t_prime: torch.Tensor, bias: torch.Tensor,
                              timg: torch.Tensor, ttxt: torch.Tensor,
                              teacher_t_prime: torch.Tensor,
                              teacher_bias: torch.Tensor, alpha: float = 1.0,
                              diag_offset: Optional[int] = None,
                              col_chunk: Optional[int] = None,
                              impl: str = "auto",
                              teacher_quant: str = "bf16") -> torch.Tensor:
    """Sum over the ``(b, n)`` block of the sigmoid cross-entropy of every
    student pair against the teacher's pair probability mixed with the hard
    label (see the module docstring).  Differentiable in ``zimg``, ``ztxt``,
    ``t_prime`` and ``bias``; the teacher's arguments get no gradient.

    Args:
        zimg: ``(b, d)`` student image embeddings (L2-normalized by the
            caller).
        ztxt: ``(n, d)`` student text embeddings.
        t_prime: scalar; the student's temperature is ``exp(t_prime)``.
        bias: scalar additive logit bias of the student.
        timg, ttxt: ``(b, d_T)`` / ``(n, d_T)`` teacher embeddings of the same
            samples; ``d_T`` is independent of ``d``.
        teacher_t_prime, teacher_bias: the teacher's scalars (tensors or
            Python numbers), in the student's parametrisation.
        alpha: weight of the teacher's probability in the target, in
            ``[0, 1]``; the hard label weighs ``1 − alpha``.
        diag_offset: column of row 0's hard positive; ``None``: none.
        col_chunk: columns per kernel pass, bounding the workspace to
            ``O(b · col_chunk)``; ``None``: the whole block (saved-g when
            gradients are wanted and the slab stays below 2³² bytes).
        impl: ``auto`` (``hip`` on GPU when all four embeddings are bf16,
            ``torch`` elsewhere) | ``hip`` (bf16 on GPU, ``d % 8 == 0`` and
            ``d_T % 8 == 0``; raises without the built extension or for other
            dtypes) | ``torch``.
        teacher_quant: ``bf16`` | ``mxfp8`` — the teacher pair read as OCP
            MXFP8 (``d_T % 32 == 0``): each of ``timg`` / ``ttxt`` is a
            tensor, quantised once per call with ``ops.quantize_mx``, or a
            stored ``(q, e8)`` pair as it returns one.  ``hip`` runs the
            teacher's K loop on the MX-scaled MFMA; ``torch`` dequantises and
            runs the composite.  The student pair and all gradients are
            untouched.

    Returns a 0-d tensor; the caller normalises.
    """
    if zimg.dim() != 2 or ztxt.dim() != 2 or zimg.shape[1] != ztxt.shape[1]:
        raise ValueError(f"shape mismatch: student image "
                         f"{tuple(zimg.shape)} text {tuple(ztxt.shape)}")
    _check_teacher(timg, ttxt, zimg.shape[0], ztxt.shape[0])
    alpha = float(alpha)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"alpha must lie in [0, 1] (got {alpha})")
    if impl == "auto":
        impl = "hip" if _hip_auto(zimg, ztxt, timg, ttxt) else "torch"
    if impl not in ("hip", "torch"):
        raise ValueError(f"unknown impl {impl!r}")
    teacher = _teacher_operands(
        timg, ttxt, teacher_quant, impl == "hip",
        torch.float64 if zimg.dtype == torch.float64 else torch.float32)
    if impl == "torch":
        return _torch_distill(zimg, ztxt, t_prime, bias, *teacher,
                              teacher_t_prime, teacher_bias, alpha,
                              diag_offset, col_chunk)
    dev = zimg.device
    want_grad = torch.is_grad_enabled() and any(
        t.requires_grad for t in (zimg, ztxt, t_prime, bias))
    return _FusedDistillLoss.apply(
        zimg, ztxt, t_prime, bias, teacher,
        ops._prep_scalar(torch.as_tensor(teacher_t_prime), dev),
        ops._prep_scalar(torch.as_tensor(teacher_bias), dev), alpha,
        diag_offset, col_chunk, want_grad)


def _first(x):
    """The tensor that carries a teacher operand's shape, dtype and device:
    itself, or the ``q`` of a ``(q, e8)`` pair."""
    return x[0] if _is_pair(x) and len(x) else x


def _check_teacher(timg, ttxt, b: int, n: int):
    """The teacher operands' shapes against the student's ``(b, n)`` block."""
    ti, tt = _first(timg), _first(ttxt)
    if ti.dim() != 2 or tt.dim() != 2 or ti.shape[1] != tt.shape[1]:
        raise ValueError(f"shape mismatch: teacher image {tuple(ti.shape)} "
                         f"text {tuple(tt.shape)}")
    if (ti.shape[0], tt.shape[0]) != (b, n):
        raise ValueError(
            f"teacher rows {(ti.shape[0], tt.shape[0])} do not pair up "
            f"with the student's {(b, n)}")


def _hip_auto(zimg, ztxt, timg, ttxt) -> bool:
    """``impl="auto"`` takes ``hip``: bf16 students on a GPU with a teacher in
    bf16 or stored as ``(q, e8)`` pairs."""
    return zimg.is_cuda and all(
        x.dtype == torch.bfloat16 for x in (zimg, ztxt)) and all(
        _is_pair(x) or x.dtype == torch.bfloat16 for x in (timg, ttxt))


class DistributedSigmoidDistillLoss(nn.Module):
    """All-rank sigmoid distillation loss with module-owned student scalars.

    ``t_prime`` (init ``log 10``) and ``bias`` (init ``−10``) are parameters
    as in ``DistributedSigmoidLoss``; the teacher's ``teacher_t_prime`` and
    ``teacher_bias`` are buffers (they move and save with the module and get
    no gradient).  ``forward`` takes the *local* student and teacher shards,
    all-gathers the student text shard differentiably and the teacher text
    shard plainly, evaluates the local ``(b, W·b)`` grid in one call with
    ``diag_offset = rank·b`` and divides by ``gpu_batch_size``; under DDP
    gradient averaging that is the single-rank ``sum / (W·b)``.  All-gather
    strategy only.
    """

    def __init__(self, gpu_batch_size: int, alpha: float,
                 teacher_t_prime: float, teacher_bias: float,
                 col_chunk: Optional[int] = None, impl: str = "auto",
                 teacher_quant: str = "bf16"):
        super().__init__()
        if not 0.0 <= float(alpha) <= 1.0:
            raise ValueError(f"alpha must lie in [0, 1] (got {alpha})")
        if teacher_quant not in TEACHER_QUANTS:
            raise ValueError(f"unknown teacher_quant {teacher_quant!r}")
        self.teacher_quant = teacher_quant
        self.t_prime = nn.Parameter(torch.tensor(math.log(10.0)))
        self.bias = nn.Parameter(torch.tensor(-10.0))
        self.register_buffer("teacher_t_prime",
                             torch.tensor(float(teacher_t_prime)))
        self.register_buffer("teacher_bias", torch.tensor(float(teacher_bias)))
        self.gpu_batch_size = gpu_batch_size
        self.alpha = float(alpha)
        self.col_chunk = col_chunk
        self.impl = impl

    def forward(self, image_embeddings: torch.Tensor,
                text_embeddings: torch.Tensor,
                teacher_image_embeddings: torch.Tensor,
                teacher_text_embeddings: torch.Tensor,
                group=None) -> torch.Tensor:
        world, rank = 1, 0
        if dist.is_available() and dist.is_initialized():
            world, rank = dist.get_world_size(group), dist.get_rank(group)
        b_txt = text_embeddings.shape[0]
        all_txt = all_gather_with_grad(text_embeddings, group=group)
        all_ttxt = _gather_teacher_text(teacher_text_embeddings,
                                        self.teacher_quant, world, group)
        total = sigmoid_distillation_loss(
            image_embeddings, all_txt, self.t_prime, self.bias,
            teacher_image_embeddings, all_ttxt, self.teacher_t_prime,
            self.teacher_bias, alpha=self.alpha, diag_offset=rank * b_txt,
            col_chunk=self.col_chunk, impl=self.impl,
            teacher_quant=self.teacher_quant)
        return total / self.gpu_batch_size


# ---------------------------------------------------------------------------
# The softmax / KL form
# ---------------------------------------------------------------------------
#
# With t = exp(t_prime) and t_T = exp(teacher_t_prime) (no bias: it cancels):
#
#     z_ij = t·<zimg_i, ztxt_j>                  v_ij = t_T·<timg_i, ttxt_j>
#     LS^r_i = log Σ_j exp z_ij                   LS^c_j = log Σ_i exp z_ij
#     LT^r_i = log Σ_j exp v_ij                   LT^c_j = log Σ_i exp v_ij
#     P^r_ij = exp(v_ij − LT^r_i)                 P^c_ij = exp(v_ij − LT^c_j)
#     x^r_i  = Σ_j P^r_ij·(v_ij − z_ij)           x^c_j  = Σ_i P^c_ij·(v_ij − z_ij)
#
#     D = Σ_i (LS^r_i − LT^r_i + x^r_i)     (= Σ_i KL(P^r_i ‖ softmax z_i))
#       + Σ_j (LS^c_j − LT^c_j + x^c_j)
#     H = softmax_contrastive_loss(zimg, ztxt, t_prime, diag_offset)
#     total = alpha·D + (1 − alpha)·H
#
#     g_ij = rw_i·exp(z_ij − LS^r_i) + cw_j·exp(z_ij − LS^c_j)
#            − rtw_i·P^r_ij − ctw_j·P^c_ij − [j == i + diag]·(rhw_i + chw_j)
#     rtw = go·alpha   rhw = go·(1 − alpha)·[row has a positive]   rw = rtw + rhw
#     dzimg = t·g@ztxt    dztxt = t·gᵀ@zimg    dt' = t·Σ g_ij·s_ij   (s = z/t)
#
# Sum form; the teacher side gets no gradient.  x rides on the teacher's LSE:
# over column chunks and ranks the LSEs fold with logaddexp and x as
# Σ_c exp(LT_c − LT)·x_c.


def _fold_x(lt_a, x_a, lt_b, x_b):
    """Two shares of a teacher LSE and of the expectation that rides on it →
    ``(lse, x)`` of their union."""
    lt = torch.logaddexp(lt_a, lt_b)
    return lt, torch.exp(lt_a - lt) * x_a + torch.exp(lt_b - lt) * x_b


def _torch_pair_distill_stats(zimg, ztxt, t_prime, timg, ttxt,
                              teacher_t_prime, row_chunk=_TORCH_ROW_CHUNK):
    """``ops.pair_distill_stats`` as a row-chunked torch composite: holds
    ``O(row_chunk · n)`` logits of each grid at a time."""
    b, n = zimg.shape[0], ztxt.shape[0]
    dev, cdt = zimg.device, _compute_dtype(zimg)
    t = t_prime.detach().to(device=dev, dtype=cdt).exp()
    tt = teacher_t_prime.detach().to(device=dev, dtype=cdt).exp()
    zt, ttx = ztxt.detach().to(cdt), ttxt.detach().to(cdt)
    row = [torch.empty(b, device=dev, dtype=cdt) for _ in range(3)]
    col_ls = torch.full((n,), -math.inf, device=dev, dtype=cdt)
    col_lt, col_x = col_ls.clone(), torch.zeros(n, device=dev, dtype=cdt)
    for r0 in range(0, b, row_chunk):
        r1 = min(b, r0 + row_chunk)
        z = (zimg[r0:r1].detach().to(cdt) @ zt.T) * t
        v = (timg[r0:r1].detach().to(cdt) @ ttx.T) * tt

        def stats(dim):
            lt = torch.logsumexp(v, dim)
            x = (torch.exp(v - lt.unsqueeze(dim)) * (v - z)).sum(dim)
            return torch.logsumexp(z, dim), lt, x

        for out, val in zip(row, stats(1)):
            out[r0:r1] = val
        ls_c, lt_c, x_c = stats(0)
        col_ls = torch.logaddexp(col_ls, ls_c)
        col_lt, col_x = _fold_x(col_lt, col_x, lt_c, x_c)
    return ops.PairDistillStats(*row, col_ls, col_lt, col_x)


def _torch_softmax_distill_g(zimg, ztxt, t_prime, timg, ttxt,
                             teacher_t_prime, row, col, diag_offset, g=None,
                             row_chunk=_TORCH_ROW_CHUNK):
    """``ops.softmax_distill_g`` as a row-chunked torch composite; ``g`` is
    in the compute dtype and ``gs_partials`` has one entry."""
    b, n = zimg.shape[0], ztxt.shape[0]
    dev, cdt = zimg.device, _compute_dtype(zimg)
    t = t_prime.detach().to(device=dev, dtype=cdt).exp()
    tt = teacher_t_prime.detach().to(device=dev, dtype=cdt).exp()
    zt, ttx = ztxt.detach().to(cdt), ttxt.detach().to(cdt)
    if g is None:
        g = torch.empty((b, n), device=dev, dtype=cdt)
    gs = torch.zeros((), device=dev, dtype=torch.float64)
    cols = torch.arange(n, device=dev)
    for r0 in range(0, b, row_chunk):
        r1 = min(b, r0 + row_chunk)
        s = zimg[r0:r1].detach().to(cdt) @ zt.T
        z, v = s * t, (timg[r0:r1].detach().to(cdt) @ ttx.T) * tt
        gv, hw = torch.zeros_like(z), torch.zeros_like(z)
        for side, sl in ((row, lambda x: x[r0:r1, None]),
                         (col, lambda x: x[None, :])):
            if side is None:
                continue
            ls, lt, w, tw, h = (sl(x) for x in side)
            gv += w * torch.exp(z - ls) - tw * torch.exp(v - lt)
            hw += h
        if diag_offset is not None:
            pos = torch.arange(r0, r1, device=dev) + int(diag_offset)
            gv -= hw * (cols[None, :] == pos[:, None])
        g[r0:r1] = gv
        gs += (gv * s).double().sum()
    return g, gs.reshape(1)


class _SoftmaxDistillLoss(torch.autograd.Function):
    """Both implementations, in the shape of ``_SoftmaxLoss``: ``hip`` runs
    the fused kernels and the library gradient GEMMs, ``torch`` the
    composites above; the chunking, the collectives and the weights are
    shared."""

    @staticmethod
    def forward(ctx, zimg, ztxt, t_prime, teacher, teacher_t_prime, alpha,
                diag_offset, col_chunk, impl, group):
        # teacher: (timg, ttxt), or the four tensors of an MXFP8 pair (hip).
        hip, mx = impl == "hip", len(teacher) == 4
        stats_fn = ((ops.pair_distill_stats_mx if mx
                     else ops.pair_distill_stats) if hip
                    else _torch_pair_distill_stats)
        zimg, ztxt = zimg.contiguous(), ztxt.contiguous()
        teacher = tuple(x.contiguous() for x in teacher)
        b, n = zimg.shape[0], ztxt.shape[0]
        row, col_parts = None, []
        for j0, j1, _ in ops.col_bands(n, _fwd_step(col_chunk, n)):
            st = stats_fn(zimg, ztxt[j0:j1], t_prime,
                          *_teacher_text_rows(teacher, j0, j1),
                          teacher_t_prime)
            if row is None:
                row = st[:3]
            else:
                row = (torch.logaddexp(row[0], st[0]),
                       *_fold_x(row[1], row[2], st[1], st[2]))
            col_parts.append(torch.stack(st[3:]))
        col = col_parts[0] if len(col_parts) == 1 else torch.cat(col_parts, 1)
        own = slice(0, n)
        if group is not None:
            # This rank's rows are a share of every column: gather the
            # shares and fold them in rank order, the same on every rank.
            world, rank = dist.get_world_size(group), dist.get_rank(group)
            shares = torch.empty(world * 3 * n, device=col.device,
                                 dtype=col.dtype)
            dist.all_gather_into_tensor(shares, col.reshape(-1), group=group)
            shares = shares.view(world, 3, n)
            ls = torch.logsumexp(shares[:, 0], dim=0)
            lt, x = shares[0, 1], shares[0, 2]
            for q in range(1, world):
                lt, x = _fold_x(lt, x, shares[q, 1], shares[q, 2])
            col = torch.stack((ls, lt, x))
            # Column j belongs to the loss of rank j // b, its text's owner.
            own = slice(rank * b, (rank + 1) * b)
        cdt = row[0].dtype
        kl = ((row[0].double() - row[1].double() + row[2].double()).sum()
              + (col[0, own].double() - col[1, own].double()
                 + col[2, own].double()).sum())
        rows, cols = _positive_rows(b, n, diag_offset, zimg.device)
        t = t_prime.detach().to(device=zimg.device, dtype=cdt).exp()
        z_pos = positive_scores(zimg, ztxt, diag_offset)[rows] * t
        hard = (row[0][rows].double() + col[0][cols].double()
                - 2.0 * z_pos.double()).sum()
        total = (alpha * kl + (1.0 - alpha) * hard).to(cdt)
        ctx.save_for_backward(zimg, ztxt, t_prime, teacher_t_prime, row[0],
                              row[1], col[0].contiguous(),
                              col[1].contiguous(), *teacher)
        ctx.alpha, ctx.diag_offset, ctx.col_chunk = alpha, diag_offset, col_chunk
        ctx.hip, ctx.group = hip, group
        return total

    @staticmethod
    def backward(ctx, grad_output):
        (zimg, ztxt, t_prime, teacher_t_prime, row_ls, row_lt, col_ls,
         col_lt, *teacher) = ctx.saved_tensors
        teacher = tuple(teacher)
        b, n = zimg.shape[0], ztxt.shape[0]
        dev, cdt = zimg.device, row_ls.dtype
        go = ops._go_scalar(grad_output, dev, cdt)
        rows, cols = _positive_rows(b, n, ctx.diag_offset, dev)
        row_tw = (go * ctx.alpha).expand(b).contiguous()
        row_hw = torch.zeros(b, device=dev, dtype=cdt)
        row_hw[rows] = go * (1.0 - ctx.alpha)
        if ctx.group is not None:
            # Every column has its positive on its owner, whose go it takes.
            col_go = _owner_go(go, b, ctx.group)
            col_hw = col_go * (1.0 - ctx.alpha)
        else:
            col_go = go.expand(n)
            col_hw = torch.zeros(n, device=dev, dtype=cdt)
            col_hw[cols] = go * (1.0 - ctx.alpha)
        col_tw = (col_go * ctx.alpha).contiguous()
        row = (row_ls, row_lt, row_tw + row_hw, row_tw, row_hw)
        col = (col_ls, col_lt, col_tw + col_hw, col_tw, col_hw)
        t = t_prime.detach().to(device=dev, dtype=cdt).exp()
        g_fn = ((ops.softmax_distill_g_mx if len(teacher) == 4
                 else ops.softmax_distill_g) if ctx.hip
                else _torch_softmax_distill_g)
        gs_parts = []

        def g_band(j0, j1, diag_j, g, gt):
            g, gs = g_fn(zimg, ztxt[j0:j1], t_prime,
                         *_teacher_text_rows(teacher, j0, j1),
                         teacher_t_prime, row,
                         tuple(v[j0:j1].contiguous() for v in col), diag_j,
                         g=g)
            gs_parts.append(gs)
            return g

        # fp32_bands: with soft targets g takes both signs along a row, the
        # bands' partial dzimg sums cancel, and a bf16 partial would be
        # rounded at its own size, not at the element's.
        return _backward(ctx.hip, zimg, ztxt, t_prime, t, ctx.col_chunk,
                         ctx.diag_offset, g_band, gs_parts, 10,
                         fp32_bands=True)


def softmax_distillation_loss(zimg: torch.Tensor, ztxt: torch.Tensor,
                              t_prime: torch.Tensor, timg: torch.Tensor,
                              ttxt: torch.Tensor,
                              teacher_t_prime: torch.Tensor,
                              alpha: float = 1.0,
                              diag_offset: Optional[int] = None,
                              col_chunk: Optional[int] = None,
                              impl: str = "auto", group=None,
                              teacher_quant: str = "bf16") -> torch.Tensor:
    """Sum over the rows and the columns of the ``(b, n)`` block of the KL
    divergence of the student's softmax from the teacher's, mixed with the
    hard softmax contrastive loss: ``alpha·D + (1 − alpha)·H`` (see the
    contract above).  Differentiable in ``zimg``, ``ztxt`` and ``t_prime``;
    the teacher's arguments get no gradient.

    ``alpha = 0`` is ``softmax_contrastive_loss``; ``alpha = 1`` is pure
    distillation — non-negative, and 0 with zero gradient where the
    student's logits equal the teacher's; ``diag_offset=None`` leaves out
    the hard part.

    Args:
        zimg: ``(b, d)`` student image embeddings (L2-normalized by the
            caller).
        ztxt: ``(n, d)`` student text embeddings.
        t_prime: scalar; the student's temperature is ``exp(t_prime)``.
        timg, ttxt: ``(b, d_T)`` / ``(n, d_T)`` teacher embeddings of the same
            samples; ``d_T`` is independent of ``d``.
        teacher_t_prime: the teacher's scalar (tensor or Python number).
        alpha: weight of the KL part, in ``[0, 1]``; the hard loss weighs
            ``1 − alpha``.
        diag_offset: column of row 0's hard positive; ``None``: none.
        col_chunk: columns per kernel pass (forward statistics and backward
            g band), bounding the workspace to ``O(b · col_chunk)``; ``None``:
            the whole block, banded in backward only when the bf16 g slab
            would reach 2³² bytes.
        impl: ``auto`` (``hip`` on GPU when all four embeddings are bf16,
            ``torch`` elsewhere) | ``hip`` (bf16 on GPU, ``d % 8 == 0`` and
            ``d_T % 8 == 0``; raises without the built extension or for other
            dtypes) | ``torch``.
        group: a process group of ``W > 1`` ranks for the one-grid
            distributed form (``n == W·b``, ``diag_offset == rank·b``):
            column ``j`` counts for the loss of rank ``j // b``; ``None``:
            this block alone.
        teacher_quant: ``bf16`` | ``mxfp8``, as for
            ``sigmoid_distillation_loss``: the teacher pair as OCP MXFP8
            (``d_T % 32 == 0``), tensors quantised per call or stored ``(q,
            e8)`` pairs.

    Returns a 0-d tensor; the caller normalises.
    """
    impl, group, world, rank = _check_block(
        zimg, ztxt, impl, group, _hip_auto(zimg, ztxt, timg, ttxt))
    b, n = zimg.shape[0], ztxt.shape[0]
    _check_teacher(timg, ttxt, b, n)
    teacher = _teacher_operands(timg, ttxt, teacher_quant, impl == "hip",
                                _compute_dtype(zimg))
    alpha = float(alpha)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"alpha must lie in [0, 1] (got {alpha})")
    if group is not None and (n != world * b or diag_offset != rank * b):
        raise ValueError(
            f"the distributed form needs n == W·b and diag_offset == "
            f"rank·b (got b={b}, n={n}, W={world}, rank={rank}, "
            f"diag_offset={diag_offset})")
    if not isinstance(teacher_t_prime, torch.Tensor):
        # A Python number keeps its precision on the fp64 path.
        teacher_t_prime = torch.tensor(float(teacher_t_prime),
                                       dtype=torch.float64)
    return _SoftmaxDistillLoss.apply(
        zimg, ztxt, t_prime, teacher,
        teacher_t_prime.detach().to(zimg.device), alpha, diag_offset,
        col_chunk, impl, group)


class DistributedSoftmaxDistillLoss(nn.Module):
    """All-rank softmax distillation loss with a module-owned, learnable
    student ``t_prime`` (init ``log(1 / init_temperature)``, clamped in the
    forward at ``log(max_logit_scale)`` as in ``DistributedSoftmaxLoss``);
    the teacher's ``teacher_t_prime`` is a buffer.

    ``forward`` takes the *local* student and teacher shards, all-gathers
    the student text shard differentiably and the teacher text shard
    plainly, evaluates the ``(b, W·b)`` grid in one call with ``diag_offset =
    rank·b`` and returns ``total / (2·gpu_batch_size)``; under DDP gradient
    averaging ``W`` ranks reproduce the single-rank gradients of the global
    batch.  All-gather strategy only.
    """

    def __init__(self, gpu_batch_size: int, alpha: float,
                 teacher_t_prime: float, col_chunk: Optional[int] = None,
                 impl: str = "auto", init_temperature: float = 0.07,
                 max_logit_scale: float = 100.0, teacher_quant: str = "bf16"):
        super().__init__()
        if not 0.0 <= float(alpha) <= 1.0:
            raise ValueError(f"alpha must lie in [0, 1] (got {alpha})")
        if teacher_quant not in TEACHER_QUANTS:
            raise ValueError(f"unknown teacher_quant {teacher_quant!r}")
        self.teacher_quant = teacher_quant
        self.t_prime = nn.Parameter(
            torch.tensor(math.log(1.0 / init_temperature)))
        self.register_buffer("teacher_t_prime",
                             torch.tensor(float(teacher_t_prime)))
        self.gpu_batch_size = gpu_batch_size
        self.alpha = float(alpha)
        self.col_chunk = col_chunk
        self.impl = impl
        self.max_logit_scale = max_logit_scale

    def forward(self, image_embeddings: torch.Tensor,
                text_embeddings: torch.Tensor,
                teacher_image_embeddings: torch.Tensor,
                teacher_text_embeddings: torch.Tensor,
                group=None) -> torch.Tensor:
        world, rank = 1, 0
        if dist.is_available() and dist.is_initialized():
            world, rank = dist.get_world_size(group), dist.get_rank(group)
        b_txt = text_embeddings.shape[0]
        t_prime = self.t_prime.clamp(max=math.log(self.max_logit_scale))
        all_txt = all_gather_with_grad(text_embeddings, group=group)
        all_ttxt = _gather_teacher_text(teacher_text_embeddings,
                                        self.teacher_quant, world, group)
        if world > 1 and group is None:
            group = dist.group.WORLD
        total = softmax_distillation_loss(
            image_embeddings, all_txt, t_prime, teacher_image_embeddings,
            all_ttxt, self.teacher_t_prime, alpha=self.alpha,
            diag_offset=rank * b_txt, col_chunk=self.col_chunk,
            impl=self.impl, group=group if world > 1 else None,
            teacher_quant=self.teacher_quant)
        return total / (2 * self.gpu_batch_size)
