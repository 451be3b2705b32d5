"""Single-device sigmoid contrastive loss op: fused HIP kernel + torch fallback.

This is the op-level core that the loss modules build on.  It computes, for a
local image block ``zimg (b, d)`` against a text block ``ztxt (n, d)``:

    z_ij    = t · ⟨zimg_i, ztxt_j⟩ + bias,      t = exp(t_prime)
    l_ij    = +1 if j == i + diag_offset else −1
    loss    = Σ_ij  −logsigmoid(l_ij · z_ij)  =  Σ_ij softplus(−l_ij · z_ij)

(the reference computes exactly this per chunk — ``distributed_sigmoid_loss.py:22-33``
and ``rwightman_sigmoid_loss.py:43-66`` — but materializes the ``(b, n)`` labels
and logits; here labels are an index predicate and on GPU the logits tile never
leaves registers).

Backward (wrt zimg, ztxt, t_prime, bias), with g_ij = −l_ij·σ(−l_ij·z_ij):

    dzimg  = go · t · (g @ ztxt)
    dztxt  = go · t · (gᵀ @ zimg)
    dt'    = go · Σ g_ij · (z_ij − bias)        (chain rule through t = e^{t'})
    dbias  = go · Σ g_ij

On a GPU, dispatch goes to the hand-written CDNA4 kernels in
``distributed_sigmoid_loss_amd.ops`` (MFMA logits, fused epilogue, fp32
accumulation).  By default the forward also emits the dL/dlogit slab
("saved-g" — single-slab or column-banded) so backward is pure GEMMs; the
recompute-backward kernels serve explicit ``col_chunk`` runs and batches
whose g would not fit HBM.  On CPU (and only on CPU) a plain differentiable
PyTorch path is used — on a GPU a missing extension raises rather than
silently falling back.

Column chunking: ``col_chunk`` bounds the working set to ``O(b·col_chunk)`` so
per-GPU batches of 131072+ (BASELINE config 4) never materialize a full
``(b, n)`` intermediate anywhere.
"""

from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from .. import ops

# With col_chunk=None the GPU backward uses a single g slab whenever its
# 32-bit store addressing allows (b·n·esz < 2^32) and auto-halves the slab
# otherwise — e.g. per-GPU b=131072 against n=131072 runs at 8192-column
# slabs (2 GiB workspace), comfortably inside 288 GB HBM3E.  Set col_chunk
# explicitly to bound workspace tighter.


def _labels(b: int, n: int, diag_offset: Optional[int], device, dtype):
    """Materialized ±1 label block (CPU fallback path only)."""
    lab = -torch.ones((b, n), device=device, dtype=dtype)
    if diag_offset is not None:
        i = torch.arange(b, device=device)
        j = i + diag_offset
        m = (j >= 0) & (j < n)
        lab[i[m], j[m]] = 1.0
    return lab


def _torch_loss(zimg: torch.Tensor, ztxt: torch.Tensor, t_prime: torch.Tensor,
                bias: torch.Tensor, diag_offset: Optional[int],
                col_chunk: Optional[int]) -> torch.Tensor:
    """Differentiable reference path (CPU).  fp32 compute for stability."""
    b, d = zimg.shape
    n = ztxt.shape[0]
    t = t_prime.exp()
    total = None
    step = col_chunk or n
    for j0 in range(0, n, step):
        j1 = min(j0 + step, n)
        zt = ztxt[j0:j1]
        logits = zimg @ zt.T * t + bias
        off = None if diag_offset is None else diag_offset - j0
        lab = _labels(b, j1 - j0, off, logits.device, logits.dtype)
        part = -F.logsigmoid(lab * logits).sum()
        total = part if total is None else total + part
    return total


def _torch_bwd(zimg, ztxt, t_prime, bias, diag_offset, grad_output,
               col_chunk):
    """Manual backward for the CPU path (no autograd), chunked over columns.

    Mirrors the gradient algebra in the module docstring; used by the
    hand-written distributed autograd Functions whose backward cannot rely on
    a saved graph.
    """
    b, d = zimg.shape
    n = ztxt.shape[0]
    t = t_prime.exp()
    dzimg = torch.zeros_like(zimg)
    dztxt = torch.zeros_like(ztxt)
    # Scalar partials accumulate at >= fp32 (fp64 inputs keep fp64 — the
    # float64 gradcheck/property oracles compare against autograd exactly).
    acc = torch.promote_types(zimg.dtype, torch.float32)
    dt_raw = torch.zeros((), dtype=acc, device=zimg.device)
    dbias = torch.zeros((), dtype=acc, device=zimg.device)
    step = col_chunk or n
    for j0 in range(0, n, step):
        j1 = min(j0 + step, n)
        zt = ztxt[j0:j1]
        dot = zimg @ zt.T
        z = dot * t + bias
        off = None if diag_offset is None else diag_offset - j0
        lab = _labels(b, j1 - j0, off, z.device, z.dtype)
        g = -lab * torch.sigmoid(-lab * z)
        dzimg += (g @ zt) * t
        dztxt[j0:j1] = (g.T @ zimg) * t
        dt_raw += (g * dot).to(acc).sum() * t.to(acc)
        dbias += g.to(acc).sum()
    go = grad_output
    return (dzimg * go, dztxt * go,
            (dt_raw * go).to(t_prime.dtype).reshape(t_prime.shape),
            (dbias * go).to(bias.dtype).reshape(bias.shape))


def chunk_loss_fwd(zimg, ztxt, t_prime, bias, diag_offset=None,
                   col_chunk=None, impl="auto", quant="bf16", qcache=None):
    """Non-differentiable forward of the block loss (used inside hand-written
    autograd Functions).  Returns a scalar tensor."""
    if impl == "auto":
        impl = "hip" if zimg.is_cuda else "torch"
    if impl == "hip":
        return ops.siglip_fwd(zimg.contiguous(), ztxt.contiguous(), t_prime,
                              bias, diag_offset, quant=quant, qcache=qcache)
    with torch.no_grad():
        return _torch_loss(zimg, ztxt, t_prime, bias, diag_offset, col_chunk)


def chunk_loss_bwd(zimg, ztxt, t_prime, bias, diag_offset, grad_output,
                   col_chunk=None, impl="auto", quant="bf16",
                   on_dztxt=None, qcache=None):
    """Gradients of :func:`chunk_loss_fwd` wrt (zimg, ztxt, t_prime, bias).

    ``on_dztxt(dztxt)`` (optional) is invoked as soon as the text gradient is
    materialized, before the image-gradient GEMM — lets a distributed caller
    start its reduce-scatter while the remaining GEMM runs.  ``qcache`` is
    the forward's ``ops.QuantCache`` (fp8/mixed; ignored on the torch path).
    """
    if impl == "auto":
        impl = "hip" if zimg.is_cuda else "torch"
    if impl == "hip":
        return ops.siglip_bwd(zimg.contiguous(), ztxt.contiguous(), t_prime,
                              bias, diag_offset, grad_output, col_chunk,
                              quant=quant, on_dztxt=on_dztxt, qcache=qcache)
    with torch.no_grad():
        out = _torch_bwd(zimg, ztxt, t_prime, bias, diag_offset, grad_output,
                         col_chunk)
        if on_dztxt is not None:
            on_dztxt(out[1])
        return out


class _FusedSigmoidLoss(torch.autograd.Function):
    """GPU path: hand-written HIP kernels.

    Three backward regimes (`ops.save_g_enabled` and
    `ops.save_g_banded_enabled` pick); backward is a three-way dispatch to
    `ops.siglip_bwd_from_g` / `ops.siglip_bwd_banded` / `ops.siglip_bwd`:

    - **saved-g** (default when the slab fits — 2 GiB at the B=32k bf16
      headline config): forward runs the fwd+g kernel emitting loss, the
      dL/dlogit slab and both scalar partials in one pass; backward is then
      two GEMMs.  The logits GEMM runs once per step, like the reference's
      autograd (which saves the logits graph) but at O(b·n) g-slab memory
      instead of O(b·n) fp32 logits + labels.
    - **banded saved-g** (huge batches where ONE slab exceeds the kernel's
      32-bit addressing but the full g fits HBM — 32 GB at 131k² vs
      288 GB): forward emits g in column bands; backward is per-band GEMMs,
      still no recompute.
    - **recompute** (g would not fit HBM, explicit col_chunk, or
      SIGLIP_SAVE_G=0): forward emits only the scalar; backward recomputes
      logit tiles slab by slab.
    """

    @staticmethod
    def forward(ctx, zimg, ztxt, t_prime, bias, diag_offset, col_chunk,
                quant, want_grad):
        zimg = zimg.contiguous()
        ztxt = ztxt.contiguous()
        b, n = zimg.shape[0], ztxt.shape[0]
        d = zimg.shape[1]
        # want_grad is computed by the CALLER (grad mode is disabled inside
        # Function.forward, so it cannot be probed here).
        save_g = (want_grad and col_chunk is None and zimg.is_cuda
                  and ops.save_g_enabled(b, n, quant))
        banded = (not save_g and want_grad and col_chunk is None
                  and zimg.is_cuda and ops.extension_available()
                  and ops.save_g_banded_enabled(b, n, quant))
        qc = None
        if quant in ("fp8", "mixed") and zimg.is_cuda:
            # fp8 + saved-g on aligned shapes: ROW-wise pow2 scales, hardware
            # dequant in the MX MFMA (exact per-row dynamic range); otherwise
            # per-tensor scales folded into the temperature.
            if (quant == "fp8" and save_g and ops.extension_available()
                    and ops.rowwise_ok(b, n, d)):
                qc = ops.quantize_fp8_rowwise_pair(zimg, ztxt)
            else:
                qc = ops.quantize_fp8_pair(zimg, ztxt)
        # Saved layout: the four inputs, the regime's own tensors, then the
        # quantization cache's tensors (ctx.n_qc of them).
        if save_g:
            buf, g, gt = ops.siglip_fwd_g(zimg, ztxt, t_prime, bias,
                                          diag_offset, quant=quant,
                                          qcache=qc)
            out3 = ops.reduce_out3(buf)
            loss = out3[0].clone()
            regime = (out3, g) + ((gt,) if gt is not None else ())
        elif banded:
            buf = ops._out_buf(zimg.device)
            slabs = []
            for j0, j1, diag in ops.col_bands(n, ops.banded_col_step(b),
                                              diag_offset):
                g_s = torch.empty((b, j1 - j0), device=zimg.device,
                                  dtype=torch.bfloat16)
                ops.siglip_fwd_g(zimg, ztxt[j0:j1].contiguous(), t_prime,
                                 bias, diag, quant=quant, g_slab=g_s,
                                 out3=buf)
                slabs.append(g_s)
            out3 = ops.reduce_out3(buf)
            loss = out3[0].clone()
            regime = (out3,) + tuple(slabs)
        else:
            loss = ops.siglip_fwd(zimg, ztxt, t_prime, bias, diag_offset,
                                  quant=quant, qcache=qc)
            regime = ()
        qts = qc.tensors() if qc is not None else ()
        ctx.save_for_backward(zimg, ztxt, t_prime, bias, *regime, *qts)
        ctx.n_qc = len(qts)
        ctx.saved_g = save_g
        ctx.banded = banded
        ctx.diag_offset = diag_offset
        ctx.col_chunk = col_chunk   # None → single slab when addressable
        ctx.quant = quant
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        saved = ctx.saved_tensors
        inputs = saved[:4]
        regime = saved[4:len(saved) - ctx.n_qc]
        qc = (ops.QuantCache.from_tensors(saved[len(saved) - ctx.n_qc:])
              if ctx.n_qc else None)
        if ctx.banded:
            grads = ops.siglip_bwd_banded(*inputs, grad_output, regime[0],
                                          regime[1:])
        elif ctx.saved_g:
            out3, g, gt = (regime + (None,))[:3]
            grads = ops.siglip_bwd_from_g(*inputs, grad_output, out3, g, gt,
                                          quant=ctx.quant, qcache=qc)
        else:
            grads = ops.siglip_bwd(*inputs, ctx.diag_offset, grad_output,
                                   ctx.col_chunk, quant=ctx.quant, qcache=qc)
        return grads + (None, None, None, None)


def sigmoid_contrastive_loss(zimg: torch.Tensor, ztxt: torch.Tensor,
                             t_prime: torch.Tensor, bias: torch.Tensor,
                             diag_offset: Optional[int] = 0,
                             col_chunk: Optional[int] = None,
                             impl: str = "auto",
                             quant: str = "bf16") -> torch.Tensor:
    """Sum of per-pair sigmoid cross-entropy over the ``(b, n)`` block.

    Args:
        zimg: ``(b, d)`` image embeddings (assumed L2-normalized by caller,
            as in the reference — ``distributed_sigmoid_loss.py:20``).
        ztxt: ``(n, d)`` text embeddings.
        t_prime: scalar parameter; temperature is ``exp(t_prime)``.
        bias: scalar additive logit bias.
        diag_offset: column of row 0's positive pair, or ``None`` for a
            negatives-only block (remote chunk).
        col_chunk: column-slab size bounding workspace; None = single slab
            when addressable (see module note above).
        impl: ``auto`` | ``hip`` | ``torch``.

    Returns a scalar tensor (caller applies the ``1/b`` normalization).
    """
    if zimg.dim() != 2 or ztxt.dim() != 2 or zimg.shape[1] != ztxt.shape[1]:
        raise ValueError(
            f"shape mismatch: zimg {tuple(zimg.shape)} ztxt {tuple(ztxt.shape)}")
    if impl == "auto":
        impl = "hip" if zimg.is_cuda else "torch"
    if impl == "hip":
        want_grad = torch.is_grad_enabled() and any(
            t.requires_grad for t in (zimg, ztxt, t_prime, bias))
        return _FusedSigmoidLoss.apply(zimg, ztxt, t_prime, bias, diag_offset,
                                       col_chunk, quant, want_grad)
    if impl == "torch":
        return _torch_loss(zimg, ztxt, t_prime, bias, diag_offset, col_chunk)
    raise ValueError(f"unknown impl {impl!r}")
