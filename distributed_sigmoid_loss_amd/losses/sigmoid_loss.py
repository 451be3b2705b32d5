"""Distributed SigLIP loss modules.

Two public modules, mirroring the reference repo's API surface:

- :class:`DistributedSigmoidLoss` — module-owned learnable ``t_prime`` (init
  ``log 10``) and ``bias`` (init ``−10``); forward takes the *local* image and
  text embedding shards and returns ``Σ loss / gpu_batch_size``.  Behavioral
  parity with reference ``distributed_sigmoid_loss.py:8-48``.  Strategy is
  selectable: ``"all_gather"`` (differentiable all-gather, the reference's
  scheme) or ``"ring"`` (pipelined P2P ring with comm/compute overlap — the
  MI355X performance path).
- :class:`SigLipLoss` — caller-owned ``logit_scale``/``logit_bias`` passed to
  ``forward`` as arguments; ring strategy via the autograd neighbour-exchange
  primitives.  Behavioral parity with reference
  ``rwightman_sigmoid_loss.py:12-124`` (including ``bidir`` and the
  ``output_dict`` return form).

Unlike the reference (which builds labels on the default CPU device,
``distributed_sigmoid_loss.py:28-30``), everything here is device- and
dtype-correct: labels are an ``i == j + offset`` index predicate, never a
materialized tensor on the hot path.
"""

from __future__ import annotations

import math
import os
from typing import Optional

import torch
import torch.nn as nn
import torch.distributed as dist

from .. import ops as _ops
from .functional import (
    sigmoid_contrastive_loss,
    chunk_loss_fwd,
    chunk_loss_bwd,
)
from .id_labels import sigmoid_contrastive_loss_ids
from ..parallel.collectives import all_gather_with_grad, _backend_is_gloo
from ..parallel.ring import (
    neighbour_exchange_with_grad,
    neighbour_exchange_bidir_with_grad,
    hop_span,
    walk_ring,
)


def _world_and_rank(group=None):
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(group), dist.get_rank(group)
    return 1, 0


class _PlainWire:
    """Ring wire format of the bf16 / mixed policies: the chunk itself."""

    def pack(self, ztxt):
        return (ztxt,)

    def qcache(self, payload):
        return None

    def unpack(self, payload):
        return payload[0], None


class _Fp8Wire:
    """Ring wire format of the fp8 policy: ``(e4m3 codes, (1,) fp32 scale)``.

    Every shard is quantized ONCE, by its owner — half the xGMI bytes per hop
    versus bf16, and every rank computes with the exact quantized values the
    owner produced.  The image side is quantized once, here, and shared by
    every chunk's :class:`ops.QuantCache`.
    """

    def __init__(self, zimg):
        self.zi_q, self.si = _ops._quant_fp8(zimg)
        self.dtype = zimg.dtype

    def pack(self, ztxt):
        zt_q, st = _ops._quant_fp8(ztxt)
        return (zt_q, st.reshape(1).float())

    def qcache(self, payload):
        zt_q, st = payload
        return _ops.QuantCache(self.zi_q, zt_q, self.si, st.reshape(()))

    def unpack(self, payload):
        zt_q, st = payload
        chunk = (zt_q.to(torch.float32) * st).to(self.dtype)
        return chunk, self.qcache(payload)


class _RingChunks:
    """One rank's share of the ring loss: its image block against the text
    chunks of all ``world`` ranks, added one by one as they arrive.  Plain
    Python — no autograd, no process group.

    ``regime`` (fixed at construction) says what forward keeps for backward:

    - ``"slab"`` — bf16/mixed saved-g: every chunk's fwd+g kernel writes its
      dL/dlogit block into ONE ``(b, W·b)`` slab (column offset = source
      rank; mixed also the ``gᵀ`` slab) and accumulates into one scalar
      buffer, so backward is pure GEMMs over the concatenated text.
    - ``"chunk_slabs"`` — fp8 saved-g: the text scales differ per chunk, so
      each chunk keeps its own g slab and scalars; ``gᵀ`` is still one slab
      (the image side has one scale).
    - ``"chunk_recompute"`` — fp8 on GPU without saved g: backward recomputes
      chunk by chunk.  Both fp8 regimes reuse the forward's per-source
      quantization — fwd and bwd must see the same quantized values.
    - ``"concat_recompute"`` — everything else (incl. CPU): one recompute
      backward over the concatenated text block.
    """

    _META = ("world", "rank", "b_txt", "quant", "col_chunk", "impl", "regime")
    # Tensor state by field name: single tensors, and lists indexed by source
    # rank.  Unused fields stay None and are not saved.
    _ONE = ("zimg", "t_prime", "bias", "g", "gt", "out3", "zi_q", "si")
    _PER_SRC = ("chunks", "g_chunks", "out3s", "zt_qs", "sts")

    def __init__(self, zimg, t_prime, bias, world, rank, b_txt, quant,
                 col_chunk, impl, want_grad):
        self._restore({}, world=world, rank=rank, b_txt=b_txt, quant=quant,
                      col_chunk=col_chunk, impl=impl, regime=None)
        self.zimg, self.t_prime, self.bias = zimg, t_prime, bias
        b_img, n = zimg.shape[0], world * b_txt
        on_gpu = zimg.is_cuda and impl != "torch"
        # want_grad comes from the caller (grad mode is off inside
        # Function.forward).
        save_g = (on_gpu and col_chunk is None and want_grad
                  and _ops.extension_available()
                  and _ops.save_g_enabled(b_img, n, quant))
        if save_g:
            self.regime = "chunk_slabs" if quant == "fp8" else "slab"
            g_dtype = (torch.bfloat16 if quant == "bf16"
                       else torch.float8_e4m3fn)
            if quant != "fp8":
                self.g = torch.empty((b_img, n), device=zimg.device,
                                     dtype=g_dtype)
                self.out3 = _ops._out_buf(zimg.device)
            if quant != "bf16":
                self.gt = torch.empty((n, b_img), device=zimg.device,
                                      dtype=g_dtype)
        elif quant == "fp8" and on_gpu:
            self.regime = "chunk_recompute"
        else:
            self.regime = "concat_recompute"

    def _restore(self, named, **meta):
        self.__dict__.update(meta)
        for k in self._ONE:
            setattr(self, k, named.get(k))
        for k in self._PER_SRC:
            setattr(self, k, [named.get(f"{k}.{s}")
                              for s in range(self.world)])
        self._loss = None

    def tensors(self) -> dict:
        """The populated tensor fields by name, per-source ones as
        ``field.src`` (``save_for_backward`` the values, keep the keys)."""
        named = {k: getattr(self, k) for k in self._ONE}
        for k in self._PER_SRC:
            named.update({f"{k}.{s}": t
                          for s, t in enumerate(getattr(self, k))})
        return {k: t for k, t in named.items() if t is not None}

    def meta(self) -> dict:
        return {k: getattr(self, k) for k in self._META}

    @classmethod
    def from_tensors(cls, named, **meta) -> "_RingChunks":
        """Inverse of :meth:`tensors` + :meth:`meta`, for backward."""
        self = cls.__new__(cls)
        self._restore(named, **meta)
        return self

    def _qc(self, src):
        return _ops.QuantCache(self.zi_q, self.zt_qs[src], self.si,
                               self.sts[src])

    def add(self, src, chunk, qc, diag):
        """Run the loss kernel of source rank ``src``'s text ``chunk`` (``qc``:
        its fp8 QuantCache or None; ``diag``: 0 for the own block, None for a
        negatives-only remote one)."""
        self.chunks[src] = chunk
        if self.regime in ("chunk_slabs", "chunk_recompute"):
            # the image side is shared: kept once, not per source
            self.zi_q, self.si = qc.zi_q, qc.si
            self.zt_qs[src], self.sts[src] = qc.zt_q, qc.st
        args = (self.zimg, chunk, self.t_prime, self.bias, diag)
        col0 = src * self.b_txt
        if self.regime == "slab":
            _ops.siglip_fwd_g(*args, quant=self.quant, g_slab=self.g,
                              gt_slab=self.gt, col0=col0, out3=self.out3)
        elif self.regime == "chunk_slabs":
            self.out3s[src], self.g_chunks[src], _ = _ops.siglip_fwd_g(
                *args, quant=self.quant, qcache=qc, gt_slab=self.gt,
                col0=col0)
        else:
            part = chunk_loss_fwd(*args, col_chunk=self.col_chunk,
                                  impl=self.impl, quant=self.quant, qcache=qc)
            self._loss = part if self._loss is None else self._loss + part

    def loss(self):
        """Finish the forward (call once, after the last ``add``): reduce the
        per-XCD scalar buffers every chunk's kernel accumulated into."""
        if self.regime == "slab":
            self.out3 = _ops.reduce_out3(self.out3)
            return self.out3[0].clone()
        if self.regime == "chunk_slabs":
            self.out3s = [_ops.reduce_out3(o) for o in self.out3s]
            return sum(o[0] for o in self.out3s).clone()
        return self._loss

    def grads(self, grad_output, on_dztxt):
        """``(dzimg, dtxt_flat, dt_prime, dbias)`` with ``dtxt_flat`` the
        ``(W·b, d)`` gradient of ALL ranks' text, rows in source-rank order;
        ``on_dztxt(dtxt_flat)`` fires as soon as it exists, before the
        image-gradient GEMM."""
        zimg, t_prime, bias = self.zimg, self.t_prime, self.bias
        world, b, quant = self.world, self.b_txt, self.quant
        if self.regime == "chunk_slabs":
            return _ops.siglip_bwd_from_g_chunks(
                zimg, self.chunks, t_prime, bias, grad_output, self.out3s,
                self.g_chunks, self.gt, [self._qc(s) for s in range(world)],
                on_dztxt=on_dztxt)
        if self.regime == "chunk_recompute":
            dzimg_acc = torch.zeros_like(zimg, dtype=torch.float32)
            dtxt_flat = torch.empty((world * b, zimg.shape[1]),
                                    device=zimg.device, dtype=zimg.dtype)
            dt_prime = dbias = 0
            for src in range(world):
                dzi, dzt, dtp, dbs = chunk_loss_bwd(
                    zimg, self.chunks[src], t_prime, bias,
                    0 if src == self.rank else None, grad_output,
                    col_chunk=self.col_chunk, impl=self.impl, quant=quant,
                    qcache=self._qc(src))
                dzimg_acc += dzi.float()
                dtxt_flat[src * b:(src + 1) * b] = dzt
                dt_prime, dbias = dt_prime + dtp, dbias + dbs
            on_dztxt(dtxt_flat)
            return dzimg_acc.to(zimg.dtype), dtxt_flat, dt_prime, dbias
        # One (W·b, d) text block: identical math to per-chunk calls, with
        # the diagonal at the own-rank block.
        all_txt = (self.chunks[0] if world == 1
                   else torch.cat(self.chunks, dim=0))
        if self.regime == "slab":
            # mixed: g came from exact bf16 logits; quantization only
            # compresses the grad GEMM operands — one pass here.
            qc = (_ops.quantize_fp8_pair(zimg, all_txt)
                  if quant == "mixed" else None)
            return _ops.siglip_bwd_from_g(
                zimg, all_txt, t_prime, bias, grad_output, self.out3, self.g,
                self.gt, quant=quant, qcache=qc, on_dztxt=on_dztxt)
        return chunk_loss_bwd(
            zimg, all_txt, t_prime, bias, self.rank * b, grad_output,
            col_chunk=self.col_chunk, impl=self.impl, quant=quant,
            on_dztxt=on_dztxt)


class _RingAllGatherLoss(torch.autograd.Function):
    """Fused distributed loss: ring-pipelined forward, reduce-scatter backward.

    Forward walks the text shards around a P2P ring (``parallel.ring``); the
    exchange of the next chunk is posted *before* the loss kernel for the
    current one runs, so on RCCL the wire time hides under the MFMA compute
    (the reference serializes these — ``distributed_utils.py:25-26``).  What
    travels is the wire format's payload (:class:`_PlainWire` /
    :class:`_Fp8Wire`); the per-chunk compute and everything kept for
    backward — all received shards included, so backward never
    re-communicates embeddings — belong to :class:`_RingChunks`.

    Backward produces the full text-gradient block and issues ONE
    ``reduce_scatter_tensor(SUM)`` — the algebraic collapse of the
    reference's W−1 reversed autograd ring hops
    (``distributed_utils.py:74-77``) into a single RCCL collective —
    launched async from the ``on_dztxt`` hook so its wire time overlaps the
    remaining image-gradient GEMM.

    Gradient semantics match the differentiable all-gather strategy exactly:
    raw per-rank grads already carry full cross-rank contributions (what the
    reference's strategy-equivalence oracle asserts,
    ``test_sigmoid_loss_variants.py:112-113``).
    """

    @staticmethod
    def forward(ctx, zimg, ztxt, t_prime, bias, group, col_chunk, impl,
                quant, want_grad, bidir=False):
        world, rank = _world_and_rank(group)
        zimg = zimg.contiguous()
        ztxt = ztxt.contiguous()
        wire = _Fp8Wire(zimg) if quant == "fp8" else _PlainWire()
        own = wire.pack(ztxt)
        acc = _RingChunks(zimg, t_prime, bias, world, rank, ztxt.shape[0],
                          quant, col_chunk, impl, want_grad)
        ring = walk_ring(own, world, rank, bidir, group)
        next(ring)      # hop 1 is on the wire before the local-block kernel
        acc.add(rank, ztxt, wire.qcache(own), 0)
        for label, arrived in ring:
            # hop k+1 is already posted; these kernels hide its wire time
            got = [(src,) + wire.unpack(payload) for src, payload in arrived]
            with hop_span(label):
                for src, chunk, qc in got:
                    acc.add(src, chunk, qc, None)
        loss = acc.loss()
        named = acc.tensors()
        ctx.save_for_backward(*named.values())
        ctx.names = tuple(named)
        ctx.meta = acc.meta()
        ctx.group = group
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        acc = _RingChunks.from_tensors(
            dict(zip(ctx.names, ctx.saved_tensors)), **ctx.meta)
        world, rank, b = acc.world, acc.rank, acc.b_txt

        # The cross-rank reduce-scatter is launched ASYNC from the on_dztxt
        # hook, so its xGMI wire time overlaps the dzimg gradient GEMM(s)
        # still running on the compute stream.
        gloo = world > 1 and _backend_is_gloo(ctx.group)
        pending = []

        def on_dztxt(flat):
            if world == 1:
                return
            if gloo:    # no reduce-scatter: all-reduce, keep the own slice
                out = flat[rank * b:(rank + 1) * b]
                work = dist.all_reduce(flat, op=dist.ReduceOp.SUM,
                                       group=ctx.group, async_op=True)
            else:
                out = torch.empty_like(flat[:b])
                work = dist.reduce_scatter_tensor(
                    out, flat, op=dist.ReduceOp.SUM, group=ctx.group,
                    async_op=True)
            pending.append((work, out))

        dzimg, dztxt, dt_prime, dbias = acc.grads(grad_output, on_dztxt)
        for work, out in pending:
            work.wait()
            dztxt = out.clone() if gloo else out
        return (dzimg, dztxt, dt_prime, dbias, None, None, None, None, None,
                None)


class DistributedSigmoidLoss(nn.Module):
    """All-rank distributed sigmoid contrastive loss with module-owned params.

    Parity with reference ``DDPSigmoidLoss`` (``distributed_sigmoid_loss.py``):
    ``t_prime`` init ``log(10)``, ``bias`` init ``−10.0`` (``:11-12``); forward
    all-gathers the text shard, computes ``−logsigmoid(l·z)`` over the local
    ``(b, W·b)`` pair grid (labels ``+1`` on the rank-diagonal block's
    diagonal, ``−1`` elsewhere) and divides by the *local* ``gpu_batch_size``
    (``:47``).  Under DDP grad averaging this reproduces single-rank
    ``sum/(W·b)`` normalization exactly.

    ``strategy``:
        - ``"all_gather"`` — differentiable all-gather (one RCCL all-gather
          fwd, one reduce-scatter bwd), then ONE fused kernel call over the
          whole ``(b, W·b)`` block.
        - ``"ring"`` — pipelined P2P ring (xGMI point-to-point) with
          comm/compute overlap and reduce-scatter backward.

    Sample-ID labels: ``forward(..., image_ids=, text_ids=)`` (both or
    neither; int64 ``(b,)`` each) replaces the positional labels by
    ``sigmoid_contrastive_loss_ids`` — ids equal: positive
    (``duplicates="positive"``), or the position stays the only positive and
    other pairs with equal ids are ignored (``"ignore"``); a negative id
    masks its row / column.  The text ids are all-gathered next to the text
    shard and the ``(b, W·b)`` grid is one call with ``diag_offset =
    rank·b``.  Supported with ``strategy="all_gather"`` (or any strategy at
    ``W = 1``) and ``quant="bf16"``; anything else raises.  The result is
    still divided by ``gpu_batch_size`` — not by the number of unmasked rows
    — so a batch with masked rows weighs less, it is not renormalised.

    Works with DistributedDataParallel (DDP) only (not DataParallel); pass
    ``t_prime``/``bias`` to your optimizer like any other parameter
    (reference ``README.md:19-20``).
    """

    def __init__(self, gpu_batch_size: int, strategy: str = "all_gather",
                 col_chunk: Optional[int] = None, impl: str = "auto",
                 quant: str = "bf16", bidir: Optional[bool] = None):
        super().__init__()
        self.t_prime = nn.Parameter(torch.tensor(math.log(10.0)))
        self.bias = nn.Parameter(torch.tensor(-10.0))
        self.gpu_batch_size = gpu_batch_size
        if strategy not in ("all_gather", "ring"):
            raise ValueError(f"unknown strategy {strategy!r}")
        if quant not in ("bf16", "fp8", "mixed"):
            raise ValueError(f"unknown quant {quant!r}")
        self.strategy = strategy
        self.col_chunk = col_chunk
        self.impl = impl
        self.quant = quant
        # Ring hop-halving via two simultaneous xGMI links (W > 2 only).
        # Default on; SIGLIP_RING_BIDIR=0 (or bidir=False) forces the
        # unidirectional ring for A/B comparison.
        if bidir is None:
            bidir = os.environ.get("SIGLIP_RING_BIDIR", "1") != "0"
        self.bidir = bidir
        if quant in ("fp8", "mixed") and torch.cuda.is_available():
            from .. import ops as _ops
            _ops.load_tuned_gemms()

    def _forward_ids(self, image_embeddings, text_embeddings, group,
                     image_ids, text_ids, duplicates):
        world, rank = _world_and_rank(group)
        if self.quant != "bf16" or (self.strategy == "ring" and world > 1):
            raise ValueError(
                "sample-ID labels are supported with strategy='all_gather' "
                "(or a single rank) and quant='bf16' (got strategy="
                f"{self.strategy!r}, quant={self.quant!r}, world={world})")
        b_txt = text_embeddings.shape[0]
        text_ids = text_ids.to(device=text_embeddings.device,
                               dtype=torch.int64).contiguous()
        all_txt = all_gather_with_grad(text_embeddings, group=group)
        all_ids = text_ids
        if world > 1:
            all_ids = torch.empty(world * b_txt, device=text_ids.device,
                                  dtype=torch.int64)
            dist.all_gather_into_tensor(all_ids, text_ids, group=group)
        total = sigmoid_contrastive_loss_ids(
            image_embeddings, all_txt, self.t_prime, self.bias, image_ids,
            all_ids, duplicates=duplicates, diag_offset=rank * b_txt,
            col_chunk=self.col_chunk, impl=self.impl)
        return total / self.gpu_batch_size

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
        world, rank = _world_and_rank(group)
        b_txt = text_embeddings.shape[0]
        if self.strategy == "all_gather" or world == 1:
            all_txt = all_gather_with_grad(text_embeddings, group=group)
            total = sigmoid_contrastive_loss(
                image_embeddings, all_txt, self.t_prime, self.bias,
                diag_offset=rank * b_txt, col_chunk=self.col_chunk,
                impl=self.impl, quant=self.quant)
        else:
            want_grad = torch.is_grad_enabled() and any(
                t.requires_grad for t in (image_embeddings, text_embeddings,
                                          self.t_prime, self.bias))
            total = _RingAllGatherLoss.apply(
                image_embeddings, text_embeddings, self.t_prime, self.bias,
                group, self.col_chunk, self.impl, self.quant, want_grad,
                self.bidir)
        return total / self.gpu_batch_size


class SigLipLoss(nn.Module):
    """Ring-strategy SigLIP loss with caller-owned scale/bias parameters.

    Parity with the open_clip-style reference (``rwightman_sigmoid_loss.py``):
    local positive block first (``:69``), then ``W−1`` ring hops —
    bidirectional pairs plus one unidirectional remainder when ``bidir``
    (``:77-107``), else a pure unidirectional ring (``:108-122``) — each
    remote chunk contributing negatives-only loss, every chunk normalized by
    the local batch size (``:65``).  Gradients hop home through the
    autograd-reversed exchanges.

    ``use_horovod`` is unsupported, as in the reference (``:35``).
    """

    def __init__(self, cache_labels: bool = False, rank: int = 0,
                 world_size: int = 1, bidir: bool = True,
                 use_horovod: bool = False, impl: str = "auto",
                 col_chunk: Optional[int] = None):
        super().__init__()
        if use_horovod:
            raise NotImplementedError("horovod is not supported")
        self.cache_labels = cache_labels  # kept for API parity; predicate labels need no cache
        self.rank = rank
        self.world_size = world_size
        self.bidir = bidir
        self.use_horovod = use_horovod
        self.impl = impl
        self.col_chunk = col_chunk

    def get_ground_truth(self, device, dtype, num_logits,
                         negative_only=False) -> torch.Tensor:
        """Materialized ±1 label block — API parity with the reference
        (``rwightman_sigmoid_loss.py:43-47``).  The fused path never calls
        this (labels are an index predicate); it exists for users porting
        code that consumes it."""
        labels = -torch.ones((num_logits, num_logits), device=device,
                             dtype=dtype)
        if not negative_only:
            labels = 2 * torch.eye(num_logits, device=device,
                                   dtype=dtype) + labels
        return labels

    def get_logits(self, image_features, text_features, logit_scale,
                   logit_bias=None):
        """Pairwise logits — API parity with the reference
        (``rwightman_sigmoid_loss.py:49-53``)."""
        logits = logit_scale.exp() * image_features @ text_features.T
        if logit_bias is not None:
            logits = logits + logit_bias
        return logits

    def _loss(self, image_features, text_features, logit_scale, logit_bias,
              negative_only=False):
        off = None if negative_only else 0
        total = sigmoid_contrastive_loss(
            image_features, text_features, logit_scale, logit_bias,
            diag_offset=off, col_chunk=self.col_chunk, impl=self.impl)
        return total / image_features.shape[0]

    def forward(self, image_features, text_features, logit_scale, logit_bias,
                output_dict: bool = False):
        loss = self._loss(image_features, text_features, logit_scale,
                          logit_bias)

        if self.world_size > 1:
            right_rank = (self.rank + 1) % self.world_size
            left_rank = (self.rank - 1 + self.world_size) % self.world_size
            if self.bidir:
                to_right = to_left = text_features
                num_bidir, remainder = divmod(self.world_size - 1, 2)
                for _ in range(num_bidir):
                    recv = neighbour_exchange_bidir_with_grad(
                        left_rank, right_rank, to_left, to_right)
                    for f in recv:
                        loss = loss + self._loss(image_features, f,
                                                 logit_scale, logit_bias,
                                                 negative_only=True)
                    to_left, to_right = recv
                if remainder:
                    recv = neighbour_exchange_with_grad(
                        left_rank, right_rank, to_right)
                    loss = loss + self._loss(image_features, recv,
                                             logit_scale, logit_bias,
                                             negative_only=True)
            else:
                to_right = text_features
                for _ in range(self.world_size - 1):
                    from_left = neighbour_exchange_with_grad(
                        left_rank, right_rank, to_right)
                    loss = loss + self._loss(image_features, from_left,
                                             logit_scale, logit_bias,
                                             negative_only=True)
                    to_right = from_left

        return {"contrastive_loss": loss} if output_dict else loss
