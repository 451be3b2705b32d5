"""Retrieval ranks and recall@k over the image×text pair grid.

The loss is a poor quality signal at the SigLIP initialisation (a negative
pair carries under 1 % of it); the number people read for an image–text model
is the rank of the matching pair, reported as recall@k in both directions.
For a block ``zimg (b, d)`` × ``ztxt (n, d)`` with ``s_ij = <zimg_i, ztxt_j>``
and the positive of row ``i`` at column ``i + diag_offset``:

    rank_i2t[i] = #{ j ≠ i+off : s_ij > s_{i,i+off} }
    rank_t2i[j] = #{ i ≠ j−off : s_ij > s_{j−off,j} }

(strict ``>``: a tie does not count against the positive; ``-1`` where the
positive lies outside the block).  Temperature and bias are a monotone map of
``s``, so ranks do not depend on them and nothing here takes them.  Inputs
need not be normalised.  Nothing here is differentiable.

On GPU the counts come from the fused HIP kernel (``ops.pair_rank_counts``):
one MFMA pass over the grid, the ``(b, n)`` logits never reach memory.  Counts
are integers and add over column chunks and over ranks, so the same kernel
serves the single-device and the all-gathered distributed case, and results
are bitwise reproducible.

Retrieval itself — which partners score highest, and how high — is
:func:`pair_topk`: for every row the ``k`` best candidates ``j ≠ i +
diag_offset`` in the total order "higher score first, among equal scores the
lower column first", ``(−inf, −1)`` once the candidates run out.  With the
positive excluded these are the row's hardest negatives.  The order is total,
so results are bitwise reproducible and :func:`merge_topk` of results over
disjoint column chunks equals the single call.  On GPU the lists come from
the fused HIP kernel (``ops.pair_topk``) in one pass over the grid;
:func:`retrieval_topk` runs both directions, :func:`distributed_retrieval_topk`
the global batch.
"""

from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence

import torch
import torch.distributed as dist

from ..parallel.collectives import _backend_is_gloo, all_gather_with_grad

_TORCH_ROW_CHUNK = 1024


class RetrievalRanks(NamedTuple):
    """int64 ranks, ``-1`` where there is no positive: ``i2t`` ``(b,)`` per
    image, ``t2i`` ``(n,)`` per text."""
    i2t: torch.Tensor
    t2i: torch.Tensor


def _compute_dtype(x: torch.Tensor) -> torch.dtype:
    return torch.float64 if x.dtype == torch.float64 else torch.float32


def _check_side(name, thr, cnt, length, device):
    if thr is None:
        if cnt is not None:
            raise RuntimeError(f"{name}_cnt given without {name}_thr")
        return None
    if thr.shape != (length,):
        raise RuntimeError(
            f"{name}_thr must have shape ({length},), got {tuple(thr.shape)}")
    if cnt is None:
        return torch.zeros(length, device=device, dtype=torch.int32)
    if cnt.shape != (length,) or cnt.dtype != torch.int32:
        raise RuntimeError(
            f"{name}_cnt must be int32 of shape ({length},), got "
            f"{cnt.dtype} {tuple(cnt.shape)}")
    return cnt


def _torch_pair_rank_counts(zimg, ztxt, row_thr, col_thr, diag_offset,
                            row_cnt, col_cnt, row_chunk=_TORCH_ROW_CHUNK):
    """Row-chunked torch composite: holds ``O(row_chunk · n)`` scores at a
    time.  fp32 compute for bf16/fp16/fp32 inputs, fp64 for fp64."""
    b, n = zimg.shape[0], ztxt.shape[0]
    dev = zimg.device
    cdt = _compute_dtype(zimg)
    row_cnt = _check_side("row", row_thr, row_cnt, b, dev)
    col_cnt = _check_side("col", col_thr, col_cnt, n, dev)
    if row_cnt is None and col_cnt is None:
        return None, None
    zt = ztxt.detach().to(cdt)
    cols = torch.arange(n, device=dev)
    rthr = None if row_thr is None else row_thr.detach().to(cdt)
    cthr = None if col_thr is None else col_thr.detach().to(cdt)
    for r0 in range(0, b, max(1, int(row_chunk))):
        r1 = min(b, r0 + max(1, int(row_chunk)))
        s = zimg[r0:r1].detach().to(cdt) @ zt.T
        if diag_offset is not None:
            pos = torch.arange(r0, r1, device=dev) + int(diag_offset)
            s.masked_fill_(cols[None, :] == pos[:, None], -math.inf)
        if rthr is not None:
            row_cnt[r0:r1] += (s > rthr[r0:r1, None]).sum(1, dtype=torch.int32)
        if cthr is not None:
            col_cnt += (s > cthr[None, :]).sum(0, dtype=torch.int32)
    return row_cnt, col_cnt


def pair_rank_counts(zimg: torch.Tensor, ztxt: torch.Tensor,
                     row_thr: Optional[torch.Tensor] = None,
                     col_thr: Optional[torch.Tensor] = None,
                     diag_offset: Optional[int] = None,
                     row_cnt: Optional[torch.Tensor] = None,
                     col_cnt: Optional[torch.Tensor] = None,
                     impl: str = "auto"):
    """Threshold counts over the score grid → ``(row_cnt | None, col_cnt |
    None)``, int32:

    ``row_cnt[i] += #{j ≠ i+diag_offset : s_ij > row_thr[i]}``,
    ``col_cnt[j] += #{i ≠ j−diag_offset : s_ij > col_thr[j]}``.

    ``diag_offset=None`` excludes nothing.  A side without a threshold is
    skipped.  Counts are added into ``row_cnt`` / ``col_cnt`` when given (the
    caller zeroes them) and start from fresh zeros otherwise, so calls over
    column chunks ``ztxt[j0:j1]`` with ``diag_offset − j0`` accumulate.

    ``impl``: ``auto`` (``hip`` on GPU, ``torch`` on CPU) | ``hip`` (bf16
    embeddings, ``d % 8 == 0``, fp32 thresholds; raises without the built
    extension) | ``torch`` (row-chunked composite).
    """
    if zimg.dim() != 2 or ztxt.dim() != 2 or zimg.shape[1] != ztxt.shape[1]:
        raise RuntimeError(
            f"expected (b, d) and (n, d) embeddings, got "
            f"{tuple(zimg.shape)} and {tuple(ztxt.shape)}")
    if impl == "auto":
        impl = "hip" if zimg.is_cuda else "torch"
    if impl == "hip":
        from .. import ops
        return ops.pair_rank_counts(zimg, ztxt, row_thr, col_thr, diag_offset,
                                    row_cnt, col_cnt)
    if impl == "torch":
        return _torch_pair_rank_counts(zimg, ztxt, row_thr, col_thr,
                                       diag_offset, row_cnt, col_cnt)
    raise ValueError(f"unknown impl {impl!r}")


def _positive_rows(b: int, n: int, diag_offset: Optional[int], device):
    """Rows of the block that have a positive, and those positives' columns."""
    if diag_offset is None:
        empty = torch.empty(0, dtype=torch.long, device=device)
        return empty, empty
    off = int(diag_offset)
    lo, hi = max(0, -off), min(b, n - off)
    rows = torch.arange(lo, max(lo, hi), device=device)
    return rows, rows + off


def positive_scores(zimg: torch.Tensor, ztxt: torch.Tensor,
                    diag_offset: Optional[int] = 0) -> torch.Tensor:
    """``(b,)`` scores of the positive pairs ``<zimg_i, ztxt_{i+diag_offset}>``
    and ``+inf`` where the positive lies outside the block.  fp32 (fp64 for
    fp64 inputs); ``O(b · d)``."""
    b, n = zimg.shape[0], ztxt.shape[0]
    cdt = _compute_dtype(zimg)
    out = torch.full((b,), math.inf, device=zimg.device, dtype=cdt)
    rows, cols = _positive_rows(b, n, diag_offset, zimg.device)
    if rows.numel():
        out[rows] = (zimg.detach()[rows].to(cdt)
                     * ztxt.detach()[cols].to(cdt)).sum(-1)
    return out


def retrieval_ranks(zimg: torch.Tensor, ztxt: torch.Tensor,
                    diag_offset: Optional[int] = 0,
                    impl: str = "auto") -> RetrievalRanks:
    """Retrieval rank of every matching pair in both directions: for image
    ``i`` the number of texts that score above its own text, for text ``j``
    the number of images that score above its own image.  One
    :func:`pair_rank_counts` pass over the whole grid, thresholded at
    :func:`positive_scores`."""
    b, n = zimg.shape[0], ztxt.shape[0]
    dev = zimg.device
    pos = positive_scores(zimg, ztxt, diag_offset)
    rows, cols = _positive_rows(b, n, diag_offset, dev)
    col_thr = torch.full((n,), math.inf, device=dev, dtype=pos.dtype)
    col_thr[cols] = pos[rows]
    row_cnt, col_cnt = pair_rank_counts(zimg, ztxt, pos, col_thr, diag_offset,
                                        impl=impl)
    i2t = torch.full((b,), -1, device=dev, dtype=torch.long)
    t2i = torch.full((n,), -1, device=dev, dtype=torch.long)
    i2t[rows] = row_cnt[rows].long()
    t2i[cols] = col_cnt[cols].long()
    return RetrievalRanks(i2t, t2i)


def recall_at_k(ranks: torch.Tensor, ks: Sequence[int] = (1, 5, 10)) -> dict:
    """``{"R@k": fraction of entries with 0 ≤ rank < k}`` among the entries
    that have a positive (``rank ≥ 0``); ``nan`` when there are none."""
    valid = ranks[ranks >= 0]
    if valid.numel() == 0:
        return {f"R@{k}": float("nan") for k in ks}
    return {f"R@{k}": float((valid < k).double().mean()) for k in ks}


def distributed_retrieval_ranks(zimg: torch.Tensor, ztxt: torch.Tensor,
                                group=None,
                                impl: str = "auto") -> RetrievalRanks:
    """Ranks of this rank's ``b`` images against all ``W·b`` texts and of its
    ``b`` texts against all ``W·b`` images (equal ``b`` on every rank; the
    positive of local image ``i`` is local text ``i``).

    The text shard and the local positive scores are all-gathered; one
    :func:`pair_rank_counts` pass over the ``(b, W·b)`` block with
    ``diag_offset = rank·b`` completes ``i2t`` and yields this rank's share of
    every text's count; the shares are summed across ranks (integers, so the
    order is irrelevant) and the local slice kept.  World size 1 is
    :func:`retrieval_ranks`."""
    if (not dist.is_available() or not dist.is_initialized()
            or dist.get_world_size(group) == 1):
        return retrieval_ranks(zimg, ztxt, 0, impl=impl)
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    b = zimg.shape[0]
    if ztxt.shape[0] != b:
        raise RuntimeError("distributed_retrieval_ranks needs paired shards")
    with torch.no_grad():
        pos = positive_scores(zimg, ztxt, 0)
        zt_all = all_gather_with_grad(ztxt.detach(), group)
        pos_all = all_gather_with_grad(pos, group)
        row_cnt, col_cnt = pair_rank_counts(zimg, zt_all, pos, pos_all,
                                            rank * b, impl=impl)
        if _backend_is_gloo(group):
            dist.all_reduce(col_cnt, op=dist.ReduceOp.SUM, group=group)
            local = col_cnt[rank * b:(rank + 1) * b]
        else:
            local = torch.empty(b, device=col_cnt.device, dtype=col_cnt.dtype)
            dist.reduce_scatter_tensor(local, col_cnt, op=dist.ReduceOp.SUM,
                                       group=group)
    return RetrievalRanks(row_cnt.long(), local.long())


class TopK(NamedTuple):
    """``scores`` ``(rows, k)`` (fp32; fp64 for fp64 inputs), best first, and
    int64 ``indices`` ``(rows, k)``; ``(−inf, −1)`` in the slots past the
    last candidate."""
    scores: torch.Tensor
    indices: torch.Tensor


def _torch_pair_topk(zimg, ztxt, k, diag_offset, row_chunk=_TORCH_ROW_CHUNK):
    """Row-chunked torch composite with the contract of the kernel, the tie
    rule included (a stable descending sort keeps the lower column first)."""
    b, n = zimg.shape[0], ztxt.shape[0]
    dev = zimg.device
    cdt = _compute_dtype(zimg)
    scores = torch.full((b, k), -math.inf, device=dev, dtype=cdt)
    cols = torch.full((b, k), -1, device=dev, dtype=torch.long)
    kk = min(k, n)
    zt = ztxt.detach().to(cdt)
    col_ids = torch.arange(n, device=dev)
    for r0 in range(0, b, max(1, int(row_chunk))):
        r1 = min(b, r0 + max(1, int(row_chunk)))
        s = zimg[r0:r1].detach().to(cdt) @ zt.T
        pos = None
        if diag_offset is not None:
            pos = torch.arange(r0, r1, device=dev) + int(diag_offset)
            s.masked_fill_(col_ids[None, :] == pos[:, None], -math.inf)
        top_s, top_c = torch.sort(s, dim=1, descending=True, stable=True)
        top_s, top_c = top_s[:, :kk].clone(), top_c[:, :kk].clone()
        if pos is not None:
            # The excluded column sorts behind every candidate; it shows up
            # only where the candidates ran out.
            gone = top_c == pos[:, None]
            top_s[gone] = -math.inf
            top_c[gone] = -1
        scores[r0:r1, :kk] = top_s
        cols[r0:r1, :kk] = top_c
    return scores, cols


def pair_topk(zimg: torch.Tensor, ztxt: torch.Tensor, k: int,
              diag_offset: Optional[int] = None, col_base: int = 0,
              impl: str = "auto") -> TopK:
    """The ``k`` best scoring columns of every row of the score grid.

    The candidates of row ``i`` are the columns ``j`` of ``ztxt`` with ``j ≠
    i + diag_offset`` (``None``: all columns), ordered by higher score first
    and, among equal scores, lower column first (``+0`` equals ``−0``); slot
    ``q`` holds the ``q``-th candidate and ``(−inf, −1)`` past the last one.
    Indices are ``column + col_base``.  No autograd.

    ``impl``: ``auto`` (``hip`` on GPU for bf16 inputs and ``k`` within the
    kernel's range, ``torch`` otherwise) | ``hip`` (bf16, ``d % 8 == 0``,
    ``k ≤ ops.pair_topk_max_k()``; raises otherwise) | ``torch`` (row-chunked
    composite, any ``k``).
    """
    if zimg.dim() != 2 or ztxt.dim() != 2 or zimg.shape[1] != ztxt.shape[1]:
        raise RuntimeError(
            f"expected (b, d) and (n, d) embeddings, got "
            f"{tuple(zimg.shape)} and {tuple(ztxt.shape)}")
    k = int(k)
    if k < 1:
        raise ValueError(f"k must be at least 1, got {k}")
    if impl == "auto":
        impl = "torch"
        if (zimg.is_cuda and zimg.dtype == torch.bfloat16
                and ztxt.dtype == torch.bfloat16):
            from .. import ops
            if k <= ops.pair_topk_max_k():
                impl = "hip"
    if impl == "hip":
        from .. import ops
        scores, cols = ops.pair_topk(zimg, ztxt, k, diag_offset)
        cols = cols.long()
    elif impl == "torch":
        if zimg.shape[0] < 1 or ztxt.shape[0] < 1:
            raise RuntimeError("pair_topk needs a non-empty block")
        scores, cols = _torch_pair_topk(zimg, ztxt, k, diag_offset)
    else:
        raise ValueError(f"unknown impl {impl!r}")
    if col_base:
        cols = torch.where(cols >= 0, cols + int(col_base), cols)
    return TopK(scores, cols)


def merge_topk(parts: Sequence[TopK], k: Optional[int] = None) -> TopK:
    """Merge results over disjoint column sets (same rows, global indices)
    under the same total order; ``−1`` slots are ignored.  ``k`` defaults to
    the first part's.  A chunked call is ``pair_topk(zimg, ztxt[j0:j1], k,
    diag_offset − j0, col_base=j0)`` per chunk and one merge, and equals the
    single call bit for bit."""
    parts = list(parts)
    if not parts:
        raise ValueError("merge_topk needs at least one part")
    k = parts[0].scores.shape[1] if k is None else int(k)
    if k < 1:
        raise ValueError(f"k must be at least 1, got {k}")
    scores = torch.cat([p.scores for p in parts], dim=1)
    idx = torch.cat([p.indices for p in parts], dim=1)
    last = torch.iinfo(torch.long).max
    fill = idx < 0
    key = torch.where(fill, torch.full_like(idx, last), idx)
    sc = scores.masked_fill(fill, -math.inf)
    # Lexicographic (score descending, index ascending): order by the minor
    # key first, then stably by the major one.
    key, o = torch.sort(key, dim=1, stable=True)
    sc = sc.gather(1, o)
    sc, o = torch.sort(sc, dim=1, descending=True, stable=True)
    key = key.gather(1, o)
    out_s = torch.full((sc.shape[0], k), -math.inf, device=sc.device,
                       dtype=sc.dtype)
    out_i = torch.full((sc.shape[0], k), -1, device=sc.device,
                       dtype=torch.long)
    kk = min(k, sc.shape[1])
    out_s[:, :kk] = sc[:, :kk]
    out_i[:, :kk] = torch.where(key[:, :kk] == last,
                                torch.full_like(key[:, :kk], -1),
                                key[:, :kk])
    return TopK(out_s, out_i)


def retrieval_topk(zimg: torch.Tensor, ztxt: torch.Tensor, k: int,
                   diag_offset: Optional[int] = None, impl: str = "auto"):
    """``(i2t, t2i)``: for every image its ``k`` best texts and for every
    text its ``k`` best images (:class:`TopK` each).  With an integer
    ``diag_offset`` the pair ``(i, i + diag_offset)`` is left out on both
    sides — the lists are the hardest negatives; ``None`` is plain
    retrieval.  The text side is the same op with the operands exchanged."""
    i2t = pair_topk(zimg, ztxt, k, diag_offset, impl=impl)
    t2i = pair_topk(ztxt, zimg, k,
                    None if diag_offset is None else -int(diag_offset),
                    impl=impl)
    return i2t, t2i


def distributed_retrieval_topk(zimg: torch.Tensor, ztxt: torch.Tensor, k: int,
                               exclude_positive: bool = False, group=None,
                               impl: str = "auto"):
    """``(i2t, t2i)`` of this rank's ``b`` images against all ``W·b`` texts
    and of its ``b`` texts against all ``W·b`` images, with global indices
    (equal ``b`` on every rank; the positive of local image ``i`` is local
    text ``i``, left out when ``exclude_positive``).

    The text shard is all-gathered for the image side and the image shard for
    the text side; each side is one :func:`pair_topk` pass over a ``(b,
    W·b)`` block and complete on its own, so nothing is reduced.  World size
    1 is :func:`retrieval_topk`."""
    if (not dist.is_available() or not dist.is_initialized()
            or dist.get_world_size(group) == 1):
        return retrieval_topk(zimg, ztxt, k, 0 if exclude_positive else None,
                              impl=impl)
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    b = zimg.shape[0]
    if ztxt.shape[0] != b:
        raise RuntimeError("distributed_retrieval_topk needs paired shards")
    off = rank * b if exclude_positive else None
    with torch.no_grad():
        zt_all = all_gather_with_grad(ztxt.detach(), group)
        i2t = pair_topk(zimg.detach(), zt_all, k, off, impl=impl)
        del zt_all
        zi_all = all_gather_with_grad(zimg.detach(), group)
        t2i = pair_topk(ztxt.detach(), zi_all, k, off, impl=impl)
    return i2t, t2i
