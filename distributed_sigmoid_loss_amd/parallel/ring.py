"""Autograd-correct ring neighbour-exchange primitives over torch.distributed.

Behavioral parity with the reference's L1 layer (``distributed_utils.py:10-106``):
``neighbour_exchange`` / ``neighbour_exchange_bidir`` post paired isend/irecv via
``P2POp`` + ``batch_isend_irecv``; the ``*_with_grad`` autograd wrappers re-send
``grad_output`` along the reversed route in backward, so gradients hop backwards
around the ring one exchange per backward step.

MI355X mapping: with ``init_process_group("nccl")`` on ROCm these P2P ops are
RCCL send/recv over xGMI point-to-point links (7 links × ≈153 GB/s per GPU on an
8-GPU node).  A unidirectional hop uses one link per direction; the bidirectional
variant engages two links simultaneously and halves the hop count to
``⌈(W-1)/2⌉``.  RCCL runs these on its own internal HIP stream, so an exchange
issued *before* the compute on the previously-received chunk overlaps with it
(the reference serializes comm and compute by calling ``req.wait()``
immediately, ``distributed_utils.py:25-26``).

The double-buffered schedule that ``_RingAllGatherLoss`` drives is three pieces
here: :func:`ring_schedule` (whose chunk travels where at each hop — pure),
:func:`exchange_start` (one batched post of tuple payloads) and
:func:`walk_ring` (post hop k+1, then hand hop k's chunks to the caller).
"""

from __future__ import annotations

import contextlib
import os
from typing import NamedTuple, Optional, Sequence

import torch
import torch.distributed as dist

from ..utils.profiling import roctx_range, HopStats

# Debug escape hatch (SURVEY §5 race-detection plan): SIGLIP_SYNC_COMM=1
# makes every exchange complete before returning, serializing comm against
# compute — use to bisect overlap bugs (with HIP_LAUNCH_BLOCKING=1 for
# kernel-side ordering).
_SYNC_COMM = os.environ.get("SIGLIP_SYNC_COMM", "0") == "1"


def set_sync_comm(enabled: bool) -> None:
    global _SYNC_COMM
    _SYNC_COMM = enabled


@contextlib.contextmanager
def hop_span(label: Optional[str]):
    # roctx marker for external profilers + CUDA-event pair for the
    # in-process per-hop stats (SIGLIP_HOP_STATS=1 / bench --csv).
    if label is None:
        yield
        return
    with roctx_range(label), HopStats.record(label):
        yield


class RingHandle:
    """In-flight neighbour exchange: receive buffers plus pending requests.

    Lets callers overlap the wire time with compute: start the exchange, do
    compute on the previous chunk, then ``wait()`` for the received tensors.
    """

    __slots__ = ("_reqs", "_recv", "_done")

    def __init__(self, reqs: Sequence, recv):
        self._reqs = reqs
        self._recv = recv
        self._done = False

    def wait(self):
        if not self._done:
            for r in self._reqs:
                r.wait()
            self._done = True
        return self._recv


def _is_fp8(t: torch.Tensor) -> bool:
    return t.dtype.is_floating_point and t.element_size() == 1


def exchange_start(left_rank: int, right_rank: int, to_right=None,
                   to_left=None, group=None, _result=None) -> RingHandle:
    """Non-blocking exchange of tuple payloads with one or both neighbours.

    ``to_right`` / ``to_left`` are tuples of tensors (or None: nothing travels
    that way).  Every rank of the ring makes the same call, so what is sent
    right arrives from the left with the same shapes, and vice versa.
    ``wait()`` returns ``(from_right, from_left)`` as tuples (empty for an
    unused direction).  float8 tensors ride as their uint8 view — collectives
    do not take float8 dtypes — and come back viewed as float8, bit for bit.

    One ``batch_isend_irecv``: sends (right, then left), then receives (right,
    then left), a payload's tensors in tuple order — ranks match P2P ops by
    order.  (``_result(from_right, from_left)`` reshapes what ``wait()``
    returns, for the reference-parity wrappers below.)
    """
    to_right, to_left = tuple(to_right or ()), tuple(to_left or ())
    nr, nl = len(to_right), len(to_left)
    sends = [t.view(torch.uint8) if _is_fp8(t) else t
             for t in to_right + to_left]
    # from the right comes what the neighbour sent left, and vice versa
    recvs = [torch.empty_like(t) for t in sends[nr:] + sends[:nr]]
    back = [r.view(t.dtype) for r, t in zip(recvs, to_left + to_right)]
    result = (tuple(back[:nl]), tuple(back[nl:]))
    ops = [dist.P2POp(dist.isend, t.contiguous(), peer, group=group)
           for t, peer in zip(sends, [right_rank] * nr + [left_rank] * nl)]
    ops += [dist.P2POp(dist.irecv, t, peer, group=group)
            for t, peer in zip(recvs, [right_rank] * nl + [left_rank] * nr)]
    handle = RingHandle(dist.batch_isend_irecv(ops),
                        _result(*result) if _result else result)
    if _SYNC_COMM:
        handle.wait()
    return handle


def neighbour_exchange(from_rank: int, to_rank: int, tensor: torch.Tensor,
                       group=None) -> torch.Tensor:
    """Blocking one-hop ring exchange: send to ``to_rank``, receive from
    ``from_rank``.  Parity: reference ``distributed_utils.py:10-27``."""
    return neighbour_exchange_start(from_rank, to_rank, tensor,
                                    group=group).wait()[0]


def neighbour_exchange_start(from_rank: int, to_rank: int, tensor: torch.Tensor,
                             group=None) -> RingHandle:
    """Non-blocking variant of :func:`neighbour_exchange` for comm/compute
    overlap; ``wait()`` returns ``[received]``."""
    return exchange_start(from_rank, to_rank, to_right=(tensor,), group=group,
                          _result=lambda r, l: [l[0]])


def neighbour_exchange_bidir(left_rank: int, right_rank: int,
                             tensor_to_left: torch.Tensor,
                             tensor_to_right: torch.Tensor,
                             group=None):
    """Blocking bidirectional exchange (two simultaneous ring hops).

    Returns ``(tensor_from_right, tensor_from_left)`` — same contract as the
    reference (``distributed_utils.py:30-62``).  On an xGMI-connected node the
    two directions ride two distinct point-to-point links.
    """
    return tuple(neighbour_exchange_bidir_start(
        left_rank, right_rank, tensor_to_left, tensor_to_right,
        group=group).wait())


def neighbour_exchange_bidir_start(left_rank: int, right_rank: int,
                                   tensor_to_left: torch.Tensor,
                                   tensor_to_right: torch.Tensor,
                                   group=None) -> RingHandle:
    """``wait()`` returns ``[from_right, from_left]``."""
    return exchange_start(left_rank, right_rank, (tensor_to_right,),
                          (tensor_to_left,), group=group,
                          _result=lambda r, l: [r[0], l[0]])


class Hop(NamedTuple):
    """One exchange of the ring walk: the SOURCE ranks of the chunks sent and
    of those arriving; None for a direction the hop does not use."""
    send_right: Optional[int]
    send_left: Optional[int]
    from_right: Optional[int]
    from_left: Optional[int]
    wait_label: str
    loss_label: Optional[str]


def ring_schedule(world: int, rank: int, bidir: bool = False) -> list:
    """The hops in which ``rank`` sees every other rank's chunk exactly once.

    Unidirectional: ``W−1`` hops from the left, sources ``rank−k``.
    Bidirectional (``W > 2``): ``⌊(W−1)/2⌋`` rounds receiving ``rank+r`` from
    the right and ``rank−r`` from the left, plus one from-left remainder hop
    when ``W−1`` is odd.  Each hop forwards what the previous one delivered
    in the same travel direction (hop 1: the own chunk); the remainder hop
    forwards the rightward-travelling stream.
    """
    if not (bidir and world > 2):
        return [Hop((rank - k + 1) % world, None, None, (rank - k) % world,
                    f"ring_hop{k}_wait", f"ring_chunk{k}_loss")
                for k in range(1, world)]
    nb, rem = divmod(world - 1, 2)
    hops = [Hop((rank - r + 1) % world, (rank + r - 1) % world,
                (rank + r) % world, (rank - r) % world,
                f"ring_bhop{r}_wait", f"ring_bchunk{r}_loss")
            for r in range(1, nb + 1)]
    if rem:
        hops.append(Hop((rank - nb) % world, None, None,
                        (rank - nb - 1) % world, "ring_rem_wait", None))
    return hops


def walk_ring(own, world: int, rank: int, bidir: bool = False, group=None):
    """Generator driving :func:`ring_schedule` with ``own`` (a payload tuple)
    as this rank's chunk.  The first ``next()`` posts hop 1 and yields, so its
    wire time hides under the local block's kernel.  Every later step waits
    for a hop, posts the NEXT one — before the caller computes on this one —
    and yields ``(loss_label, [(src, payload), ...])``: the hop's chunks in
    right-then-left order and the span label for their kernels.
    """
    hops = ring_schedule(world, rank, bidir)
    left, right = (rank - 1) % world, (rank + 1) % world
    if group is not None and world > 1:
        # P2POp peers are GLOBAL ranks even when a group is given; rank, left
        # and right above are group-local.  Identity for the default group,
        # required for subgroups like {1, 2}.
        left = dist.get_global_rank(group, left)
        right = dist.get_global_rank(group, right)
    have = {rank: own}

    def post(hop):      # have.get(None) is None: nothing goes that way
        return exchange_start(left, right, have.get(hop.send_right),
                              have.get(hop.send_left), group=group)

    handle = post(hops[0]) if hops else None
    yield
    for k, hop in enumerate(hops):
        with hop_span(hop.wait_label):
            arrived = handle.wait()
        arrived = [(src, payload) for src, payload
                   in zip((hop.from_right, hop.from_left), arrived)
                   if src is not None]
        have.update(arrived)
        if k + 1 < len(hops):
            handle = post(hops[k + 1])
        yield hop.loss_label, arrived


class NeighbourExchange(torch.autograd.Function):
    """Differentiable one-hop exchange; backward performs the mirror-image
    exchange of ``grad_output`` (reference ``distributed_utils.py:65-77``)."""

    @staticmethod
    def forward(ctx, from_rank, to_rank, group, tensor):
        ctx.group = group
        ctx.from_rank = from_rank
        ctx.to_rank = to_rank
        return neighbour_exchange(from_rank, to_rank, tensor, group=group)

    @staticmethod
    def backward(ctx, grad_output):
        return (None, None, None) + (
            NeighbourExchange.apply(ctx.to_rank, ctx.from_rank, ctx.group,
                                    grad_output),
        )


def neighbour_exchange_with_grad(from_rank, to_rank, tensor, group=None):
    return NeighbourExchange.apply(from_rank, to_rank, group, tensor)


class NeighbourExchangeBidir(torch.autograd.Function):
    """Differentiable bidirectional exchange; backward swaps left/right
    (reference ``distributed_utils.py:84-98``)."""

    @staticmethod
    def forward(ctx, left_rank, right_rank, group, tensor_to_left,
                tensor_to_right):
        ctx.group = group
        ctx.left_rank = left_rank
        ctx.right_rank = right_rank
        return neighbour_exchange_bidir(left_rank, right_rank, tensor_to_left,
                                        tensor_to_right, group=group)

    @staticmethod
    def backward(ctx, *grad_outputs):
        return (None, None, None) + NeighbourExchangeBidir.apply(
            ctx.right_rank, ctx.left_rank, ctx.group, *grad_outputs)


def neighbour_exchange_bidir_with_grad(left_rank, right_rank, tensor_to_left,
                                       tensor_to_right, group=None):
    return NeighbourExchangeBidir.apply(left_rank, right_rank, group,
                                        tensor_to_left, tensor_to_right)
