"""distributed_sigmoid_loss_amd — MI355X-native distributed SigLIP loss framework.

A from-scratch, MI355X-first (gfx950 / CDNA4) implementation of distributed
sigmoid contrastive loss (SigLIP, arXiv:2303.15343) with the same capabilities
as the reference repo ahmdtaha/distributed_sigmoid_loss:

- ``DistributedSigmoidLoss`` — all-gather strategy, module-owned learnable
  ``t_prime``/``bias`` (behavioral parity with reference
  ``distributed_sigmoid_loss.py:8-48``).
- ``SigLipLoss`` — ring strategy with caller-owned ``logit_scale``/``logit_bias``
  (behavioral parity with reference ``rwightman_sigmoid_loss.py:12-124``).
- ``parallel`` — autograd-correct ring neighbour-exchange primitives and
  differentiable collectives over torch.distributed (RCCL on ROCm, gloo on CPU)
  (behavioral parity with reference ``distributed_utils.py:1-106``).
- ``ops`` — hand-written CDNA4 HIP kernels (MFMA, LDS-tiled, gfx950) fusing
  pairwise logits + temperature/bias + log-sigmoid + reduction, forward and
  backward, never materializing the full N×N logits matrix.
- ``retrieval_ranks`` / ``recall_at_k`` / ``distributed_retrieval_ranks`` —
  the retrieval rank of every matching pair in both directions, counted by a
  fused HIP kernel over the same never-materialized grid.
- ``pair_topk`` / ``retrieval_topk`` / ``distributed_retrieval_topk`` /
  ``merge_topk`` — the ``k`` best scoring partners of every sample in both
  directions, with the positive left out on request (hard-negative mining),
  from a fused HIP kernel that keeps running per-row lists across column
  tiles; exact tie rule, bitwise reproducible, mergeable over column chunks.
- ``DistributedSoftmaxLoss`` / ``softmax_contrastive_loss`` — the softmax
  (CLIP / InfoNCE) baseline with the same contract: fused row and column
  log-sum-exp forward, fused dL/dlogit backward, single device or one grid
  across ranks.
- ``sigmoid_contrastive_loss_ids`` — the sigmoid loss with sample-ID labels:
  int64 ids decide what is a positive, a negative or an ignored pair (several
  captions per image, repeated samples, padding rows), from a fused HIP kernel
  with a saved-g and a band-recompute backward; ``DistributedSigmoidLoss``
  takes ``image_ids`` / ``text_ids``.
- ``softmax_contrastive_loss_ids`` — the softmax loss with the same sample-ID
  labels (multi-positive InfoNCE: the mean over a row's or column's positives
  of ``−log softmax``, masked pairs out of both normalisers), from a fused
  HIP kernel pair that adds positive sums and counts to the log-sum-exp pass;
  ``DistributedSoftmaxLoss`` takes ``image_ids`` / ``text_ids``.

The compute path is PyTorch-ROCm + HIP/CDNA4 kernels + RCCL over xGMI; there
are no CUDA compatibility layers and no multi-backend dispatch.
"""

__version__ = "0.2.0"

from .losses.sigmoid_loss import DistributedSigmoidLoss, SigLipLoss
from .losses.functional import sigmoid_contrastive_loss
from .losses.retrieval import (
    RetrievalRanks,
    pair_rank_counts,
    positive_scores,
    retrieval_ranks,
    recall_at_k,
    distributed_retrieval_ranks,
    TopK,
    pair_topk,
    merge_topk,
    retrieval_topk,
    distributed_retrieval_topk,
)
from .losses.softmax_loss import (
    DistributedSoftmaxLoss,
    softmax_contrastive_loss,
    softmax_contrastive_loss_ids,
)
from .losses.id_labels import sigmoid_contrastive_loss_ids
from .parallel.ring import (
    neighbour_exchange,
    neighbour_exchange_bidir,
    neighbour_exchange_with_grad,
    neighbour_exchange_bidir_with_grad,
)
from .parallel.collectives import all_gather_with_grad

__all__ = [
    "DistributedSigmoidLoss",
    "SigLipLoss",
    "sigmoid_contrastive_loss",
    "RetrievalRanks",
    "pair_rank_counts",
    "positive_scores",
    "retrieval_ranks",
    "recall_at_k",
    "distributed_retrieval_ranks",
    "TopK",
    "pair_topk",
    "merge_topk",
    "retrieval_topk",
    "distributed_retrieval_topk",
    "DistributedSoftmaxLoss",
    "softmax_contrastive_loss",
    "softmax_contrastive_loss_ids",
    "sigmoid_contrastive_loss_ids",
    "neighbour_exchange",
    "neighbour_exchange_bidir",
    "neighbour_exchange_with_grad",
    "neighbour_exchange_bidir_with_grad",
    "all_gather_with_grad",
]
