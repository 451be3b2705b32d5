from .sigmoid_loss import DistributedSigmoidLoss, SigLipLoss
from .functional import sigmoid_contrastive_loss
from .retrieval import (
    RetrievalRanks,
    pair_rank_counts,
    positive_scores,
    retrieval_ranks,
    recall_at_k,
    distributed_retrieval_ranks,
)
from .softmax_loss import DistributedSoftmaxLoss, softmax_contrastive_loss
from .id_labels import sigmoid_contrastive_loss_ids

__all__ = ["DistributedSigmoidLoss", "SigLipLoss", "sigmoid_contrastive_loss",
           "RetrievalRanks", "pair_rank_counts", "positive_scores",
           "retrieval_ranks", "recall_at_k", "distributed_retrieval_ranks",
           "DistributedSoftmaxLoss", "softmax_contrastive_loss",
           "sigmoid_contrastive_loss_ids"]
