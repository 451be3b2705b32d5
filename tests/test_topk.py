"""CPU tests for the top-k retrieval API (``losses/retrieval.py``): the torch
composite against brute force (tie rule and fill included), ``merge_topk``,
consistency with ``retrieval_ranks``, the gloo distributed form and the
example's ``--hard-negatives`` line."""

import math
import os
import subprocess
import sys

import pytest
import torch

from distributed_sigmoid_loss_amd import (
    TopK,
    distributed_retrieval_topk,
    merge_topk,
    pair_topk,
    retrieval_ranks,
    retrieval_topk,
)

from helpers import run_distributed

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute_topk(s, k, off):
    """Plain-Python selection under the total order (score descending, column
    ascending) → (scores (b, k), columns (b, k)) as lists."""
    b, n = s.shape
    scores, cols = [], []
    for i in range(b):
        cand = [(-float(s[i, j]), j) for j in range(n)
                if off is None or j != i + off]
        cand.sort()
        cand = cand[:k]
        scores.append([-v for v, _ in cand] + [-math.inf] * (k - len(cand)))
        cols.append([j for _, j in cand] + [-1] * (k - len(cand)))
    return scores, cols


def integer_pair(b, n, d, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    zi = torch.randint(-2, 3, (b, d), generator=g).to(dtype)
    zt = torch.randint(-2, 3, (n, d), generator=g).to(dtype)
    return zi, zt


@pytest.mark.parametrize("off", [None, 0, 3, -3, 40])
@pytest.mark.parametrize("k", [1, 4, 11, 20])
def test_torch_path_matches_brute_force(k, off):
    zi, zt = integer_pair(13, 11, 8, torch.float64, seed=1)
    s = zi @ zt.T
    got = pair_topk(zi, zt, k, off, impl="torch")
    assert isinstance(got, TopK)
    assert got.scores.dtype == torch.float64
    assert got.indices.dtype == torch.long
    ref_s, ref_c = brute_topk(s, k, off)
    assert got.indices.tolist() == ref_c
    assert got.scores.tolist() == ref_s
    # ties exist (few distinct integer scores), and the fill where k > n
    assert len(set(s[0].tolist())) < s.shape[1]
    if k > 11:
        assert bool((got.indices[:, -1] == -1).all())
        assert bool((got.scores[:, -1] == -math.inf).all())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_low_precision_inputs_compute_in_fp32(dtype):
    zi, zt = integer_pair(9, 14, 16, dtype, seed=2)
    got = pair_topk(zi, zt, 5, 0)               # auto: torch on CPU
    assert got.scores.dtype == torch.float32
    ref_s, ref_c = brute_topk(zi.double() @ zt.double().T, 5, 0)
    assert got.indices.tolist() == ref_c
    assert got.scores.tolist() == ref_s


def test_signed_zeros_tie():
    zi = torch.tensor([[1.0, 0.0]], dtype=torch.float64)
    zt = torch.tensor([[-0.0, 0.0], [0.0, 0.0], [-1.0, 0.0]],
                      dtype=torch.float64)
    got = pair_topk(zi, zt, 3, impl="torch")
    assert got.indices.tolist() == [[0, 1, 2]]


def test_col_base_and_bad_arguments():
    zi, zt = integer_pair(5, 3, 8, torch.float32, seed=3)
    plain = pair_topk(zi, zt, 4)
    moved = pair_topk(zi, zt, 4, col_base=100)
    assert bool((plain.indices[:, 3] == -1).all())
    assert torch.equal(moved.indices[:, :3], plain.indices[:, :3] + 100)
    assert bool((moved.indices[:, 3] == -1).all())
    with pytest.raises((RuntimeError, ValueError)):
        pair_topk(zi, zt, 0)
    with pytest.raises((RuntimeError, ValueError)):
        pair_topk(zi, zt[:, :4], 2)
    with pytest.raises(ValueError):
        pair_topk(zi, zt, 2, impl="triton")
    with pytest.raises(RuntimeError):
        pair_topk(zi, zt, 2, impl="hip")        # loud on CPU


def test_merge_topk_with_ties_and_fill():
    inf = math.inf
    a = TopK(torch.tensor([[5.0, 3.0, 3.0], [1.0, -inf, -inf]]),
             torch.tensor([[7, 2, 9], [4, -1, -1]]))
    b = TopK(torch.tensor([[5.0, 3.0, -inf], [-inf, -inf, -inf]]),
             torch.tensor([[1, 4, -1], [-1, -1, -1]]))
    got = merge_topk([a, b])
    assert got.indices.tolist() == [[1, 7, 2], [4, -1, -1]]
    assert got.scores.tolist() == [[5.0, 5.0, 3.0], [1.0, -inf, -inf]]
    got = merge_topk([b, a], k=7)
    assert got.indices.tolist() == [[1, 7, 2, 4, 9, -1, -1],
                                    [4, -1, -1, -1, -1, -1, -1]]
    assert got.scores[0].tolist() == [5.0, 5.0, 3.0, 3.0, 3.0, -inf, -inf]
    with pytest.raises(ValueError):
        merge_topk([])


@pytest.mark.parametrize("off", [None, 0, 5, -4])
def test_column_chunks_merge_to_the_single_call(off):
    zi, zt = integer_pair(12, 23, 8, torch.float32, seed=4)
    whole = pair_topk(zi, zt, 6, off)
    parts = [pair_topk(zi, zt[j0:j1], 6, None if off is None else off - j0,
                       col_base=j0)
             for j0, j1 in ((0, 4), (4, 5), (5, 17), (17, 23))]
    merged = merge_topk(parts)
    assert torch.equal(merged.indices, whole.indices)
    assert torch.equal(merged.scores, whole.scores)


@pytest.mark.parametrize("off", [0, 3, -2])
def test_consistent_with_retrieval_ranks(off):
    g = torch.Generator().manual_seed(5)
    zi = torch.randn(15, 8, generator=g, dtype=torch.float64)
    zt = torch.randn(19, 8, generator=g, dtype=torch.float64)
    s = zi @ zt.T
    assert s.unique().numel() == s.numel()      # distinct scores
    k = 4
    ranks = retrieval_ranks(zi, zt, off)
    i2t, t2i = retrieval_topk(zi, zt, k, None)
    rows = torch.arange(15)
    cols = torch.arange(19)
    assert torch.equal((ranks.i2t >= 0) & (ranks.i2t < k),
                       (i2t.indices == (rows + off)[:, None]).any(1))
    assert torch.equal((ranks.t2i >= 0) & (ranks.t2i < k),
                       (t2i.indices == (cols - off)[:, None]).any(1))
    # with the positive left out, the lists are the other direction's view
    neg_i2t, neg_t2i = retrieval_topk(zi, zt, k, off)
    assert not bool((neg_i2t.indices == (rows + off)[:, None]).any())
    assert not bool((neg_t2i.indices == (cols - off)[:, None]).any())
    ref_s, ref_c = brute_topk(s.T, k, -off)
    assert neg_t2i.indices.tolist() == ref_c


def _dist_topk(rank, world, b, d, k):
    zi, zt = integer_pair(world * b, world * b, d, torch.float32, seed=6)
    out = []
    for exclude in (False, True):
        i2t, t2i = distributed_retrieval_topk(
            zi[rank * b:(rank + 1) * b], zt[rank * b:(rank + 1) * b], k,
            exclude_positive=exclude)
        out.append((i2t.scores, i2t.indices, t2i.scores, t2i.indices))
    return out


@pytest.mark.parametrize("world", [2, 3])
def test_distributed_topk_equals_single_process_slices(world):
    b, d, k = 7, 16, 5
    zi, zt = integer_pair(world * b, world * b, d, torch.float32, seed=6)
    out = run_distributed(_dist_topk, world, b, d, k)
    assert sorted(out) == list(range(world))
    for e, exclude in enumerate((False, True)):
        ref_i2t, ref_t2i = retrieval_topk(zi, zt, k, 0 if exclude else None)
        for rank in range(world):
            sl = slice(rank * b, (rank + 1) * b)
            got = out[rank][e]
            assert torch.equal(got[0], ref_i2t.scores[sl])
            assert torch.equal(got[1], ref_i2t.indices[sl])
            assert torch.equal(got[2], ref_t2i.scores[sl])
            assert torch.equal(got[3], ref_t2i.indices[sl])


def test_world_one_is_retrieval_topk():
    zi, zt = integer_pair(9, 9, 8, torch.float32, seed=7)
    for exclude in (False, True):
        got = distributed_retrieval_topk(zi, zt, 3, exclude_positive=exclude)
        ref = retrieval_topk(zi, zt, 3, 0 if exclude else None)
        for g, r in zip(got, ref):
            assert torch.equal(g.scores, r.scores)
            assert torch.equal(g.indices, r.indices)


def test_example_hard_negatives_prints_margins():
    cmd = [sys.executable, os.path.join(REPO, "examples", "train_siglip.py"),
           "--device", "cpu", "--batch-per-gpu", "8", "--dim", "16",
           "--steps", "2", "--log-every", "1", "--eval-every", "1"]
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    on = subprocess.run(cmd + ["--hard-negatives", "3"], capture_output=True,
                        text=True, env=env, timeout=300)
    assert on.returncode == 0, on.stderr
    lines = [ln for ln in on.stdout.splitlines() if ln.startswith("hardneg")]
    assert len(lines) == 2
    for key in ("k=3", "i2t margin=", "t2i margin="):
        assert key in lines[0]
    assert len([ln for ln in on.stdout.splitlines()
                if ln.startswith("eval")]) == 2
