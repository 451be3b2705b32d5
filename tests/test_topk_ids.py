"""Top-k under sample-ID labels on the CPU: the torch path of
``pair_topk_ids`` against a dense brute force, chunk merging, consistency with
the id ranks, the gloo composition and the example's hard-negative report."""

import importlib.util
import math
import os
import subprocess
import sys

import pytest
import torch

from distributed_sigmoid_loss_amd import (
    distributed_retrieval_topk_ids, merge_topk, pair_topk_ids,
    positive_scores, retrieval_ranks_ids, retrieval_topk, retrieval_topk_ids)
from distributed_sigmoid_loss_amd.losses.id_labels import pair_classes

from helpers import run_distributed

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = -math.inf
MODES = [("positive", None), ("ignore", 0), ("ignore", 9), ("ignore", -4)]


def case(b, n, d, seed=0):
    """Integer-valued float64 embeddings (ties, exact scores), 3 images and 5
    shuffled texts per id, a masked row and column."""
    g = torch.Generator().manual_seed(seed)
    zi = torch.randint(-3, 4, (b, d), generator=g).double()
    zt = torch.randint(-3, 4, (n, d), generator=g).double()
    ii = torch.arange(b) // 3
    ti = (torch.arange(n) // 5)[torch.randperm(n, generator=g)]
    ii[1], ti[2] = -1, -1
    return zi, zt, ii, ti


def brute(zi, zt, ii, ti, mode, off, k):
    pos, masked = pair_classes(ii, ti, mode, off)
    s, scores, cols = zi @ zt.T, [], []
    for i in range(zi.shape[0]):
        cand = sorted((-float(s[i, j]), j) for j in range(zt.shape[0])
                      if not pos[i, j] and not masked[i, j])[:k]
        scores.append([-c[0] for c in cand] + [NINF] * (k - len(cand)))
        cols.append([c[1] for c in cand] + [-1] * (k - len(cand)))
    return torch.tensor(scores, dtype=torch.float64), torch.tensor(cols)


@pytest.mark.parametrize("mode,off", MODES)
@pytest.mark.parametrize("k", [1, 5, 40])
def test_torch_path_matches_brute_force_and_merges(mode, off, k):
    zi, zt, ii, ti = case(23, 37, 8)
    ws, wc = brute(zi, zt, ii, ti, mode, off, k)
    got = pair_topk_ids(zi, zt, k, ii, ti, mode, off)
    assert torch.equal(got.scores, ws) and torch.equal(got.indices, wc)
    assert bool((wc[1] == -1).all()) and bool((wc != 2).all())
    parts = [pair_topk_ids(zi, zt[j0:j0 + 10], k, ii, ti[j0:j0 + 10], mode,
                           None if off is None else off - j0, col_base=j0)
             for j0 in range(0, 37, 10)]
    merged = merge_topk(parts)
    assert torch.equal(merged.scores, ws) and torch.equal(merged.indices, wc)


def test_consistent_with_the_id_ranks():
    zi, zt, ii, ti = case(23, 37, 8, seed=1)
    k = 6
    ranks = retrieval_ranks_ids(zi, zt, ii, ti).i2t
    pos, masked = pair_classes(ii, ti)
    best = (zi @ zt.T).masked_fill(~pos | masked, NINF).amax(1)
    above = (pair_topk_ids(zi, zt, k, ii, ti).scores > best[:, None]).sum(1)
    low = (ranks >= 0) & (ranks < k)
    assert bool(low.any()) and torch.equal(above[low], ranks[low])


def _dist_topk(rank, world, b, d, mode):
    zi, zt, ii, ti = case(world * b, world * b, d, seed=3)
    sl = slice(rank * b, (rank + 1) * b)
    i2t, t2i = distributed_retrieval_topk_ids(zi[sl], zt[sl], 4, ii[sl],
                                              ti[sl], mode)
    return (*i2t, *t2i)


@pytest.mark.parametrize("mode", ["positive", "ignore"])
@pytest.mark.parametrize("world", [2, 3])
def test_distributed_lists_equal_single_process_slices(world, mode):
    b, d = 7, 16
    zi, zt, ii, ti = case(world * b, world * b, d, seed=3)
    ref = retrieval_topk_ids(zi, zt, 4, ii, ti, mode, 0)
    ref = (*ref[0], *ref[1])
    out = run_distributed(_dist_topk, world, b, d, mode)
    for rank in range(world):
        for got, want in zip(out[rank], ref):
            assert torch.equal(got, want[rank * b:(rank + 1) * b])


def test_example_mines_hard_negatives_by_id():
    cmd = [sys.executable, os.path.join(REPO, "examples", "train_siglip.py"),
           "--device", "cpu", "--batch-per-gpu", "16", "--dim", "32",
           "--steps", "2", "--log-every", "1", "--strategy", "all_gather",
           "--captions-per-image", "2", "--eval-every", "1",
           "--hard-negatives", "3"]
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    out = subprocess.run(cmd, capture_output=True, text=True, env=env,
                         timeout=300)
    assert out.returncode == 0, out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("hardneg")]
    assert len(lines) == 2
    # The first report recomputed: by id, and the positional one differs.
    spec = importlib.util.spec_from_file_location("train_siglip_ex", cmd[1])
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    example.set_seed(1234)
    model = example.TwoTowerModel(32, 32)
    img, txt = example.synthetic_batch(16, 32, "cpu", torch.float32, 0)
    with torch.no_grad():
        zi, zt = model(img[:8].repeat_interleave(2, 0), txt)
    ids = torch.arange(16) // 2
    pos = positive_scores(zi, zt, 0)

    def report(lists):
        m = [float((pos - neg.scores.mean(1)).mean()) for neg in lists]
        return f"i2t margin={m[0]:.4f}  t2i margin={m[1]:.4f}"

    by_id = report(retrieval_topk_ids(zi, zt, 3, ids, ids))
    assert by_id != report(retrieval_topk(zi, zt, 3, 0))
    assert by_id in lines[0]
