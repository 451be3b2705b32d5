"""CPU tests for the retrieval ranks with sample-ID labels: the torch path
against the dense form, the gloo composition and the example's report."""

import importlib.util
import math
import os
import subprocess
import sys

import pytest
import torch

from distributed_sigmoid_loss_amd import (
    distributed_retrieval_ranks_ids, pair_best_positive_ids,
    pair_rank_counts_ids, recall_at_k, retrieval_ranks, retrieval_ranks_ids)
from distributed_sigmoid_loss_amd.losses.id_labels import pair_classes

from helpers import run_distributed

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [("positive", None), ("ignore", 0), ("ignore", 3), ("ignore", -4),
         ("ignore", 40)]


def case(b, n, d, dtype=torch.float64, seed=0):
    """Integer embeddings; ids with several positives per row and column,
    masked entries and ids missing on either side."""
    g = torch.Generator().manual_seed(seed)
    zi = torch.randint(-3, 4, (b, d), generator=g).to(dtype)
    zt = torch.randint(-3, 4, (n, d), generator=g).to(dtype)
    img_ids = torch.randint(0, 8, (b,), generator=g)
    txt_ids = torch.randint(2, 10, (n,), generator=g)
    img_ids[1], txt_ids[2] = -1, -3
    return zi, zt, img_ids, txt_ids


def dense_ranks(zi, zt, img_ids, txt_ids, mode, off):
    s = zi.double() @ zt.double().T
    pos, masked = pair_classes(img_ids, txt_ids, mode, off)
    pos, neg = pos & ~masked, ~pos & ~masked
    sp = s.masked_fill(~pos, -math.inf)
    rb, cb = sp.amax(1), sp.amax(0)
    i2t = ((s > rb[:, None]) & neg).sum(1)
    t2i = ((s > cb[None, :]) & neg).sum(0)
    i2t[rb == -math.inf], t2i[cb == -math.inf] = -1, -1
    return rb, cb, i2t, t2i


@pytest.mark.parametrize("mode,off", MODES)
def test_torch_path_matches_the_dense_form_in_fp64(mode, off):
    zi, zt, ii, ti = case(21, 17, 16)
    rb, cb, i2t, t2i = dense_ranks(zi, zt, ii, ti, mode, off)
    k_rb, k_cb = pair_best_positive_ids(zi, zt, ii, ti, mode, off)
    assert k_rb.dtype == torch.float64
    assert torch.equal(k_rb, rb) and torch.equal(k_cb, cb)
    got = retrieval_ranks_ids(zi, zt, ii, ti, mode, off)
    assert got.i2t.dtype == torch.long
    assert torch.equal(got.i2t, i2t) and torch.equal(got.t2i, t2i)
    assert bool((got.i2t == -1).any())
    assert off == 40 or bool((got.i2t >= 0).any())
    with pytest.raises(RuntimeError):
        retrieval_ranks_ids(zi.bfloat16(), zt.bfloat16(), ii, ti, impl="hip")


@pytest.mark.parametrize("mode,off", [("positive", None), ("ignore", 3)])
def test_chunk_invariance_and_accumulation(mode, off):
    zi, zt, ii, ti = case(37, 29, 8, torch.float32, seed=1)
    rb, cb = pair_best_positive_ids(zi, zt, ii, ti, mode, off)
    rc, cc = pair_rank_counts_ids(zi, zt, rb, cb, ii, ti, mode, off)
    for chunk in (1, 5, 36):
        got = pair_best_positive_ids(zi, zt, ii, ti, mode, off,
                                     row_chunk=chunk)
        assert torch.equal(got[0], rb) and torch.equal(got[1], cb)
        got = pair_rank_counts_ids(zi, zt, rb, cb, ii, ti, mode, off,
                                   row_chunk=chunk)
        assert torch.equal(got[0], rc) and torch.equal(got[1], cc)
    a_rb, a_cb = torch.full((37,), -math.inf), torch.full((29,), -math.inf)
    a_rc = torch.zeros(37, dtype=torch.int32)
    a_cc = torch.zeros(29, dtype=torch.int32)
    for j0 in (0, 10, 20):
        j1, off_j = min(29, j0 + 10), None if off is None else off - j0
        pair_best_positive_ids(zi, zt[j0:j1], ii, ti[j0:j1], mode, off_j,
                               row_best=a_rb, col_best=a_cb[j0:j1])
        pair_rank_counts_ids(zi, zt[j0:j1], rb, cb[j0:j1], ii, ti[j0:j1],
                             mode, off_j, row_cnt=a_rc, col_cnt=a_cc[j0:j1])
    assert torch.equal(a_rb, rb) and torch.equal(a_cb, cb)
    assert torch.equal(a_rc, rc) and torch.equal(a_cc, cc)
    none, o_cb = pair_best_positive_ids(zi, zt, ii, ti, mode, off, rows=False)
    assert none is None and torch.equal(o_cb, cb)


@pytest.mark.parametrize("off", [0, 5, -5, 40])
def test_distinct_ids_give_the_positional_ranks(off):
    zi, zt, _, _ = case(21, 17, 16, torch.float32, seed=2)
    want = retrieval_ranks(zi, zt, off)
    ar_b, ar_n = torch.arange(21), torch.arange(17)
    got = [retrieval_ranks_ids(zi, zt, ar_b, ar_n + 21, "ignore", off)]
    if off >= 0:
        got.append(retrieval_ranks_ids(zi, zt, ar_b + off, ar_n))
    for g in got:
        assert torch.equal(g.i2t, want.i2t) and torch.equal(g.t2i, want.t2i)


def test_all_masked_block_and_best_caption():
    zi, zt, ii, ti = case(9, 11, 8, torch.float32)
    got = retrieval_ranks_ids(zi, zt, torch.full((9,), -1), ti)
    assert bool((got.i2t == -1).all()) and bool((got.t2i == -1).all())
    assert math.isnan(recall_at_k(got.i2t)["R@1"])
    # Two captions per image, the second one the better: by position every
    # other image misses at k = 1, by id none does.
    x = torch.eye(6).repeat_interleave(2, 0)
    t = x * torch.tensor([0.5, 1.0]).repeat(6)[:, None]
    ids = torch.arange(12) // 2
    assert recall_at_k(retrieval_ranks(x, t, 0).i2t)["R@1"] == 0.5
    by_id = distributed_retrieval_ranks_ids(x, t, ids, ids)   # world size 1
    assert recall_at_k(by_id.i2t)["R@1"] == 1.0
    assert recall_at_k(by_id.t2i)["R@1"] == 1.0


def _dist_ranks(rank, world, b, d, mode):
    zi, zt, ii, ti = case(world * b, world * b, d, torch.float32, seed=3)
    sl = slice(rank * b, (rank + 1) * b)
    got = distributed_retrieval_ranks_ids(zi[sl], zt[sl], ii[sl], ti[sl], mode)
    return got.i2t, got.t2i


@pytest.mark.parametrize("mode", ["positive", "ignore"])
@pytest.mark.parametrize("world", [2, 3])
def test_distributed_ranks_equal_single_process_slices(world, mode):
    b, d = 7, 16
    zi, zt, ii, ti = case(world * b, world * b, d, torch.float32, seed=3)
    # a column's positives sit on several ranks
    pos = pair_classes(ii, ti, "positive")[0]
    assert bool((pos[:b].any(0) & pos[b:2 * b].any(0)).any())
    ref = retrieval_ranks_ids(zi, zt, ii, ti, mode, 0)
    out = run_distributed(_dist_ranks, world, b, d, mode)
    for rank in range(world):
        i2t, t2i = out[rank]
        assert torch.equal(i2t, ref.i2t[rank * b:(rank + 1) * b])
        assert torch.equal(t2i, ref.t2i[rank * b:(rank + 1) * b])


def test_example_reports_ranks_by_id():
    cmd = [sys.executable, os.path.join(REPO, "examples", "train_siglip.py"),
           "--device", "cpu", "--batch-per-gpu", "16", "--dim", "32",
           "--steps", "2", "--log-every", "1", "--strategy", "all_gather",
           "--captions-per-image", "2", "--eval-every", "1"]
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    out = subprocess.run(cmd, capture_output=True, text=True, env=env,
                         timeout=300)
    assert out.returncode == 0, out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("eval")]
    assert len(lines) == 2
    # The first report recomputed (towers at their seeded init, the batch of
    # step 0): it is the by-id figure, and the positional one differs.
    spec = importlib.util.spec_from_file_location("train_siglip_ex", cmd[1])
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    example.set_seed(1234)
    model = example.TwoTowerModel(32, 32)
    img, txt = example.synthetic_batch(16, 32, "cpu", torch.float32, 0)
    with torch.no_grad():
        zi, zt = model(img[:8].repeat_interleave(2, 0), txt)
    ids = torch.arange(16) // 2
    by_id = recall_at_k(retrieval_ranks_ids(zi, zt, ids, ids).i2t, (1, 5))
    by_pos = recall_at_k(retrieval_ranks(zi, zt, 0).i2t, (1, 5))
    assert by_id != by_pos
    assert (f"i2t R@1={by_id['R@1']:.4f} R@5={by_id['R@5']:.4f}"
            in lines[0])
