"""CPU tests for the retrieval metrics (``losses/retrieval.py``): the torch
implementation of the rank counts against brute force, the rank / recall
helpers, the distributed composition on gloo, and the example's
``--eval-every`` report."""

import math
import os
import subprocess
import sys

import pytest
import torch

from distributed_sigmoid_loss_amd import (
    RetrievalRanks,
    distributed_retrieval_ranks,
    pair_rank_counts,
    positive_scores,
    recall_at_k,
    retrieval_ranks,
)
from distributed_sigmoid_loss_amd.losses import retrieval

from helpers import run_distributed

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute_counts(s, row_thr, col_thr, off):
    """Python-loop reference on an explicit score matrix."""
    b, n = s.shape
    rc = torch.zeros(b, dtype=torch.int32)
    cc = torch.zeros(n, dtype=torch.int32)
    for i in range(b):
        for j in range(n):
            if off is not None and j == i + off:
                continue
            rc[i] += int(s[i, j] > row_thr[i])
            cc[j] += int(s[i, j] > col_thr[j])
    return rc, cc


def brute_ranks(s, off):
    b, n = s.shape
    i2t = torch.full((b,), -1, dtype=torch.long)
    t2i = torch.full((n,), -1, dtype=torch.long)
    if off is None:
        return i2t, t2i
    for i in range(b):
        j = i + off
        if 0 <= j < n:
            i2t[i] = sum(int(s[i, jj] > s[i, j]) for jj in range(n) if jj != j)
            t2i[j] = sum(int(s[ii, j] > s[i, j]) for ii in range(b) if ii != i)
    return i2t, t2i


def integer_pair(b, n, d, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    zi = torch.randint(-3, 4, (b, d), generator=g).to(dtype)
    zt = torch.randint(-3, 4, (n, d), generator=g).to(dtype)
    return zi, zt


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64,
                                   torch.bfloat16])
@pytest.mark.parametrize("off", [None, 0, 3, -4, 30])
def test_torch_counts_match_brute_force(dtype, off):
    b, n, d = 19, 23, 16
    zi, zt = integer_pair(b, n, d, dtype)
    s = zi.double() @ zt.double().T
    # thresholds from the row's / column's own scores: ties, strict >
    row_thr = s[torch.arange(b), torch.arange(b) % n].float()
    col_thr = s[torch.arange(n) % b, torch.arange(n)].float()
    rc, cc = pair_rank_counts(zi, zt, row_thr, col_thr, off, impl="torch")
    ref_rc, ref_cc = brute_counts(s, row_thr.double(), col_thr.double(), off)
    assert rc.dtype == torch.int32 and cc.dtype == torch.int32
    assert torch.equal(rc, ref_rc) and torch.equal(cc, ref_cc)


def test_fp64_inputs_compute_in_fp64():
    # Two scores 1 + 2^-40 apart around the threshold: fp32 compute would
    # merge them, fp64 must not.
    zi = torch.tensor([[1.0, 2.0 ** -40]], dtype=torch.float64)
    zt = torch.tensor([[1.0, 0.0], [1.0, 1.0], [1.0, 2.0]],
                      dtype=torch.float64)
    thr = torch.tensor([1.0 + 2.0 ** -40], dtype=torch.float64)
    rc, _ = pair_rank_counts(zi, zt, row_thr=thr, impl="torch")
    assert rc.tolist() == [1]
    assert positive_scores(zi, zt, 1).dtype == torch.float64
    assert positive_scores(zi.float(), zt.float(), 1).dtype == torch.float32


def test_chunk_size_invariance_and_accumulation():
    zi, zt = integer_pair(37, 29, 8, torch.float32, seed=1)
    row_thr = torch.zeros(37)
    col_thr = torch.ones(29)
    ref = retrieval._torch_pair_rank_counts(zi, zt, row_thr, col_thr, 2,
                                            None, None, row_chunk=1000)
    for chunk in (1, 5, 36, 37):
        got = retrieval._torch_pair_rank_counts(zi, zt, row_thr, col_thr, 2,
                                                None, None, row_chunk=chunk)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    # add-into-counts contract: a second call doubles, column chunks compose
    rc, cc = pair_rank_counts(zi, zt, row_thr, col_thr, 2,
                              row_cnt=ref[0].clone(), col_cnt=ref[1].clone())
    assert torch.equal(rc, 2 * ref[0]) and torch.equal(cc, 2 * ref[1])
    rc = torch.zeros(37, dtype=torch.int32)
    parts = []
    for j0 in (0, 10, 20):
        j1 = min(29, j0 + 10)
        _, part = pair_rank_counts(zi, zt[j0:j1], row_thr, col_thr[j0:j1],
                                   2 - j0, row_cnt=rc)
        parts.append(part)
    assert torch.equal(rc, ref[0]) and torch.equal(torch.cat(parts), ref[1])
    # one side only
    r_only, none = pair_rank_counts(zi, zt, row_thr=row_thr, diag_offset=2)
    assert none is None and torch.equal(r_only, ref[0])
    with pytest.raises(RuntimeError):
        pair_rank_counts(zi, zt, row_thr[:-1], col_thr)
    with pytest.raises(ValueError):
        pair_rank_counts(zi, zt, row_thr, col_thr, impl="nope")


def test_hip_impl_is_loud_on_cpu():
    zi, zt = integer_pair(8, 8, 8, torch.bfloat16)
    with pytest.raises(RuntimeError):
        pair_rank_counts(zi, zt, torch.zeros(8), torch.zeros(8), impl="hip")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("off", [None, 0, 5, -5, 40])
def test_retrieval_ranks_and_missing_positives(dtype, off):
    b, n, d = 21, 17, 16
    zi, zt = integer_pair(b, n, d, dtype, seed=2)
    got = retrieval_ranks(zi, zt, off)
    assert isinstance(got, RetrievalRanks)
    ref_i2t, ref_t2i = brute_ranks(zi.double() @ zt.double().T, off)
    assert got.i2t.dtype == torch.long and got.t2i.dtype == torch.long
    assert torch.equal(got.i2t, ref_i2t) and torch.equal(got.t2i, ref_t2i)
    pos = positive_scores(zi, zt, off)
    assert pos.shape == (b,)
    assert torch.equal(torch.isinf(pos), ref_i2t < 0)


def test_perfect_and_shifted_towers():
    z = torch.diag(1.0 + (torch.arange(12) % 5).float())
    r = retrieval_ranks(z, z, 0)
    assert not r.i2t.any() and not r.t2i.any()
    r = retrieval_ranks(z, z.roll(1, 0), 0)
    assert bool((r.i2t == 1).all()) and bool((r.t2i == 1).all())


def test_recall_at_k_on_hand_made_ranks():
    ranks = torch.tensor([0, 0, 3, 4, 5, 9, 10, 120, -1, -1])
    got = recall_at_k(ranks)
    assert got == {"R@1": 2 / 8, "R@5": 4 / 8, "R@10": 6 / 8}
    assert recall_at_k(ranks, ks=(11,)) == {"R@11": 7 / 8}
    assert math.isnan(recall_at_k(torch.tensor([-1, -1]))["R@1"])


def _dist_ranks(rank, world, b, d):
    zi, zt = integer_pair(world * b, world * b, d, torch.float32, seed=3)
    got = distributed_retrieval_ranks(zi[rank * b:(rank + 1) * b],
                                      zt[rank * b:(rank + 1) * b])
    return got.i2t, got.t2i


@pytest.mark.parametrize("world", [2, 3])
def test_distributed_ranks_equal_single_process_slices(world):
    b, d = 7, 16
    zi, zt = integer_pair(world * b, world * b, d, torch.float32, seed=3)
    ref = retrieval_ranks(zi, zt, 0)
    out = run_distributed(_dist_ranks, world, b, d)
    assert sorted(out) == list(range(world))
    for rank in range(world):
        i2t, t2i = out[rank]
        assert torch.equal(i2t, ref.i2t[rank * b:(rank + 1) * b])
        assert torch.equal(t2i, ref.t2i[rank * b:(rank + 1) * b])


def test_world_one_is_retrieval_ranks():
    zi, zt = integer_pair(9, 9, 8, torch.float32, seed=4)
    got = distributed_retrieval_ranks(zi, zt)
    ref = retrieval_ranks(zi, zt, 0)
    assert torch.equal(got.i2t, ref.i2t) and torch.equal(got.t2i, ref.t2i)


def test_example_eval_every_prints_metrics():
    cmd = [sys.executable, os.path.join(REPO, "examples", "train_siglip.py"),
           "--device", "cpu", "--batch-per-gpu", "8", "--dim", "16",
           "--steps", "2", "--log-every", "1"]
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    off = subprocess.run(cmd, capture_output=True, text=True, env=env,
                         timeout=300)
    assert off.returncode == 0, off.stderr
    assert "eval" not in off.stdout
    on = subprocess.run(cmd + ["--eval-every", "1"], capture_output=True,
                        text=True, env=env, timeout=300)
    assert on.returncode == 0, on.stderr
    lines = [ln for ln in on.stdout.splitlines() if ln.startswith("eval")]
    assert len(lines) == 2
    for key in ("i2t R@1=", "R@5=", "median=", "t2i R@1="):
        assert key in lines[0]
