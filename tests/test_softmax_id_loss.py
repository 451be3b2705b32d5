"""Softmax contrastive loss with sample-ID labels on the CPU: the torch path
of ``softmax_contrastive_loss_ids`` in float64 against a dense textbook form
written here (masked ``logsumexp`` both ways, mean over the positives), its
column chunking, the ``arange`` equivalence with ``softmax_contrastive_loss``,
the one-grid distributed form over gloo and the module's id arguments."""

from __future__ import annotations

import math

import pytest
import torch
import torch.distributed as dist
import torch.nn.functional as F

import distributed_sigmoid_loss_amd as pkg
from distributed_sigmoid_loss_amd import (
    DistributedSoftmaxLoss,
    softmax_contrastive_loss,
    softmax_contrastive_loss_ids,
)

from helpers import run_distributed


def _classes(iid, tid, dup, off):
    """``(positive, masked)`` of the contract, written out densely."""
    b, n = iid.shape[0], tid.shape[0]
    eq = iid[:, None] == tid[None, :]
    masked = (iid < 0)[:, None] | (tid < 0)[None, :]
    if dup == "positive":
        pos = eq
    else:
        pos = torch.zeros(b, n, dtype=torch.bool)
        if off is not None:
            pos = (torch.arange(n)[None, :]
                   == torch.arange(b)[:, None] + off)
        masked = masked | (eq & ~pos)
    return pos & ~masked, masked


def _terms(z, pos, masked):
    """Per-row terms ``lse_i − mean_{p∈P_i} z_ip`` (0 without a positive)."""
    cnt = pos.sum(1)
    has = cnt > 0
    out = torch.zeros(z.shape[0], dtype=z.dtype)
    if bool(has.any()):
        zm = z[has].masked_fill(masked[has], -math.inf)
        mean = torch.where(pos[has], z[has],
                           torch.zeros_like(z[has])).sum(1) / cnt[has]
        out = out.index_put((has.nonzero().squeeze(1),),
                            torch.logsumexp(zm, 1) - mean)
    return out


def _textbook(zi, zt, tp, iid, tid, dup, off, rows=None, cols=None):
    z = tp.exp() * zi @ zt.T
    pos, masked = _classes(iid, tid, dup, off)
    r, c = _terms(z, pos, masked), _terms(z.T, pos.T, masked.T)
    return (r if rows is None else r[rows]).sum() + (
        c if cols is None else c[cols]).sum()


def _inputs(b, n, d, dtype=torch.float64, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + b * 131 + n * 17 + d)
    zi = F.normalize(torch.randn(b, d, generator=g, dtype=dtype), dim=-1)
    zt = F.normalize(torch.randn(n, d, generator=g, dtype=dtype), dim=-1)
    return (zi.requires_grad_(), zt.requires_grad_(),
            torch.tensor(math.log(5.0), dtype=dtype).requires_grad_())


def _ids(b, n, seed=0):
    """A few values, so rows and columns have several positives; one masked
    row and column; one row whose id nobody shares."""
    g = torch.Generator().manual_seed(100 + seed + b + 3 * n)
    k = max(2, max(b, n) // 3)
    iid = torch.randint(0, k, (b,), generator=g)
    tid = torch.randint(0, k, (n,), generator=g)
    iid[1], tid[2] = -1, -7
    iid[0] = 10 ** 12
    return iid, tid


def _grads(loss, params):
    return torch.autograd.grad(loss, params, allow_unused=True)


SHAPES = [(7, 7, 8), (5, 9, 8)]


def test_exported():
    assert "softmax_contrastive_loss_ids" in pkg.__all__
    assert pkg.softmax_contrastive_loss_ids is softmax_contrastive_loss_ids
    assert "softmax_contrastive_loss_ids" in pkg.__doc__


@pytest.mark.parametrize("b,n,d", SHAPES)
@pytest.mark.parametrize("dup,off", [("positive", None), ("ignore", 0),
                                     ("ignore", 2), ("ignore", -2),
                                     ("ignore", None)])
def test_fp64_matches_textbook(b, n, d, dup, off):
    params = _inputs(b, n, d)
    iid, tid = _ids(b, n)
    pos, masked = _classes(iid, tid, dup, off)
    if dup == "positive":
        assert int(pos.sum(1).max()) >= 2 and int(pos.sum(0).max()) >= 2
        assert bool(((pos.sum(1) == 0) & (iid >= 0)).any())
    got = softmax_contrastive_loss_ids(*params, iid, tid, duplicates=dup,
                                       diag_offset=off, impl="torch")
    ref = _textbook(*params, iid, tid, dup, off)
    assert got.dtype == torch.float64 and got.dim() == 0
    torch.testing.assert_close(got, ref, rtol=1e-9, atol=1e-12)
    if off is None and dup == "ignore":      # no positive anywhere
        assert float(got.detach()) == 0.0
        assert all(float(g.abs().max()) == 0.0 for g in _grads(got, params))
        return
    for g, r in zip(_grads(got, params), _grads(ref, params)):
        assert bool(torch.isfinite(g).all())
        torch.testing.assert_close(g, r, rtol=1e-9, atol=1e-12)
    # masked rows and columns take no gradient at all
    gi, gt, _ = _grads(softmax_contrastive_loss_ids(
        *params, iid, tid, duplicates=dup, diag_offset=off), params)
    assert float(gi[1].abs().max()) == 0.0
    assert float(gt[2].abs().max()) == 0.0


@pytest.mark.parametrize("b,n,d", SHAPES)
@pytest.mark.parametrize("dup", ["positive", "ignore"])
@pytest.mark.parametrize("chunk", [1, 3, "n"])
def test_col_chunk_equals_unchunked(b, n, d, dup, chunk):
    chunk = n if chunk == "n" else chunk
    params = _inputs(b, n, d, seed=1)
    iid, tid = _ids(b, n, seed=1)
    kw = dict(duplicates=dup, diag_offset=1)
    ref = softmax_contrastive_loss_ids(*params, iid, tid, **kw)
    got = softmax_contrastive_loss_ids(*params, iid, tid, col_chunk=chunk,
                                       **kw)
    torch.testing.assert_close(got, ref, rtol=1e-10, atol=0)
    for g, r in zip(_grads(got, params), _grads(ref, params)):
        torch.testing.assert_close(g, r, rtol=1e-10, atol=1e-14)


@pytest.mark.parametrize("b,n,d", SHAPES)
@pytest.mark.parametrize("diag", [0, 2, -2])
def test_arange_ids_are_the_positional_loss(b, n, d, diag):
    params = _inputs(b, n, d, seed=2)
    # ids stay non-negative (a negative id is a mask): shift the other side
    # for a negative offset
    got = softmax_contrastive_loss_ids(
        *params, torch.arange(b) + max(diag, 0),
        torch.arange(n) + max(-diag, 0))
    ref = softmax_contrastive_loss(*params, diag_offset=diag)
    torch.testing.assert_close(got, ref, rtol=1e-12, atol=1e-12)
    for g, r in zip(_grads(got, params), _grads(ref, params)):
        torch.testing.assert_close(g, r, rtol=1e-10, atol=1e-13)


def test_ignore_and_positive_differ():
    """A repeated caption: "positive" pulls it in, "ignore" only takes it out
    of the normalisers — both differ from each other and from treating it as
    a negative."""
    params = _inputs(6, 6, 8, seed=3)
    iid = torch.tensor([0, 1, 2, 3, 4, 5])
    tid = torch.tensor([0, 1, 2, 0, 4, 5])     # text 3 repeats sample 0
    pos = softmax_contrastive_loss_ids(*params, iid, tid)
    ign = softmax_contrastive_loss_ids(*params, iid, tid,
                                       duplicates="ignore", diag_offset=0)
    plain = softmax_contrastive_loss(*params, diag_offset=0)
    for dup, got in (("positive", pos), ("ignore", ign)):
        torch.testing.assert_close(
            got, _textbook(*params, iid, tid, dup, 0), rtol=1e-9, atol=1e-12)
    vals = [float(v.detach()) for v in (pos, ign, plain)]
    assert len({round(v, 9) for v in vals}) == 3, vals
    # "ignore" drops one term from row 0's and column 3's normaliser and
    # nothing else: it can only lower those terms.
    assert vals[1] < vals[2]


def test_all_masked_block():
    params = _inputs(5, 9, 8, seed=4)
    iid, tid = torch.full((5,), -1), torch.arange(9)
    for dup in ("positive", "ignore"):
        got = softmax_contrastive_loss_ids(*params, iid, tid, duplicates=dup,
                                           diag_offset=0, col_chunk=4)
        assert float(got.detach()) == 0.0
        for g in _grads(got, params):
            assert float(g.abs().max()) == 0.0      # and so not NaN


def test_ids_compare_as_64_bit():
    params = _inputs(5, 9, 8, seed=5)
    iid, tid = _ids(5, 9, seed=5)
    ref = softmax_contrastive_loss_ids(*params, iid, tid)
    hi = 2 ** 40
    got = softmax_contrastive_loss_ids(
        *params, torch.where(iid >= 0, iid + hi, iid),
        torch.where(tid >= 0, tid + hi, tid))
    assert torch.equal(got, ref)
    # ids that agree in their low 32 bits only are different ids
    split = softmax_contrastive_loss_ids(
        *params, torch.where(iid >= 0, iid + 2 ** 32, iid), tid)
    assert float(split.detach()) == 0.0


def test_rejects_bad_arguments():
    zi, zt, tp = _inputs(4, 4, 8)
    ids = torch.arange(4)
    with pytest.raises(ValueError):
        softmax_contrastive_loss_ids(zi, zt[:, :4], tp, ids, ids)
    with pytest.raises(ValueError):
        softmax_contrastive_loss_ids(zi, zt, tp, ids, ids, impl="triton")
    with pytest.raises(ValueError):
        softmax_contrastive_loss_ids(zi, zt, tp, ids, ids, duplicates="drop")
    with pytest.raises(ValueError):
        softmax_contrastive_loss_ids(zi, zt, tp, ids[:3], ids)
    with pytest.raises(ValueError):
        softmax_contrastive_loss_ids(zi, zt, tp, ids, ids.float())


# ---------------------------------------------------------------------------
# gloo: W ranks against one process on the global batch.
# ---------------------------------------------------------------------------

B_RANK, DIM = 6, 8


def _global(world):
    """Ids repeat with period B_RANK, so the positives of a column (and of a
    row) live on every rank; one padding image and one padding text."""
    g = torch.Generator().manual_seed(11)
    zi = F.normalize(torch.randn(world * B_RANK, DIM, generator=g), dim=-1)
    zt = F.normalize(torch.randn(world * B_RANK, DIM, generator=g), dim=-1)
    iid = torch.arange(world * B_RANK) % B_RANK
    tid = torch.arange(world * B_RANK) % B_RANK
    iid[B_RANK + 1], tid[2] = -1, -1
    tid[4] = 77                     # a text nobody matches
    return zi, zt, iid, tid


def _module_worker(rank, world, dup, scale_by_rank):
    zi_all, zt_all, iid, tid = _global(world)
    sl = slice(rank * B_RANK, (rank + 1) * B_RANK)
    zi = zi_all[sl].clone().requires_grad_()
    zt = zt_all[sl].clone().requires_grad_()
    mod = DistributedSoftmaxLoss(B_RANK)
    loss = mod(zi, zt, image_ids=iid[sl], text_ids=tid[sl], duplicates=dup)
    (loss * (rank + 1) if scale_by_rank else loss).backward()
    # Every embedding lives on one rank: its gradient summed over ranks.
    gi = torch.zeros_like(zi_all)
    gt = torch.zeros_like(zt_all)
    gi[sl], gt[sl] = zi.grad, zt.grad
    gtp = mod.t_prime.grad.clone()
    for t in (gi, gt, gtp):
        dist.all_reduce(t)
    if rank == 0:
        return float(loss.detach()), gi, gt, gtp


def _single_process(world, dup, weights):
    """Autograd of Σ_q w_q·loss_q, every rank's loss from the textbook form:
    its rows (normalised over all columns) and its own columns (normalised
    over the rows of all ranks)."""
    zi_all, zt_all, iid, tid = _global(world)
    zi = zi_all.clone().requires_grad_()
    zt = zt_all.clone().requires_grad_()
    tp = torch.tensor(math.log(1 / 0.07)).requires_grad_()
    total = 0.0
    for q in range(world):
        sl = slice(q * B_RANK, (q + 1) * B_RANK)
        total = total + weights[q] * _textbook(
            zi, zt, tp, iid, tid, dup, 0, rows=sl, cols=sl) / (2 * B_RANK)
    total.backward()
    return zi.grad, zt.grad, tp.grad


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("dup", ["positive", "ignore"])
def test_gloo_averaged_grads_match_single_rank(world, dup):
    loss0, gi, gt, gtp = run_distributed(_module_worker, world, dup,
                                         False)[0]
    zi_all, zt_all, iid, tid = _global(world)
    pos, _ = _classes(iid, tid, dup, 0)
    if dup == "positive":   # a column's positives sit on several ranks
        assert int(pos[:B_RANK].sum(0).max()) >= 1
        assert int(pos[B_RANK:].sum(0).max()) >= 1
        assert int(pos.sum(0).max()) >= 2
    zi = zi_all.clone().requires_grad_()
    zt = zt_all.clone().requires_grad_()
    mod = DistributedSoftmaxLoss(world * B_RANK)
    mod(zi, zt, image_ids=iid, text_ids=tid, duplicates=dup).backward()
    # DDP averaging: the sum over ranks divided by W.
    torch.testing.assert_close(gi / world, zi.grad, rtol=1e-3, atol=1e-6)
    torch.testing.assert_close(gt / world, zt.grad, rtol=1e-3, atol=1e-6)
    torch.testing.assert_close(gtp / world, mod.t_prime.grad, rtol=1e-3,
                               atol=1e-6)
    assert math.isfinite(loss0)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("dup", ["positive", "ignore"])
def test_gloo_unequal_upstream(world, dup):
    _, gi, gt, gtp = run_distributed(_module_worker, world, dup, True)[0]
    ri, rt, rtp = _single_process(world, dup,
                                  [q + 1 for q in range(world)])
    torch.testing.assert_close(gi, ri, rtol=1e-3, atol=1e-6)
    torch.testing.assert_close(gt, rt, rtol=1e-3, atol=1e-6)
    torch.testing.assert_close(gtp, rtp, rtol=1e-3, atol=1e-6)


def _bad_layout_worker(rank, world):
    zi_all, zt_all, iid, tid = _global(world)
    zi = zi_all[rank * B_RANK:(rank + 1) * B_RANK]
    ids = iid[rank * B_RANK:(rank + 1) * B_RANK]
    with pytest.raises(ValueError):
        softmax_contrastive_loss_ids(
            zi, zt_all, torch.tensor(0.0), ids, tid, duplicates="ignore",
            diag_offset=0 if rank else B_RANK, group=dist.group.WORLD)
    with pytest.raises(ValueError):
        softmax_contrastive_loss_ids(
            zi, zt_all[:-1], torch.tensor(0.0), ids, tid[:-1],
            group=dist.group.WORLD)
    return True


def test_gloo_rejects_wrong_layout():
    assert run_distributed(_bad_layout_worker, 2)[0]


# ---------------------------------------------------------------------------
# Module.
# ---------------------------------------------------------------------------

def test_module_needs_both_id_vectors():
    zi, zt, _ = _inputs(4, 4, 8, dtype=torch.float32)
    mod = DistributedSoftmaxLoss(4)
    with pytest.raises(ValueError, match="together"):
        mod(zi, zt, image_ids=torch.arange(4))
    with pytest.raises(ValueError, match="together"):
        mod(zi, zt, text_ids=torch.arange(4))


def test_module_without_ids_is_unchanged():
    zi, zt, _ = _inputs(6, 6, 8, dtype=torch.float32)
    mod = DistributedSoftmaxLoss(6)
    got = mod(zi, zt)
    ref = softmax_contrastive_loss(
        zi, zt, mod.t_prime.clamp(max=math.log(mod.max_logit_scale)),
        diag_offset=0, col_chunk=None, impl="auto", group=None) / 12
    assert torch.equal(got, ref)
    ga = _grads(got, (zi, zt, mod.t_prime))
    gb = _grads(ref, (zi, zt, mod.t_prime))
    assert all(torch.equal(a, b) for a, b in zip(ga, gb))


def test_module_with_ids_normalises_by_batch():
    zi, zt, _ = _inputs(6, 6, 8, dtype=torch.float32)
    iid = torch.tensor([0, 0, 1, -1, 2, 3])
    tid = torch.tensor([0, 1, 1, 2, -1, 9])
    mod = DistributedSoftmaxLoss(6)
    t_prime = mod.t_prime.clamp(max=math.log(mod.max_logit_scale))
    for dup in ("positive", "ignore"):
        got = mod(zi, zt, image_ids=iid, text_ids=tid, duplicates=dup)
        ref = _textbook(zi, zt, t_prime, iid, tid, dup, 0) / 12
        torch.testing.assert_close(got, ref, rtol=1e-5, atol=1e-6)
