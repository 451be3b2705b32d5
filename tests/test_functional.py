"""Unit tests of the op-level loss core (CPU path) against a direct
materialized-label formula, plus the manual backward used by the fused
distributed Function."""

import dataclasses
import math

import pytest
import torch
import torch.nn.functional as F

from distributed_sigmoid_loss_amd.losses.functional import (
    sigmoid_contrastive_loss,
    chunk_loss_fwd,
    chunk_loss_bwd,
    _torch_bwd,
)


def naive_loss(zimg, ztxt, t_prime, bias, diag_offset):
    """Direct formula with materialized labels (the reference's shape,
    rwightman_sigmoid_loss.py:43-66)."""
    b, n = zimg.shape[0], ztxt.shape[0]
    logits = zimg @ ztxt.T * t_prime.exp() + bias
    labels = -torch.ones(b, n)
    if diag_offset is not None:
        for i in range(b):
            j = i + diag_offset
            if 0 <= j < n:
                labels[i, j] = 1.0
    return -F.logsigmoid(labels * logits).sum()


def rand_inputs(b, n, d, seed=0):
    g = torch.Generator().manual_seed(seed)
    zi = F.normalize(torch.randn(b, d, generator=g), dim=-1)
    zt = F.normalize(torch.randn(n, d, generator=g), dim=-1)
    tp = torch.tensor(math.log(10.0), requires_grad=True)
    bs = torch.tensor(-10.0, requires_grad=True)
    return zi, zt, tp, bs


@pytest.mark.parametrize("b,n,diag", [
    (8, 8, 0), (8, 8, None), (6, 18, 6), (6, 18, None), (9, 5, -2), (5, 9, 7),
])
@pytest.mark.parametrize("col_chunk", [None, 4])
def test_loss_matches_naive(b, n, diag, col_chunk):
    zi, zt, tp, bs = rand_inputs(b, n, 16)
    got = sigmoid_contrastive_loss(zi, zt, tp, bs, diag_offset=diag,
                                   col_chunk=col_chunk)
    want = naive_loss(zi, zt, tp, bs, diag)
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("diag", [0, None, 3])
def test_autograd_grads_match_naive(diag):
    zi, zt, tp, bs = rand_inputs(8, 12, 16, seed=1)
    zi = zi.clone().requires_grad_(True)
    zt = zt.clone().requires_grad_(True)
    loss = sigmoid_contrastive_loss(zi, zt, tp, bs, diag_offset=diag,
                                    col_chunk=5)
    loss.backward()

    zi2 = zi.detach().clone().requires_grad_(True)
    zt2 = zt.detach().clone().requires_grad_(True)
    tp2 = tp.detach().clone().requires_grad_(True)
    bs2 = bs.detach().clone().requires_grad_(True)
    naive_loss(zi2, zt2, tp2, bs2, diag).backward()

    for a, bgrad in [(zi.grad, zi2.grad), (zt.grad, zt2.grad),
                     (tp.grad, tp2.grad), (bs.grad, bs2.grad)]:
        assert torch.allclose(a, bgrad, rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("diag", [0, None, -3])
@pytest.mark.parametrize("go", [1.0, 0.37])
def test_manual_bwd_matches_autograd(diag, go):
    """_torch_bwd (used by the hand-written distributed Function) must equal
    autograd on the differentiable path, including grad_output scaling."""
    zi, zt, tp, bs = rand_inputs(7, 11, 16, seed=2)
    zi_a = zi.clone().requires_grad_(True)
    zt_a = zt.clone().requires_grad_(True)
    tp_a = tp.detach().clone().requires_grad_(True)
    bs_a = bs.detach().clone().requires_grad_(True)
    loss = sigmoid_contrastive_loss(zi_a, zt_a, tp_a, bs_a, diag_offset=diag)
    (loss * go).backward()

    dzi, dzt, dtp, dbs = _torch_bwd(zi, zt, tp.detach(), bs.detach(), diag,
                                    torch.tensor(go), col_chunk=4)
    assert torch.allclose(dzi, zi_a.grad, rtol=1e-5, atol=1e-7)
    assert torch.allclose(dzt, zt_a.grad, rtol=1e-5, atol=1e-7)
    assert torch.allclose(dtp, tp_a.grad, rtol=1e-5, atol=1e-7)
    assert torch.allclose(dbs, bs_a.grad, rtol=1e-5, atol=1e-7)


def test_chunk_fwd_bwd_helpers_consistent():
    zi, zt, tp, bs = rand_inputs(6, 10, 8, seed=3)
    full = chunk_loss_fwd(zi, zt, tp, bs, diag_offset=2)
    chunked = chunk_loss_fwd(zi, zt, tp, bs, diag_offset=2, col_chunk=3)
    assert torch.allclose(full, chunked, rtol=1e-6, atol=1e-7)

    g1 = chunk_loss_bwd(zi, zt, tp, bs, 2, torch.tensor(1.0), col_chunk=None)
    g2 = chunk_loss_bwd(zi, zt, tp, bs, 2, torch.tensor(1.0), col_chunk=3)
    for a, b_ in zip(g1, g2):
        assert torch.allclose(a, b_, rtol=1e-6, atol=1e-7)


def test_chunk_helpers_ignore_qcache_on_torch_path():
    """qcache= is forwarded to the HIP ops only; the torch path returns the
    same values with and without the argument."""
    zi, zt, tp, bs = rand_inputs(6, 10, 8, seed=4)
    go = torch.tensor(0.5)
    assert torch.equal(
        chunk_loss_fwd(zi, zt, tp, bs, diag_offset=2, qcache=None),
        chunk_loss_fwd(zi, zt, tp, bs, diag_offset=2))
    with_q = chunk_loss_bwd(zi, zt, tp, bs, 2, go, col_chunk=3, qcache=None)
    without = chunk_loss_bwd(zi, zt, tp, bs, 2, go, col_chunk=3)
    for a, b_ in zip(with_q, without):
        assert torch.equal(a, b_)


@pytest.mark.parametrize("rowwise", [False, True])
def test_quant_cache_round_trip(rowwise):
    """QuantCache flattens to tensors (save_for_backward) and rebuilds
    field for field, for both policies."""
    from distributed_sigmoid_loss_amd.ops import QuantCache
    g = torch.Generator().manual_seed(5)
    zi_q, zt_q = torch.randn(4, 16, generator=g), torch.randn(6, 16,
                                                              generator=g)
    if rowwise:
        c = QuantCache(
            zi_q, zt_q,
            zi_e8=torch.randint(0, 255, (4,), generator=g).to(torch.uint8),
            zt_e8=torch.randint(0, 255, (6,), generator=g).to(torch.uint8),
            zi_ratio=torch.rand(4, generator=g),
            zt_ratio=torch.rand(6, generator=g),
            si_ref=torch.tensor(0.25), st_ref=torch.tensor(0.5))
    else:
        c = QuantCache(zi_q, zt_q, torch.tensor(0.01), torch.tensor(0.02))
    assert c.rowwise is rowwise
    ts = c.tensors()
    assert len(ts) == (8 if rowwise else 4)
    assert all(isinstance(t, torch.Tensor) for t in ts)
    r = QuantCache.from_tensors(ts)
    assert r.rowwise is rowwise
    for f in dataclasses.fields(QuantCache):
        a, b_ = getattr(c, f.name), getattr(r, f.name)
        assert (a is None and b_ is None) or (a is b_), f.name
    with pytest.raises(ValueError):
        QuantCache.from_tensors(ts[:3])


def test_shape_validation():
    zi = torch.randn(4, 8)
    zt = torch.randn(4, 6)
    with pytest.raises(ValueError):
        sigmoid_contrastive_loss(zi, zt, torch.tensor(0.0), torch.tensor(0.0))
