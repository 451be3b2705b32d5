"""Sample-ID labels on CPU: the torch path of
``sigmoid_contrastive_loss_ids`` against a dense textbook evaluation in
float64 (explicit ``(b, n)`` label and mask matrices), its chunking and
equivalences, the distributed module over gloo against the single-rank
gradients of the global batch, the module's errors and the example's
``--captions-per-image`` flag.
"""

import math
import os
import subprocess
import sys

import pytest
import torch
import torch.distributed as dist
import torch.nn.functional as F

import distributed_sigmoid_loss_amd as pkg
from distributed_sigmoid_loss_amd import (
    DistributedSigmoidLoss,
    sigmoid_contrastive_loss,
    sigmoid_contrastive_loss_ids,
)
from helpers import run_distributed

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N, D = 13, 17, 8


def _inputs(b=B, n=N, d=D, dtype=torch.float64, seed=0):
    g = torch.Generator().manual_seed(seed)
    zi = F.normalize(torch.randn(b, d, generator=g, dtype=torch.float64), dim=-1)
    zt = F.normalize(torch.randn(n, d, generator=g, dtype=torch.float64), dim=-1)
    return (zi.to(dtype).requires_grad_(), zt.to(dtype).requires_grad_(),
            torch.tensor(math.log(4.0), dtype=dtype, requires_grad=True),
            torch.tensor(-0.5, dtype=dtype, requires_grad=True))


def _ids(b=B, n=N, seed=1):
    """Four values over 13 × 17: rows with several positives; value 9 on one
    row that no text carries; masked rows and columns."""
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 4, (b,), generator=g)
    txt = torch.randint(0, 4, (n,), generator=g)
    img[2], img[5], img[7] = -1, 9, -7
    txt[0], txt[11] = -1, -3
    return img, txt


def _dense(zi, zt, tp, bias, img, txt, duplicates, diag):
    """Textbook form: label and mask matrices written out."""
    b, n = zi.shape[0], zt.shape[0]
    lab = -torch.ones(b, n, dtype=zi.dtype)
    mask = torch.ones(b, n, dtype=zi.dtype)
    for i in range(b):
        for j in range(n):
            same = int(img[i]) == int(txt[j])
            on_diag = diag is not None and j == i + diag
            if int(img[i]) < 0 or int(txt[j]) < 0:
                mask[i, j] = 0.0
            elif duplicates == "positive":
                lab[i, j] = 1.0 if same else -1.0
            elif on_diag:
                lab[i, j] = 1.0
            elif same:
                mask[i, j] = 0.0
    z = tp.exp() * zi @ zt.T + bias
    return (mask * F.softplus(-lab * z, threshold=1e9)).sum(), lab, mask


CASES = [("positive", None), ("ignore", 0), ("ignore", 3), ("ignore", -2),
         ("ignore", None)]


@pytest.mark.parametrize("duplicates,diag", CASES)
def test_torch_path_matches_dense_textbook_fp64(duplicates, diag):
    img, txt = _ids()
    zi, zt, tp, bias = _inputs()
    ref, lab, mask = _dense(zi, zt, tp, bias, img, txt, duplicates, diag)
    # what the fixture is for
    pos = (lab > 0) & (mask > 0)
    assert bool((mask.sum(1) == 0).any()) and bool((mask.sum(0) == 0).any())
    if duplicates == "positive":
        assert bool((pos.sum(1) > 1).any())
        assert bool(((pos.sum(1) == 0) & (mask.sum(1) > 0)).any())
    else:
        assert bool(((mask == 0) & (img[:, None] >= 0)
                     & (txt[None, :] >= 0)).any())      # ignored duplicates
    ref_grads = torch.autograd.grad(ref, (zi, zt, tp, bias))
    got = sigmoid_contrastive_loss_ids(zi, zt, tp, bias, img, txt,
                                       duplicates=duplicates,
                                       diag_offset=diag, impl="torch")
    assert got.dtype == torch.float64 and got.dim() == 0
    torch.testing.assert_close(got, ref, rtol=1e-10, atol=0)
    grads = torch.autograd.grad(got, (zi, zt, tp, bias))
    for a, r in zip(grads, ref_grads):
        torch.testing.assert_close(a, r, rtol=1e-10, atol=1e-14)


@pytest.mark.parametrize("duplicates,diag", CASES)
@pytest.mark.parametrize("col_chunk", [1, 5, 17, 100])
def test_col_chunk_invariance(duplicates, diag, col_chunk):
    img, txt = _ids()
    zi, zt, tp, bias = _inputs()
    kw = dict(duplicates=duplicates, diag_offset=diag, impl="torch")
    whole = sigmoid_contrastive_loss_ids(zi, zt, tp, bias, img, txt, **kw)
    part = sigmoid_contrastive_loss_ids(zi, zt, tp, bias, img, txt,
                                        col_chunk=col_chunk, **kw)
    torch.testing.assert_close(part, whole, rtol=1e-12, atol=0)
    for a, r in zip(torch.autograd.grad(part, (zi, zt, tp, bias)),
                    torch.autograd.grad(whole, (zi, zt, tp, bias))):
        torch.testing.assert_close(a, r, rtol=1e-10, atol=1e-14)


@pytest.mark.parametrize("diag", [0, 4, -3])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_arange_ids_are_the_positional_loss(diag, dtype):
    zi, zt, tp, bias = _inputs(dtype=dtype)
    ref = sigmoid_contrastive_loss(zi, zt, tp, bias, diag_offset=diag,
                                   impl="torch")
    # a negative id would mask its row: shift both sides where diag < 0
    shift = max(0, -diag)
    got = sigmoid_contrastive_loss_ids(zi, zt, tp, bias,
                                       torch.arange(B) + diag + shift,
                                       torch.arange(N) + shift, impl="auto")
    assert got.dtype == dtype
    tol = dict(rtol=1e-10, atol=0) if dtype == torch.float64 else dict(
        rtol=1e-5, atol=0)
    torch.testing.assert_close(got, ref, **tol)
    # "ignore" with distinct ids is the positional loss as well
    got = sigmoid_contrastive_loss_ids(zi, zt, tp, bias, torch.arange(B),
                                       torch.arange(N) + 1000,
                                       duplicates="ignore", diag_offset=diag)
    torch.testing.assert_close(got, ref, **tol)


def test_all_masked_block_is_zero_without_nan():
    zi, zt, tp, bias = _inputs()
    off = torch.full((B,), -1)
    total = sigmoid_contrastive_loss_ids(zi, zt, tp, bias, off,
                                         torch.arange(N), impl="torch")
    assert float(total.detach()) == 0.0
    total.backward()
    for t in (zi, zt, tp, bias):
        assert bool(torch.isfinite(t.grad).all())
        assert float(t.grad.abs().max()) == 0.0


def test_ids_are_64_bit_values():
    zi, zt, tp, bias = _inputs()
    img, txt = _ids()
    base = sigmoid_contrastive_loss_ids(zi, zt, tp, bias, img, txt)
    shifted = sigmoid_contrastive_loss_ids(
        zi, zt, tp, bias, torch.where(img >= 0, img + (1 << 32), img), txt)
    none_pos = sigmoid_contrastive_loss_ids(
        zi, zt, tp, bias, torch.where(img >= 0, img + 100, img), txt)
    assert float(shifted.detach()) == float(none_pos.detach())
    assert float(shifted.detach()) != float(base.detach())


def test_argument_errors():
    zi, zt, tp, bias = _inputs()
    img, txt = _ids()
    with pytest.raises(ValueError, match="duplicates"):
        sigmoid_contrastive_loss_ids(zi, zt, tp, bias, img, txt,
                                     duplicates="keep")
    with pytest.raises(ValueError, match="impl"):
        sigmoid_contrastive_loss_ids(zi, zt, tp, bias, img, txt, impl="cuda")
    with pytest.raises(ValueError, match="txt_ids"):
        sigmoid_contrastive_loss_ids(zi, zt, tp, bias, img, txt[:-1])
    with pytest.raises(ValueError, match="img_ids"):
        sigmoid_contrastive_loss_ids(zi, zt, tp, bias, img.double(), txt)
    with pytest.raises(RuntimeError):      # hip needs bf16 on a GPU
        sigmoid_contrastive_loss_ids(zi, zt, tp, bias, img, txt, impl="hip")
    assert "sigmoid_contrastive_loss_ids" in pkg.__all__


# ---------------------------------------------------------------------------
# Module: single rank, errors, and the distributed oracle over gloo.
# ---------------------------------------------------------------------------

B_RANK, D_RANK = 6, 8


def _global(world):
    g = torch.Generator().manual_seed(11)
    zi = F.normalize(torch.randn(world * B_RANK, D_RANK, generator=g), dim=-1)
    zt = F.normalize(torch.randn(world * B_RANK, D_RANK, generator=g), dim=-1)
    # ids repeat within and across ranks; one masked sample on each side
    img = torch.arange(world * B_RANK) % 5
    txt = (torch.arange(world * B_RANK) * 2) % 5
    img[1], txt[world * B_RANK - 2] = -1, -1
    return zi, zt, img, txt


def test_module_single_rank_with_and_without_ids():
    zi, zt, img, txt = _global(2)
    mod = DistributedSigmoidLoss(zi.shape[0])
    for duplicates in ("positive", "ignore"):
        got = mod(zi, zt, image_ids=img, text_ids=txt, duplicates=duplicates)
        ref = sigmoid_contrastive_loss_ids(
            zi, zt, mod.t_prime, mod.bias, img, txt, duplicates=duplicates,
            diag_offset=0) / zi.shape[0]
        assert torch.equal(got, ref)
    # without ids: the same code path as before
    plain = sigmoid_contrastive_loss(zi, zt, mod.t_prime, mod.bias,
                                     diag_offset=0) / zi.shape[0]
    assert torch.equal(mod(zi, zt), plain)
    # a ring module at W = 1 takes ids too
    ring = DistributedSigmoidLoss(zi.shape[0], strategy="ring")
    assert torch.equal(ring(zi, zt, image_ids=img, text_ids=txt),
                       mod(zi, zt, image_ids=img, text_ids=txt))


def test_module_errors():
    zi, zt, img, txt = _global(1)
    mod = DistributedSigmoidLoss(B_RANK)
    with pytest.raises(ValueError, match="together"):
        mod(zi, zt, image_ids=img)
    with pytest.raises(ValueError, match="together"):
        mod(zi, zt, text_ids=txt)
    with pytest.raises(ValueError, match="all_gather.*bf16"):
        DistributedSigmoidLoss(B_RANK, quant="fp8")(
            zi, zt, image_ids=img, text_ids=txt)
    with pytest.raises(ValueError, match="all_gather.*bf16"):
        DistributedSigmoidLoss(B_RANK, quant="mixed")(
            zi, zt, image_ids=img, text_ids=txt)


def _module_worker(rank, world, duplicates):
    zi_all, zt_all, img, txt = _global(world)
    sl = slice(rank * B_RANK, (rank + 1) * B_RANK)
    zi = zi_all[sl].clone().requires_grad_()
    zt = zt_all[sl].clone().requires_grad_()
    # the ring form with ids is not built: it raises before any collective
    with pytest.raises(ValueError, match="all_gather.*bf16"):
        DistributedSigmoidLoss(B_RANK, strategy="ring")(
            zi, zt, image_ids=img[sl], text_ids=txt[sl])
    mod = DistributedSigmoidLoss(B_RANK)
    loss = mod(zi, zt, image_ids=img[sl], text_ids=txt[sl],
               duplicates=duplicates)
    loss.backward()
    gi, gt = torch.zeros_like(zi_all), torch.zeros_like(zt_all)
    gi[sl], gt[sl] = zi.grad, zt.grad
    gtp, gb = mod.t_prime.grad.clone(), mod.bias.grad.clone()
    for t in (gi, gt, gtp, gb):
        dist.all_reduce(t)
    losses = torch.zeros(world)
    losses[rank] = loss.detach()
    dist.all_reduce(losses)
    if rank == 0:
        return losses, gi, gt, gtp, gb


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("duplicates", ["positive", "ignore"])
def test_gloo_averaged_grads_match_single_rank(world, duplicates):
    losses, gi, gt, gtp, gb = run_distributed(
        _module_worker, world, duplicates)[0]
    zi_all, zt_all, img, txt = _global(world)
    zi = zi_all.clone().requires_grad_()
    zt = zt_all.clone().requires_grad_()
    mod = DistributedSigmoidLoss(world * B_RANK)
    ref = mod(zi, zt, image_ids=img, text_ids=txt, duplicates=duplicates)
    ref.backward()
    # the fixture has cross-rank positives (or ignored duplicates)
    eq = (img[:, None] == txt[None, :]) & (img[:, None] >= 0)
    cross = eq & (torch.arange(world * B_RANK)[:, None] // B_RANK
                  != torch.arange(world * B_RANK)[None, :] // B_RANK)
    assert bool(cross.any())
    # DDP averaging: the sum over ranks divided by W
    torch.testing.assert_close(losses.sum() / world, ref.detach(), rtol=1e-5,
                               atol=0)
    torch.testing.assert_close(gi / world, zi.grad, rtol=1e-3, atol=1e-6)
    torch.testing.assert_close(gt / world, zt.grad, rtol=1e-3, atol=1e-6)
    torch.testing.assert_close(gtp / world, mod.t_prime.grad, rtol=1e-3,
                               atol=1e-6)
    torch.testing.assert_close(gb / world, mod.bias.grad, rtol=1e-3,
                               atol=1e-6)


# ---------------------------------------------------------------------------
# Example.
# ---------------------------------------------------------------------------

def _example(*flags):
    return subprocess.run(
        [sys.executable, os.path.join(REPO, "examples", "train_siglip.py"),
         "--device", "cpu", "--batch-per-gpu", "8", "--dim", "64",
         "--steps", "2", "--log-every", "1", *flags],
        capture_output=True, text=True, cwd=REPO)


def test_example_captions_per_image_cpu():
    out = _example("--strategy", "all_gather", "--captions-per-image", "2")
    assert out.returncode == 0, out.stderr
    losses = [float(line.split("loss=")[1].split()[0])
              for line in out.stdout.splitlines() if "loss=" in line]
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses)


@pytest.mark.parametrize("flags", [
    ("--captions-per-image", "2"),                              # ring default
    ("--strategy", "all_gather", "--captions-per-image", "3"),  # 8 % 3
    ("--strategy", "all_gather", "--captions-per-image", "2", "--quant",
     "fp8"),
    ("--strategy", "all_gather", "--captions-per-image", "2", "--loss",
     "softmax"),
])
def test_example_rejects_unsupported_combinations(flags):
    out = _example(*flags)
    assert out.returncode == 2
    assert "captions-per-image" in out.stderr
