"""``sigmoid_distillation_loss`` and ``softmax_distillation_loss`` with
``impl="hip", teacher_quant="mxfp8"`` through autograd against the torch
composite in float64 on the dequantised teacher (unit rows, every 32-block
times ``2^k``, ``k`` in ``−6 … 6``) at ``(129, 257, 72, 160)``: saved-g and
``col_chunk=100`` (three bands); a stored ``(q, e8)`` pair against its bf16
tensor; both modules at W = 1.  Comparisons and tolerances are those of
``test_gpu_distill_loss.py`` and ``test_gpu_softmax_distill_loss.py``."""

import functools

import pytest
import torch

from distributed_sigmoid_loss_amd import (
    DistributedSigmoidDistillLoss,
    DistributedSoftmaxDistillLoss,
    ops,
    sigmoid_distillation_loss,
    softmax_distillation_loss,
)
from test_gpu_distill_kernel import BIAS, DEV, _pair     # skips without a GPU
from test_gpu_distill_loss import _compare as _compare_sigmoid
from test_gpu_softmax_distill_loss import _compare as _compare_softmax
from test_gpu_distill_mx_teacher import SHAPES, _dequant, _tprime

pytestmark = pytest.mark.gpu
B, N, D, D_T = SHAPES[2]
COMPARE = {"sigmoid": _compare_sigmoid, "softmax": _compare_softmax}


@functools.lru_cache(maxsize=None)
def _inputs():
    gen = torch.Generator().manual_seed(20240607)
    zi, zt, tp, _, _ = _pair(B, N, D, gen)

    def teacher(r):
        k = torch.randint(-6, 7, (r, D_T // 32, 1), generator=gen).float()
        x = torch.nn.functional.normalize(
            torch.randn(r, D_T, generator=gen), dim=-1).view(r, -1, 32)
        return (x * torch.exp2(k)).reshape(r, D_T).bfloat16().to(DEV)

    tensors = teacher(B), teacher(N)
    pairs = tuple(ops.quantize_mx(x) for x in tensors)
    deq = tuple(_dequant(*p) for p in pairs)
    return zi, zt, tp, tensors, pairs, deq, _tprime(deq[0] @ deq[1].T)


def _loss(kind, zi, zt, tp, bias, ti, tt, tp_t, alpha, diag, **kw):
    if kind == "sigmoid":
        return sigmoid_distillation_loss(zi, zt, tp, bias, ti, tt, tp_t, BIAS,
                                         alpha, diag, **kw)
    return softmax_distillation_loss(zi, zt, tp, ti, tt, tp_t, alpha, diag,
                                     **kw)


@functools.lru_cache(maxsize=None)
def _run(kind, impl, alpha, diag, col_chunk=None, teacher="pair"):
    """(loss, dzimg, dztxt, dt'[, dbias]) at the ``total / b`` scale."""
    zi, zt, tp, tensors, pairs, deq, tp_t = _inputs()
    dt = torch.float64 if impl == "torch" else torch.float32
    if impl == "torch":          # float64 on the dequantised teacher
        zi, zt, (ti, tt), quant = zi.double(), zt.double(), deq, "bf16"
    else:
        (ti, tt), quant = (pairs if teacher == "pair" else tensors), "mxfp8"
    zi, zt = zi.clone().requires_grad_(), zt.clone().requires_grad_()
    tp = tp.to(dt).clone().requires_grad_()
    bias = torch.tensor(BIAS, device=DEV, dtype=dt, requires_grad=True)
    loss = _loss(kind, zi, zt, tp, bias, ti, tt, tp_t.to(dt), alpha, diag,
                 col_chunk=col_chunk, impl=impl, teacher_quant=quant)
    (loss / B).backward()
    out = (loss.detach(), zi.grad, zt.grad, tp.grad)
    return out + (bias.grad,) if kind == "sigmoid" else out


@pytest.mark.parametrize("col_chunk", [None, 100])
@pytest.mark.parametrize("alpha,diag", [(1.0, None), (0.5, 3)])
@pytest.mark.parametrize("kind", ["sigmoid", "softmax"])
def test_hip_matches_float64_composite(kind, alpha, diag, col_chunk):
    COMPARE[kind](_run(kind, "hip", alpha, diag, col_chunk),
                  _run(kind, "torch", alpha, diag),
                  f"mx {kind} alpha={alpha} diag={diag} chunk={col_chunk}")


@pytest.mark.parametrize("col_chunk", [None, 100])
@pytest.mark.parametrize("kind", ["sigmoid", "softmax"])
def test_stored_pair_and_its_tensor_give_the_same_bits(kind, col_chunk):
    for x, y in zip(_run(kind, "hip", 0.5, 3, col_chunk),
                    _run(kind, "hip", 0.5, 3, col_chunk, teacher="tensor")):
        assert torch.equal(x, y)


@pytest.mark.parametrize("kind", ["sigmoid", "softmax"])
def test_module_single_rank(kind):
    zi, zt, _, tensors, pairs, _, tp_t = _inputs()
    if kind == "sigmoid":
        mod, scale = DistributedSigmoidDistillLoss(
            B, 0.5, float(tp_t), BIAS, teacher_quant="mxfp8").to(DEV), B
    else:
        mod, scale = DistributedSoftmaxDistillLoss(
            B, 0.5, float(tp_t), teacher_quant="mxfp8").to(DEV), 2 * B
    with torch.no_grad():        # auto is hip for bf16 students and a pair
        plain = _loss(kind, zi, zt, mod.t_prime, mod.bias if kind == "sigmoid"
                      else None, *pairs, tp_t, 0.5, 0, teacher_quant="mxfp8")
        assert torch.equal(mod(zi, zt, *pairs), plain / scale)
        assert torch.equal(mod(zi, zt, *tensors), plain / scale)
    zi = zi.detach().clone().requires_grad_()
    mod(zi, zt, *pairs).backward()
    assert bool(torch.isfinite(zi.grad).all())
    assert bool(torch.isfinite(mod.t_prime.grad).all())
