"""``softmax_distillation_loss(impl="hip")`` through autograd against the torch
composite in float64 on the same bf16 values, whole block and ``col_chunk =
100``, at the ragged shape of ``test_gpu_softmax_distill_kernel.py`` (its
inputs too); ``alpha = 0`` against ``softmax_contrastive_loss``; the module at
W = 1.  Tolerances and the ``total / b`` upstream scale are those of
``test_gpu_distill_loss.py``.
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from distributed_sigmoid_loss_amd import (
    DistributedSoftmaxDistillLoss,
    softmax_contrastive_loss,
    softmax_distillation_loss,
)
from test_gpu_softmax_distill_kernel import DEV, SHAPES, _case

SHAPE = SHAPES[2]
EMB_TOL = dict(rtol=5e-2, atol=5e-4)
SCALAR_TOL = dict(rtol=2e-2, atol=1e-3)


@functools.lru_cache(maxsize=None)
def _run(impl, alpha, diag, col_chunk=None, hard=False):
    """(loss, dzimg, dztxt, dt') at the ``total / b`` scale."""
    zi, zt, tp, ti, tt, tp_t = _case(*SHAPE)[0]
    dt = torch.float64 if impl == "torch" else torch.float32
    if impl == "torch":
        zi, zt = zi.double(), zt.double()
    zi, zt = zi.clone().requires_grad_(), zt.clone().requires_grad_()
    tp = tp.to(dt).clone().requires_grad_()
    ti, tt = ti.clone().requires_grad_(), tt.clone().requires_grad_()
    if hard:
        loss = softmax_contrastive_loss(zi, zt, tp, diag, impl=impl)
    else:
        loss = softmax_distillation_loss(zi, zt, tp, ti, tt, tp_t.to(dt),
                                         alpha, diag, col_chunk=col_chunk,
                                         impl=impl)
    (loss / SHAPE[0]).backward()
    assert ti.grad is None and tt.grad is None
    return loss.detach(), zi.grad, zt.grad, tp.grad


def _compare(got, ref, tag):
    loss, dzi, dzt, dtp = got
    r_loss, r_dzi, r_dzt, r_dtp = (x.float() for x in ref)
    print(f"SOFTMAX_DISTILL_LOSS {tag} loss={float(loss):.4f}/"
          f"{float(r_loss):.4f}"
          f" dzi={float((dzi.float() - r_dzi).abs().max()):.3e}"
          f" dzt={float((dzt.float() - r_dzt).abs().max()):.3e}"
          f" dtp={float(dtp):.5f}/{float(r_dtp):.5f} grads_bit_equal="
          f"{torch.equal(dzi.float(), r_dzi) and torch.equal(dzt.float(), r_dzt)}")
    torch.testing.assert_close(loss, r_loss, rtol=1e-4, atol=0)
    torch.testing.assert_close(dzi.float(), r_dzi, **EMB_TOL)
    torch.testing.assert_close(dzt.float(), r_dzt, **EMB_TOL)
    torch.testing.assert_close(dtp, r_dtp, **SCALAR_TOL)


@pytest.mark.parametrize("col_chunk", [None, 100])
@pytest.mark.parametrize("alpha,diag", [(1.0, None), (0.5, 3)])
def test_hip_matches_float64_composite(alpha, diag, col_chunk):
    _compare(_run("hip", alpha, diag, col_chunk), _run("torch", alpha, diag),
             f"alpha={alpha} diag={diag} chunk={col_chunk}")


def test_alpha_zero_is_the_softmax_contrastive_loss():
    _compare(_run("hip", 0.0, 7), _run("hip", 0.0, 7, hard=True),
             "alpha=0 diag=7")


def test_module_single_rank_and_auto():
    b = SHAPE[0]
    zi, zt, _, ti, tt, tp_t = _case(*SHAPE)[0]
    mod = DistributedSoftmaxDistillLoss(b, 0.5, float(tp_t)).to(DEV)
    with torch.no_grad():       # auto is hip for bf16
        plain = softmax_distillation_loss(zi, zt, mod.t_prime, ti, tt, tp_t,
                                          0.5, 0, impl="hip")
    assert torch.equal(mod(zi, zt, ti, tt).detach(), plain / (2 * b))
    zi = zi.detach().clone().requires_grad_()
    mod(zi, zt, ti, tt).backward()
    for grad in (zi.grad, mod.t_prime.grad):
        assert bool(torch.isfinite(grad).all())
