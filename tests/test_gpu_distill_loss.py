"""``sigmoid_distillation_loss(impl="hip")`` through autograd against the torch
composite in float64 on the same bf16 values: saved-g and band recompute at
the two ragged shapes of ``test_gpu_distill_kernel.py`` (its inputs too);
``alpha = 0`` against the positional loss; the module at W = 1.  Tolerances
and the ``total / b`` upstream scale are those of ``test_gpu_id_loss.py``.
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from distributed_sigmoid_loss_amd import (
    DistributedSigmoidDistillLoss,
    sigmoid_contrastive_loss,
    sigmoid_distillation_loss,
)
from test_gpu_distill_kernel import BIAS, DEV, SHAPES, _case

EMB_TOL = dict(rtol=5e-2, atol=5e-4)
SCALAR_TOL = dict(rtol=2e-2, atol=1e-3)


@functools.lru_cache(maxsize=None)
def _run(shape, impl, alpha, diag, col_chunk=None, positional=False):
    """(loss, dzimg, dztxt, dt', dbias) at the ``total / b`` scale."""
    zi, zt, tp, _, ti, tt, tp_t, bias_t = _case(*shape)[0]
    dt = torch.float64 if impl == "torch" else torch.float32
    if impl == "torch":
        zi, zt = zi.double(), zt.double()
    zi, zt = zi.clone().requires_grad_(), zt.clone().requires_grad_()
    tp = tp.to(dt).clone().requires_grad_()
    bias = torch.tensor(BIAS, device=DEV, dtype=dt, requires_grad=True)
    ti, tt = ti.clone().requires_grad_(), tt.clone().requires_grad_()
    if positional:
        loss = sigmoid_contrastive_loss(zi, zt, tp, bias, diag_offset=diag,
                                        impl=impl)
    else:
        loss = sigmoid_distillation_loss(
            zi, zt, tp, bias, ti, tt, tp_t, bias_t, alpha, diag,
            col_chunk=col_chunk, impl=impl)
    (loss / shape[0]).backward()
    assert ti.grad is None and tt.grad is None
    return loss.detach(), zi.grad, zt.grad, tp.grad, bias.grad


def _compare(got, ref, tag):
    loss, dzi, dzt, dtp, db = got
    r_loss, r_dzi, r_dzt, r_dtp, r_db = (x.float() for x in ref)
    print(f"DISTILL_LOSS {tag} loss={float(loss):.4f}/{float(r_loss):.4f}"
          f" dzi={float((dzi.float() - r_dzi).abs().max()):.3e}"
          f" dzt={float((dzt.float() - r_dzt).abs().max()):.3e}"
          f" dtp={float(dtp):.5f}/{float(r_dtp):.5f} db={float(db):.5f}")
    torch.testing.assert_close(loss, r_loss, rtol=1e-4, atol=0)
    torch.testing.assert_close(dzi.float(), r_dzi, **EMB_TOL)
    torch.testing.assert_close(dzt.float(), r_dzt, **EMB_TOL)
    torch.testing.assert_close(dtp, r_dtp, **SCALAR_TOL)
    torch.testing.assert_close(db, r_db, **SCALAR_TOL)


@pytest.mark.parametrize("col_chunk", [None, 100])
@pytest.mark.parametrize("alpha,diag", [(1.0, None), (0.5, 3)])
@pytest.mark.parametrize("shape", SHAPES[2:])
def test_hip_matches_torch_composite(shape, alpha, diag, col_chunk):
    _compare(_run(shape, "hip", alpha, diag, col_chunk),
             _run(shape, "torch", alpha, diag),
             f"{shape} alpha={alpha} diag={diag} chunk={col_chunk}")


@pytest.mark.parametrize("diag", [None, 7])
def test_alpha_zero_is_the_positional_loss(diag):
    _compare(_run(SHAPES[2], "hip", 0.0, diag),
             _run(SHAPES[2], "hip", 0.0, diag, positional=True),
             f"{SHAPES[2]} alpha=0 diag={diag}")


def test_module_single_rank_and_auto():
    b = SHAPES[2][0]
    zi, zt, _, _, ti, tt, tp_t, _ = _case(*SHAPES[2])[0]
    mod = DistributedSigmoidDistillLoss(b, 0.5, float(tp_t), BIAS).to(DEV)
    with torch.no_grad():
        # auto is hip for bf16; the loss-only kernel leaves the same bits
        plain = sigmoid_distillation_loss(zi, zt, mod.t_prime, mod.bias, ti,
                                          tt, tp_t, BIAS, 0.5, 0)
    assert torch.equal(mod(zi, zt, ti, tt).detach(), plain / b)
    zi = zi.detach().clone().requires_grad_()
    mod(zi, zt, ti, tt).backward()
    for grad in (zi.grad, mod.t_prime.grad, mod.bias.grad):
        assert bool(torch.isfinite(grad).all())
