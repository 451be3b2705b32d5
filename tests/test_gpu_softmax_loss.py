"""``softmax_contrastive_loss(impl="hip")`` through autograd against the torch
path in fp32 on the same bf16 values; column banding; the module at W = 1.

Tolerances: the loss is fp32 end to end (``rtol 1e-4``; the kernels' LSE bound
implies far less); gradients pass through a bf16 g slab and bf16 GEMMs, so
they take the bf16-class tolerances of ``test_gpu_kernels.py``
(``rtol 5e-2, atol 5e-4`` per embedding-gradient element).

Upstream scale.  The function is in sum form and the caller normalises; the
gradients are taken of ``total / (2 b)``, the module's normalisation.  The
element tolerance cannot be applied to the sum form itself: a softmax
gradient entry ``t·Σ_j g_ij·ztxt_jk`` is a sum of a positive pair's term
(``|g| ≈ 2``) and ``n − 1`` smaller ones that may cancel it, while each slab
element carries a bf16 rounding of up to ``2⁻⁹|g|`` — in the worst case
``t·2⁻⁹·Σ_j |g_ij|·max|ztxt|`` ≈ ``10 · 2⁻⁹ · 4 · 0.35`` ≈ 0.03 per entry,
60 times the absolute tolerance whatever the kernel does (the sigmoid tests
meet it in sum form because one term dominates every entry and the error is
relative to it).  At ``1 / (2 b)`` the worst case is ``0.03 / 600 = 5e-5``.
Since the absolute term then carries much of the element check, each
gradient is also held to a relative Frobenius error of ``2⁻⁷``: the slab
rounding and the two bf16 roundings of the GEMM output, ``2⁻⁹`` each and
independent, with a factor 2 of slack.
"""

import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from distributed_sigmoid_loss_amd import (
    DistributedSoftmaxLoss,
    softmax_contrastive_loss,
)

DEV = "cuda"
EMB_TOL = dict(rtol=5e-2, atol=5e-4)
TP_TOL = dict(rtol=2e-2, atol=1e-3)
DIAG = 3


def _values(b, n, d):
    g = torch.Generator().manual_seed(b * 31 + n)
    zi = F.normalize(torch.randn(b, d, generator=g), dim=-1)
    zt = F.normalize(torch.randn(n, d, generator=g), dim=-1)
    return zi.to(DEV).bfloat16(), zt.to(DEV).bfloat16()


def _run(zi, zt, impl, col_chunk=None):
    zi = zi.detach().clone().requires_grad_()
    zt = zt.detach().clone().requires_grad_()
    tp = torch.tensor(math.log(10.0), device=DEV, requires_grad=True)
    loss = softmax_contrastive_loss(zi, zt, tp, diag_offset=DIAG,
                                    col_chunk=col_chunk, impl=impl)
    (loss / (2 * zi.shape[0])).backward()
    return loss.detach(), zi.grad, zt.grad, tp.grad


@functools.lru_cache(maxsize=None)
def _reference(b, n, d):
    """The torch path in fp32 on the bf16 values, computed once."""
    zi, zt = _values(b, n, d)
    return _run(zi.float(), zt.float(), "torch")


def _compare(got, ref, loss_rtol):
    loss, dzi, dzt, dtp = got
    r_loss, r_dzi, r_dzt, r_dtp = ref
    assert loss.dtype == torch.float32 and dzi.dtype == torch.bfloat16
    print(f"SOFTMAX_LOSS loss_rel={float((loss - r_loss).abs() / r_loss):.3e}"
          f" dzi={float((dzi.float() - r_dzi).abs().max()):.3e}"
          f" dzt={float((dzt.float() - r_dzt).abs().max()):.3e}"
          f" dtp_rel={float((dtp - r_dtp).abs() / r_dtp.abs()):.3e}")
    torch.testing.assert_close(loss, r_loss, rtol=loss_rtol, atol=0)
    torch.testing.assert_close(dzi.float(), r_dzi, **EMB_TOL)
    torch.testing.assert_close(dzt.float(), r_dzt, **EMB_TOL)
    torch.testing.assert_close(dtp, r_dtp, **TP_TOL)
    for got_g, ref_g in ((dzi, r_dzi), (dzt, r_dzt)):
        rel = float((got_g.float() - ref_g).norm() / ref_g.norm())
        print(f"SOFTMAX_LOSS frobenius_rel={rel:.3e}")
        assert rel <= 2.0 ** -7, rel


@pytest.mark.parametrize("b,n,d", [(300, 333, 72), (256, 256, 64)])
def test_hip_matches_torch_path(b, n, d):
    _compare(_run(*_values(b, n, d), "hip"), _reference(b, n, d), 1e-4)


def test_banding_matches_whole_block():
    b, n, d = 300, 333, 72
    whole = _run(*_values(b, n, d), "hip")
    banded = _run(*_values(b, n, d), "hip", col_chunk=128)
    torch.testing.assert_close(banded[0], whole[0], rtol=1e-5, atol=0)
    _compare(banded, _reference(b, n, d), 1e-4)
    torch.testing.assert_close(banded[1].float(), whole[1].float(), **EMB_TOL)
    torch.testing.assert_close(banded[2].float(), whole[2].float(), **EMB_TOL)
    torch.testing.assert_close(banded[3], whole[3], **TP_TOL)


def test_auto_selects_hip_and_requires_bf16():
    zi, zt = _values(256, 256, 64)
    tp = torch.tensor(math.log(10.0), device=DEV)
    auto = softmax_contrastive_loss(zi, zt, tp)
    hip = softmax_contrastive_loss(zi, zt, tp, impl="hip")
    assert torch.equal(auto, hip)
    with pytest.raises(RuntimeError, match="bf16"):
        softmax_contrastive_loss(zi.float(), zt.float(), tp, impl="hip")


def test_module_single_rank_is_symmetric_clip_loss():
    b, d = 256, 64
    zi, zt = _values(b, b, d)
    mod = DistributedSoftmaxLoss(b, impl="hip").to(DEV)
    z = mod.t_prime.detach().exp() * zi.float() @ zt.float().T
    tgt = torch.arange(b, device=DEV)
    ref = 0.5 * (F.cross_entropy(z, tgt) + F.cross_entropy(z.T, tgt))
    zi.requires_grad_()
    loss = mod(zi, zt)
    torch.testing.assert_close(loss, ref, rtol=1e-4, atol=0)
    loss.backward()
    assert bool(torch.isfinite(zi.grad).all())
    assert bool(torch.isfinite(mod.t_prime.grad))
