"""``softmax_contrastive_loss_ids(impl="hip")`` through autograd against the
torch path in fp32 on the same bf16 values, in both ``duplicates`` modes;
column banding; ``arange`` ids against the positional loss; the module at
W = 1 with and without ids; an all-masked block.

Tolerances are those of ``test_gpu_softmax_loss.py``, for its reasons: the
loss is fp32 end to end (``rtol 1e-4``); gradients pass through a bf16 g slab
and bf16 GEMMs and are taken of ``total / (2 b)``, the module's
normalisation (``rtol 5e-2, atol 5e-4`` per embedding-gradient element plus a
relative Frobenius error of ``2⁻⁷``); ``t'`` takes ``rtol 2e-2, atol 1e-3``.

Ids: uniform over a third as many values as the longer side, so rows and
columns hold several positives, with every 29th image and every 31st text
masked by a negative id.
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
    softmax_contrastive_loss_ids,
)

DEV = "cuda"
EMB_TOL = dict(rtol=5e-2, atol=5e-4)
TP_TOL = dict(rtol=2e-2, atol=1e-3)
DIAG = 3
SHAPES = [(300, 333, 72), (256, 256, 64)]
MODES = ["positive", "ignore"]


def _values(b, n, d):
    g = torch.Generator().manual_seed(b * 31 + n)
    zi = F.normalize(torch.randn(b, d, generator=g), dim=-1)
    zt = F.normalize(torch.randn(n, d, generator=g), dim=-1)
    k = -(-max(b, n) // 3)
    iid = torch.randint(0, k, (b,), generator=g)
    tid = torch.randint(0, k, (n,), generator=g)
    iid[7::29], tid[11::31] = -1, -1
    return (zi.to(DEV).bfloat16(), zt.to(DEV).bfloat16(), iid.to(DEV),
            tid.to(DEV))


def _run(zi, zt, iid, tid, dup, impl, col_chunk=None):
    zi = zi.detach().clone().requires_grad_()
    zt = zt.detach().clone().requires_grad_()
    tp = torch.tensor(math.log(10.0), device=DEV, requires_grad=True)
    loss = softmax_contrastive_loss_ids(
        zi, zt, tp, iid, tid, duplicates=dup, diag_offset=DIAG,
        col_chunk=col_chunk, impl=impl)
    (loss / (2 * zi.shape[0])).backward()
    return loss.detach(), zi.grad, zt.grad, tp.grad


@functools.lru_cache(maxsize=None)
def _reference(b, n, d, dup):
    """The torch path in fp32 on the bf16 values, computed once."""
    zi, zt, iid, tid = _values(b, n, d)
    return _run(zi.float(), zt.float(), iid, tid, dup, "torch")


def _compare(got, ref, loss_rtol):
    loss, dzi, dzt, dtp = got
    r_loss, r_dzi, r_dzt, r_dtp = ref
    assert loss.dtype == torch.float32 and dzi.dtype == torch.bfloat16
    assert float(r_loss) > 0
    print(f"SOFTMAX_ID_LOSS loss_rel="
          f"{float((loss - r_loss).abs() / r_loss):.3e}"
          f" dzi={float((dzi.float() - r_dzi).abs().max()):.3e}"
          f" dzt={float((dzt.float() - r_dzt).abs().max()):.3e}"
          f" dtp_rel={float((dtp - r_dtp).abs() / r_dtp.abs()):.3e}")
    torch.testing.assert_close(loss, r_loss, rtol=loss_rtol, atol=0)
    torch.testing.assert_close(dzi.float(), r_dzi, **EMB_TOL)
    torch.testing.assert_close(dzt.float(), r_dzt, **EMB_TOL)
    torch.testing.assert_close(dtp, r_dtp, **TP_TOL)
    for got_g, ref_g in ((dzi, r_dzi), (dzt, r_dzt)):
        rel = float((got_g.float() - ref_g).norm() / ref_g.norm())
        print(f"SOFTMAX_ID_LOSS frobenius_rel={rel:.3e}")
        assert rel <= 2.0 ** -7, rel


@pytest.mark.parametrize("b,n,d", SHAPES)
@pytest.mark.parametrize("dup", MODES)
def test_hip_matches_torch_path(b, n, d, dup):
    vals = _values(b, n, d)
    got = _run(*vals, dup, "hip")
    _compare(got, _reference(b, n, d, dup), 1e-4)
    # masked rows and columns take exactly no gradient
    assert float(got[1][7::29].float().abs().max()) == 0.0
    assert float(got[2][11::31].float().abs().max()) == 0.0


@pytest.mark.parametrize("dup", MODES)
def test_banding_matches_whole_block(dup):
    b, n, d = SHAPES[0]
    whole = _run(*_values(b, n, d), dup, "hip")
    banded = _run(*_values(b, n, d), dup, "hip", col_chunk=100)
    torch.testing.assert_close(banded[0], whole[0], rtol=1e-5, atol=0)
    _compare(banded, _reference(b, n, d, dup), 1e-4)
    torch.testing.assert_close(banded[1].float(), whole[1].float(), **EMB_TOL)
    torch.testing.assert_close(banded[2].float(), whole[2].float(), **EMB_TOL)
    torch.testing.assert_close(banded[3], whole[3], **TP_TOL)


@pytest.mark.parametrize("b,n,d", SHAPES)
def test_arange_ids_are_the_positional_loss(b, n, d):
    zi, zt, _, _ = _values(b, n, d)
    iid = torch.arange(b, device=DEV) + DIAG
    tid = torch.arange(n, device=DEV)
    got = _run(zi, zt, iid, tid, "positive", "hip")

    zi = zi.detach().clone().requires_grad_()
    zt = zt.detach().clone().requires_grad_()
    tp = torch.tensor(math.log(10.0), device=DEV, requires_grad=True)
    loss = softmax_contrastive_loss(zi, zt, tp, diag_offset=DIAG, impl="hip")
    (loss / (2 * b)).backward()
    _compare(got, (loss.detach(), zi.grad.float(), zt.grad.float(), tp.grad),
             1e-4)


def test_auto_selects_hip_and_requires_bf16():
    zi, zt, iid, tid = _values(256, 256, 64)
    tp = torch.tensor(math.log(10.0), device=DEV)
    auto = softmax_contrastive_loss_ids(zi, zt, tp, iid, tid)
    hip = softmax_contrastive_loss_ids(zi, zt, tp, iid, tid, impl="hip")
    assert torch.equal(auto, hip)
    with pytest.raises(RuntimeError, match="bf16"):
        softmax_contrastive_loss_ids(zi.float(), zt.float(), tp, iid, tid,
                                     impl="hip")


def test_module_without_ids_is_the_parent_path():
    b, d = 256, 64
    zi, zt, _, _ = _values(b, b, d)
    mod = DistributedSoftmaxLoss(b, impl="hip").to(DEV)

    def grads(fn):
        a = zi.detach().clone().requires_grad_()
        t = zt.detach().clone().requires_grad_()
        mod.zero_grad()
        loss = fn(a, t)
        loss.backward()
        return loss.detach(), a.grad, t.grad, mod.t_prime.grad.clone()

    got = grads(lambda a, t: mod(a, t))
    ref = grads(lambda a, t: softmax_contrastive_loss(
        a, t, mod.t_prime.clamp(max=math.log(mod.max_logit_scale)),
        diag_offset=0, col_chunk=None, impl="hip", group=None) / (2 * b))
    assert all(torch.equal(x, y) for x, y in zip(got, ref))


@pytest.mark.parametrize("dup", MODES)
def test_module_with_ids(dup):
    b, d = 256, 64
    zi, zt, iid, tid = _values(b, b, d)
    mod = DistributedSoftmaxLoss(b, impl="hip").to(DEV)
    ref_mod = DistributedSoftmaxLoss(b, impl="torch").to(DEV)
    zi.requires_grad_()
    loss = mod(zi, zt, image_ids=iid, text_ids=tid, duplicates=dup)
    ref = ref_mod(zi.detach().float(), zt.float(), image_ids=iid,
                  text_ids=tid, duplicates=dup)
    torch.testing.assert_close(loss, ref, rtol=1e-4, atol=0)
    loss.backward()
    assert bool(torch.isfinite(zi.grad).all())
    assert bool(torch.isfinite(mod.t_prime.grad))
    with pytest.raises(ValueError, match="together"):
        mod(zi, zt, image_ids=iid)


@pytest.mark.parametrize("col_chunk", [None, 100])
def test_all_masked_block(col_chunk):
    b, n, d = SHAPES[0]
    zi, zt, _, tid = _values(b, n, d)
    iid = torch.full((b,), -1, device=DEV)
    for dup in MODES:
        loss, dzi, dzt, dtp = _run(zi, zt, iid, tid, dup, "hip", col_chunk)
        assert float(loss) == 0.0
        assert float(dzi.float().abs().max()) == 0.0
        assert float(dzt.float().abs().max()) == 0.0
        assert float(dtp) == 0.0
