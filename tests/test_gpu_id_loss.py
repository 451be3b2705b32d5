"""``sigmoid_contrastive_loss_ids(impl="hip")`` through autograd against the
torch path in fp32 on the same bf16 values; band recompute against saved-g;
``arange`` ids against the positional loss; the module at W = 1.

Regime (that of ``test_gpu_id_labels.py``): L2-normalised Gaussian rows,
``t' = log(1.5 / std(s))``, ``bias = −0.5``, ids uniform over
``min(b, n) // 3`` values with 10 % of each side set to ``−1`` — every pair's
``|g|`` is of order 0.1 … 0.9, rows have several positives or none, and
masked rows and columns exist.

Tolerances: those of ``test_gpu_softmax_loss.py`` (the bf16 class of
``test_gpu_kernels.py``).  The loss is fp32 end to end (``rtol 1e-4``);
gradients pass through a bf16 g slab and bf16 GEMMs (``rtol 5e-2, atol 5e-4``
per embedding-gradient element, ``rtol 2e-2, atol 1e-3`` for ``t'`` and
``bias``).

Upstream scale.  As there, the gradients are taken at the module's
normalisation, here ``total / b``, because the element tolerance cannot be
applied to the sum form in this regime: a gradient entry ``t·Σ_j g_ij·ztxt_jk``
sums ``n`` terms of comparable size that partly cancel (no single positive
dominates, unlike at the SigLIP initialisation the positional tests use), and
each slab element carries a bf16 rounding of up to ``2⁻⁹|g|``.  With
``t ≈ 12.7``, ``|g| ≈ 0.4``, ``|ztxt_jk| ≈ 0.12`` and ``n = 333`` independent
roundings that is ``12.7·2⁻⁹·√333·0.4·0.12 ≈ 0.02`` per entry whatever the
kernel does, 40 times the absolute tolerance; at ``1 / b`` it is ``7e-5``, a
seventh of it.  Since the absolute term then carries much of the element
check, each embedding gradient is also held to a relative Frobenius error of
``2⁻⁷``: the slab rounding, the bf16 rounding of the scale and that of the
GEMM output, ``2⁻⁹`` each and independent, with a factor 2 of slack.
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
    DistributedSigmoidLoss,
    sigmoid_contrastive_loss,
    sigmoid_contrastive_loss_ids,
)

DEV = "cuda"
EMB_TOL = dict(rtol=5e-2, atol=5e-4)
SCALAR_TOL = dict(rtol=2e-2, atol=1e-3)
SHAPES = [(300, 333, 72), (256, 256, 64)]
MODES = [("positive", None), ("ignore", 3)]
BIAS = -0.5


@functools.lru_cache(maxsize=None)
def _values(b, n, d):
    g = torch.Generator().manual_seed(b * 1000003 + n * 7919 + d)
    zi = F.normalize(torch.randn(b, d, generator=g), dim=-1).bfloat16()
    zt = F.normalize(torch.randn(n, d, generator=g), dim=-1).bfloat16()
    std = float((zi.double() @ zt.double().T).std())
    values = min(b, n) // 3
    ids = []
    for length in (b, n):
        v = torch.randint(0, values, (length,), generator=g)
        v[torch.randperm(length, generator=g)[:length // 10]] = -1
        ids.append(v.to(DEV))
    return zi.to(DEV), zt.to(DEV), math.log(1.5 / std), ids[0], ids[1]


def _run(b, n, d, impl, duplicates="positive", diag=None, col_chunk=None,
         ids=None, positional=False):
    zi, zt, tp0, img, txt = _values(b, n, d)
    if ids is not None:
        img, txt = ids
    if impl == "torch":
        zi, zt = zi.float(), zt.float()
    zi = zi.detach().clone().requires_grad_()
    zt = zt.detach().clone().requires_grad_()
    tp = torch.tensor(tp0, device=DEV, requires_grad=True)
    bias = torch.tensor(BIAS, device=DEV, requires_grad=True)
    if positional:
        loss = sigmoid_contrastive_loss(zi, zt, tp, bias, diag_offset=diag,
                                        impl=impl)
    else:
        loss = sigmoid_contrastive_loss_ids(
            zi, zt, tp, bias, img, txt, duplicates=duplicates,
            diag_offset=diag, col_chunk=col_chunk, impl=impl)
    (loss / b).backward()
    return loss.detach(), zi.grad, zt.grad, tp.grad, bias.grad


@functools.lru_cache(maxsize=None)
def _reference(b, n, d, duplicates, diag):
    """The torch path in fp32 on the bf16 values, computed once; asserts the
    regime."""
    zi, zt, tp0, img, txt = _values(b, n, d)
    z = math.exp(tp0) * (zi.double() @ zt.double().T) + BIAS
    on = (img[:, None] >= 0) & (txt[None, :] >= 0)
    eq = (img[:, None] == txt[None, :]) & on
    a = torch.sigmoid(torch.where(eq, -z, z))[on]
    share = float(((a >= 0.05) & (a <= 0.95)).double().mean())
    assert share >= 0.9, f"uninformative regime: {share:.3f}"
    assert bool((eq.sum(1) > 1).any()) and bool((~on).any())
    assert bool(((eq.sum(1) == 0) & (img >= 0)).any())
    return _run(b, n, d, "torch", duplicates, diag)


def _compare(got, ref, loss_rtol, tag):
    loss, dzi, dzt, dtp, db = got
    r_loss, r_dzi, r_dzt, r_dtp, r_db = ref
    assert loss.dtype == torch.float32 and loss.dim() == 0
    assert dzi.dtype == torch.bfloat16 and dzt.dtype == torch.bfloat16
    rels = [float((x.float() - r.float()).norm() / r.float().norm())
            for x, r in ((dzi, r_dzi), (dzt, r_dzt))]
    print(f"ID_LOSS {tag} loss_rel={float((loss - r_loss).abs() / r_loss):.3e}"
          f" dzi={float((dzi.float() - r_dzi.float()).abs().max()):.3e}"
          f" dzt={float((dzt.float() - r_dzt.float()).abs().max()):.3e}"
          f" dtp={float(dtp):.5f}/{float(r_dtp):.5f}"
          f" db={float(db):.5f}/{float(r_db):.5f}"
          f" frobenius_rel={rels[0]:.3e},{rels[1]:.3e}")
    torch.testing.assert_close(loss, r_loss, rtol=loss_rtol, atol=0)
    torch.testing.assert_close(dzi.float(), r_dzi.float(), **EMB_TOL)
    torch.testing.assert_close(dzt.float(), r_dzt.float(), **EMB_TOL)
    torch.testing.assert_close(dtp, r_dtp, **SCALAR_TOL)
    torch.testing.assert_close(db, r_db, **SCALAR_TOL)
    assert max(rels) <= 2.0 ** -7, rels


@pytest.mark.parametrize("b,n,d", SHAPES)
@pytest.mark.parametrize("duplicates,diag", MODES)
def test_hip_matches_torch_path(b, n, d, duplicates, diag):
    got = _run(b, n, d, "hip", duplicates, diag)
    _compare(got, _reference(b, n, d, duplicates, diag), 1e-4,
             f"{b}x{n}x{d}-{duplicates}")


@pytest.mark.parametrize("duplicates,diag", MODES)
def test_band_recompute_matches_saved_g(duplicates, diag):
    b, n, d = SHAPES[0]
    whole = _run(b, n, d, "hip", duplicates, diag)
    banded = _run(b, n, d, "hip", duplicates, diag, col_chunk=100)
    torch.testing.assert_close(banded[0], whole[0], rtol=1e-5, atol=0)
    _compare(banded, _reference(b, n, d, duplicates, diag), 1e-4,
             f"{b}x{n}x{d}-{duplicates}-bands")
    torch.testing.assert_close(banded[1].float(), whole[1].float(), **EMB_TOL)
    torch.testing.assert_close(banded[2].float(), whole[2].float(), **EMB_TOL)
    torch.testing.assert_close(banded[3], whole[3], **SCALAR_TOL)
    torch.testing.assert_close(banded[4], whole[4], **SCALAR_TOL)


def test_no_grad_forward_is_the_same_loss_bits():
    """Without gradients the loss-only instantiation runs; its partials are
    those of the g-writing one, so the fp64 sums agree to the bit."""
    b, n, d = SHAPES[0]
    zi, zt, tp0, img, txt = _values(b, n, d)
    tp = torch.tensor(tp0, device=DEV)
    bias = torch.tensor(BIAS, device=DEV)
    with_grad = _run(b, n, d, "hip")[0]
    with torch.no_grad():
        plain = sigmoid_contrastive_loss_ids(zi, zt, tp, bias, img, txt)
    assert torch.equal(plain, with_grad)


@pytest.mark.parametrize("diag", [0, 7])
def test_arange_ids_match_the_positional_loss(diag):
    b, n, d = SHAPES[0]
    ids = (torch.arange(b, device=DEV) + diag, torch.arange(n, device=DEV))
    got = _run(b, n, d, "hip", ids=ids)
    ref = _run(b, n, d, "hip", diag=diag, positional=True)
    _compare(got, ref, 1e-4, f"{b}x{n}x{d}-arange+{diag}")


def test_auto_selects_hip_and_requires_bf16():
    b, n, d = SHAPES[1]
    zi, zt, tp0, img, txt = _values(b, n, d)
    tp = torch.tensor(tp0, device=DEV)
    bias = torch.tensor(BIAS, device=DEV)
    auto = sigmoid_contrastive_loss_ids(zi, zt, tp, bias, img, txt)
    hip = sigmoid_contrastive_loss_ids(zi, zt, tp, bias, img, txt, impl="hip")
    assert torch.equal(auto, hip)
    # auto on fp32 GPU tensors is the torch path; hip refuses them
    f32 = sigmoid_contrastive_loss_ids(zi.float(), zt.float(), tp, bias, img,
                                       txt)
    torch.testing.assert_close(f32, hip, rtol=1e-4, atol=0)
    with pytest.raises(RuntimeError, match="bf16"):
        sigmoid_contrastive_loss_ids(zi.float(), zt.float(), tp, bias, img,
                                     txt, impl="hip")


def test_module_single_rank():
    b, n, d = SHAPES[1]
    zi, zt, _, img, txt = _values(b, n, d)
    mod = DistributedSigmoidLoss(b, impl="hip").to(DEV)
    for duplicates in ("positive", "ignore"):
        got = mod(zi, zt, image_ids=img, text_ids=txt, duplicates=duplicates)
        fn = sigmoid_contrastive_loss_ids(
            zi, zt, mod.t_prime, mod.bias, img, txt, duplicates=duplicates,
            diag_offset=0, impl="hip") / b
        assert torch.equal(got, fn)
    # without ids: what the module returned before
    plain = sigmoid_contrastive_loss(zi, zt, mod.t_prime, mod.bias,
                                     diag_offset=0, impl="hip") / b
    assert torch.equal(mod(zi, zt), plain)
    # and gradients flow to the parameters through the id path
    zi = zi.detach().clone().requires_grad_()
    mod(zi, zt, image_ids=img, text_ids=txt).backward()
    assert bool(torch.isfinite(zi.grad).all())
    assert bool(torch.isfinite(mod.t_prime.grad))
    assert bool(torch.isfinite(mod.bias.grad))
