"""``sigmoid_contrastive_loss_ids(impl="hip", quant="mixed")`` through
autograd, saved-g and band recompute (``col_chunk=100``); regime and scale
``1 / b`` of ``test_gpu_id_loss.py``.  Loss, ``dt'``, ``dbias``: the bits of
the ``quant="bf16"`` hip path.  Embedding gradients: against a float64
emulation of the policy, ``g_ref`` rounded through e4m3 ×448 times the other
operand as the GEMM sees it — ``quantize_fp8_pair``'s values and scales on the
fp8 hipBLASLt route (saved-g at ``(256, 256, 64)``), plain bf16 where
``grad_gemms`` dequantises ``g`` (``(300, 333, 72)``; every 100-column band).
Bound on the relative Frobenius error, a sum of three: ``2⁻⁸``, bf16 rounding
of the scale (systematic; saved-g only); ``2⁻⁹``, bf16 rounding of the outputs
(per element); ``sqrt(1e-3)·0.125``, the allowed code flips (1e-3 of the
elements by one code of at most 12.5 %).  Against the exact fp32 torch path:
the emulation's own error plus that bound.  Bands against saved-g at
``(300, 333, 72)``, where both dequantise: twice the bound."""

import math

import pytest
import torch

from distributed_sigmoid_loss_amd import ops, sigmoid_contrastive_loss_ids
from distributed_sigmoid_loss_amd.losses.id_labels import pair_classes
from test_gpu_id_loss import BIAS, MODES, _reference, _values  # skips w/o GPU

pytestmark = pytest.mark.gpu
SHAPES = [(256, 256, 64), (300, 333, 72)]


def _bound(col_chunk):
    return (col_chunk is None) * 2.0 ** -8 + 2.0 ** -9 + 1e-3 ** 0.5 * 0.125


def _rel(x, ref):
    return float((x.double() - ref.double()).norm() / ref.double().norm())


def _hip(b, n, d, duplicates, diag, col_chunk, quant="mixed"):
    zi, zt, tp0, img, txt = _values(b, n, d)
    zi, zt = zi.clone().requires_grad_(), zt.clone().requires_grad_()
    tp, bias = (torch.tensor(v, device="cuda", requires_grad=True)
                for v in (tp0, BIAS))
    loss = sigmoid_contrastive_loss_ids(
        zi, zt, tp, bias, img, txt, duplicates=duplicates, diag_offset=diag,
        col_chunk=col_chunk, impl="hip", quant=quant)
    (loss / b).backward()
    return loss.detach(), zi.grad, zt.grad, tp.grad, bias.grad


def _emulation(b, n, d, duplicates, diag, fp8_operands):
    """(None, dzimg, dztxt) of the policy in float64."""
    zi, zt, tp0, img, txt = _values(b, n, d)
    t = math.exp(tp0)
    pos, masked = pair_classes(img, txt, duplicates, diag)
    lab = torch.where(pos, 1.0, -1.0).double()
    z = t * (zi.double() @ zt.double().T) + BIAS
    g = (-lab * torch.sigmoid(-lab * z)).masked_fill(masked, 0.0)
    g8 = (448.0 * g).float().to(torch.float8_e4m3fn).double() / 448.0
    if fp8_operands:
        qc = ops.quantize_fp8_pair(zi, zt)
        zi, zt = qc.zi_q.double() * qc.si, qc.zt_q.double() * qc.st
    return None, t / b * (g8 @ zt.double()), t / b * (g8.T @ zi.double())


@pytest.mark.parametrize("b,n,d", SHAPES)
@pytest.mark.parametrize("duplicates,diag", MODES)
@pytest.mark.parametrize("col_chunk", [None, 100])
def test_mixed_against_bf16_path_and_emulation(b, n, d, duplicates, diag,
                                               col_chunk):
    got = _hip(b, n, d, duplicates, diag, col_chunk)
    base = _hip(b, n, d, duplicates, diag, col_chunk, quant="bf16")
    # loss, dt', dbias: the same bits
    assert all(torch.equal(got[i], base[i]) for i in (0, 3, 4)), (got, base)
    fp8_route = ops._mm8_ok(b, d, n, min(n, col_chunk or n))
    emu, exact = (_emulation(b, n, d, duplicates, diag, fp8_route),
                  _reference(b, n, d, duplicates, diag))
    for i in (1, 2):                # dzimg, dztxt
        to_emu, to_exact, emu_exact = (
            _rel(got[i], emu[i]), _rel(got[i], exact[i]), _rel(emu[i], exact[i]))
        print(f"ID_MIXED {b}x{n}x{d}-{duplicates}-chunk{col_chunk}-{i} fp8_route="
              f"{fp8_route} rel: hip-emulation {to_emu:.3e} hip-exact "
              f"{to_exact:.3e} emulation-exact {emu_exact:.3e}")
        assert to_emu <= _bound(col_chunk), (i, to_emu)
        assert to_exact <= emu_exact + _bound(col_chunk), (i, to_exact)
        if col_chunk and (b, n, d) == SHAPES[1]:    # bands against saved-g
            rel = _rel(got[i], _hip(b, n, d, duplicates, diag, None)[i])
            assert rel <= 2 * _bound(None), (i, rel)
