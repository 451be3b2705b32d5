"""``sigmoid_contrastive_loss_ids(impl="hip", quant="mxfp8")`` through autograd,
saved-g and band recompute (``col_chunk=100``), gradients of ``total / b``;
regime of ``test_gpu_id_loss.py``.  Everything against a float64 emulation of
the policy: logits from the dequantised ``quantize_mx`` operands ``q·2^(code −
127)``, then the ``mixed`` backward — ``g`` rounded through e4m3 ×448, times
the other operand as the GEMM sees it (``quantize_fp8_pair``'s dequantised
per-tensor values on the fp8 hipBLASLt route, plain bf16 where ``grad_gemms``
dequantises ``g``; ``ops._mm8_ok`` says which).  Bounds: those of
``test_gpu_id_loss_fp8.py``, the backward being the same code: scalars within
``1e-4·Σ|term|``, embedding gradients within ``test_gpu_id_loss_mixed.py``'s
three-term bound.  ``(304, 336, 96)`` saved-g takes the fp8 route; every band
of 100 and ``(300, 333, 96)`` dequantise.  ``d = 96``: three K-blocks."""

import math

import pytest
import torch

from distributed_sigmoid_loss_amd import ops
from distributed_sigmoid_loss_amd.losses.id_labels import pair_classes
from test_gpu_id_loss import BIAS, MODES, _values     # skips without a GPU
from test_gpu_id_loss_mixed import _bound, _hip, _rel

pytestmark = pytest.mark.gpu
SHAPES = [(304, 336, 96), (300, 333, 96)]


def _mx_values(x):
    q, e8 = ops.quantize_mx(x)
    scale = torch.exp2(e8[:, :x.shape[1] // 32].double() - 127)
    return q.float().double() * scale.repeat_interleave(32, dim=1)


def _emulation(b, n, d, duplicates, diag, fp8_route):
    """((loss, dzimg, dztxt, dt', dbias), Σ|term| of the three scalars)."""
    zi, zt, tp0, img, txt = _values(b, n, d)
    t = math.exp(tp0)
    pos, masked = pair_classes(img, txt, duplicates, diag)
    lab = torch.where(pos, 1.0, -1.0).double()
    s = _mx_values(zi) @ _mx_values(zt).T
    x = -lab * (t * s + BIAS)
    term = torch.nn.functional.softplus(x, threshold=1e9).masked_fill(masked, 0)
    g = (-lab * torch.sigmoid(x)).masked_fill(masked, 0.0)
    g8 = (448.0 * g).float().to(torch.float8_e4m3fn).double() / 448.0
    oi, ot = zi.double(), zt.double()
    if fp8_route:
        qc = ops.quantize_fp8_pair(zi, zt)
        oi = qc.zi_q.float().double() * qc.si.double()
        ot = qc.zt_q.float().double() * qc.st.double()
    scalars = [term, t / b * g * s, g / b]
    return ((scalars[0].sum(), t / b * (g8 @ ot), t / b * (g8.T @ oi),
             scalars[1].sum(), scalars[2].sum()),
            [float(v.abs().sum()) for v in scalars])


@pytest.mark.parametrize("b,n,d", SHAPES)
@pytest.mark.parametrize("duplicates,diag", MODES)
@pytest.mark.parametrize("col_chunk", [None, 100])
def test_mxfp8_against_emulation(b, n, d, duplicates, diag, col_chunk):
    got = _hip(b, n, d, duplicates, diag, col_chunk, quant="mxfp8")
    fp8_route = ops._mm8_ok(b, d, n, min(n, col_chunk or n))
    assert fp8_route == ((b, n, col_chunk) == (304, 336, None)), "routes"
    emu, mags = _emulation(b, n, d, duplicates, diag, fp8_route)
    for i, mag in zip((0, 3, 4), mags):         # loss, dt', dbias
        err = abs(float(got[i].double() - emu[i]))
        assert err <= 1e-4 * mag, (i, err, mag)
    for i in (1, 2):                            # dzimg, dztxt
        assert _rel(got[i], emu[i]) <= _bound(col_chunk), i
