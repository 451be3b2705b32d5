"""``sigmoid_contrastive_loss_ids(impl="hip", quant="fp8")`` through autograd,
saved-g and band recompute (``col_chunk=100``), gradients of ``total / b``;
regime of ``test_gpu_id_loss.py``.  Everything against a float64 emulation of
the policy: logits from the dequantised ``quantize_fp8_pair`` operands, ``g``
rounded through e4m3 ×448, times the other operand as the GEMM sees it (the
dequantised e4m3 values on the fp8 hipBLASLt route, plain bf16 where
``grad_gemms`` dequantises ``g``; ``ops._mm8_ok`` says which, printed).  Loss,
``dt'`` and ``dbias`` are NOT the bf16 path's bits here — the logits are those
of the quantised embeddings — and are held to ``1e-4·Σ|term|`` of the
emulation's own sums.  Embedding gradients: the three-term bound derived in
``test_gpu_id_loss_mixed.py``.  Routes: ``(256, 256, 64)`` and ``(304, 336,
80)`` are 16-aligned in every dimension, so saved-g takes the fp8 route there;
every 100-column band, and ``(300, 333, 80)`` (added for it) in both regimes,
dequantise.  Bands against saved-g, at the last two shapes: twice the bound
(one per side, triangle inequality through the emulations) plus the distance
between the two emulations — exactly 0 at ``(300, 333, 80)``, where both
dequantise, and at ``(304, 336, 80)`` the e4m3 rounding of the other operand,
which the fp8 route sees and the bands do not (about 2 %)."""

import math

import pytest
import torch

from distributed_sigmoid_loss_amd import ops
from distributed_sigmoid_loss_amd.losses.id_labels import pair_classes
from test_gpu_id_loss import BIAS, MODES, _values     # skips without a GPU
from test_gpu_id_loss_mixed import _bound, _hip, _rel

pytestmark = pytest.mark.gpu
SHAPES = [(256, 256, 64), (304, 336, 80), (300, 333, 80)]


def _emulation(b, n, d, duplicates, diag, fp8_route):
    """((loss, dzimg, dztxt, dt', dbias), Σ|term| of the three scalars)."""
    zi, zt, tp0, img, txt = _values(b, n, d)
    qc, t = ops.quantize_fp8_pair(zi, zt), math.exp(tp0)
    zi_q = qc.zi_q.float().double() * qc.si.double()
    zt_q = qc.zt_q.float().double() * qc.st.double()
    pos, masked = pair_classes(img, txt, duplicates, diag)
    lab = torch.where(pos, 1.0, -1.0).double()
    s = zi_q @ zt_q.T
    x = -lab * (t * s + BIAS)
    term = torch.nn.functional.softplus(x, threshold=1e9).masked_fill(masked, 0)
    g = (-lab * torch.sigmoid(x)).masked_fill(masked, 0.0)
    g8 = (448.0 * g).float().to(torch.float8_e4m3fn).double() / 448.0
    oi, ot = (zi_q, zt_q) if fp8_route else (zi.double(), zt.double())
    scalars = [term, t / b * g * s, g / b]
    return ((scalars[0].sum(), t / b * (g8 @ ot), t / b * (g8.T @ oi),
             scalars[1].sum(), scalars[2].sum()),
            [float(v.abs().sum()) for v in scalars])


@pytest.mark.parametrize("b,n,d", SHAPES)
@pytest.mark.parametrize("duplicates,diag", MODES)
@pytest.mark.parametrize("col_chunk", [None, 100])
def test_fp8_against_emulation(b, n, d, duplicates, diag, col_chunk):
    got = _hip(b, n, d, duplicates, diag, col_chunk, quant="fp8")
    fp8_route = ops._mm8_ok(b, d, n, min(n, col_chunk or n))
    emu, mags = _emulation(b, n, d, duplicates, diag, fp8_route)
    tag = f"ID_FP8 {b}x{n}x{d}-{duplicates}-chunk{col_chunk}"
    for i, mag in zip((0, 3, 4), mags):         # loss, dt', dbias
        err = abs(float(got[i].double() - emu[i]))
        print(f"{tag}-{i} fp8_route={fp8_route} err/bound={err / (1e-4 * mag):.4f}")
        assert err <= 1e-4 * mag, (i, err, mag)
    for i in (1, 2):                            # dzimg, dztxt
        rel = _rel(got[i], emu[i])
        print(f"{tag}-{i} fp8_route={fp8_route} rel: hip-emulation {rel:.3e}")
        assert rel <= _bound(col_chunk), (i, rel)
        if col_chunk and (b, n, d) in SHAPES[1:]:   # bands against saved-g
            saved = _emulation(b, n, d, duplicates, diag,
                               ops._mm8_ok(b, d, n, n))[0][i]
            gap = _rel(emu[i], saved)   # the routes' operands; 0 if the same
            rel = _rel(got[i], _hip(b, n, d, duplicates, diag, None, "fp8")[i])
            print(f"{tag}-{i} bands-saved {rel:.3e} emulations {gap:.3e}")
            assert rel <= 2 * _bound(None) + gap, (i, rel, gap)
