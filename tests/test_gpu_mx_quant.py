"""``ops.quantize_mx`` on the GPU: ``q`` and ``e8`` byte-equal with the torch
composite (``test_mx_quant.py`` holds that one to float64).  Gaussians times
``2^(r + c)``, ``r`` per row and ``c`` per block in ``−10 … 10`` (``2^−20 …
2^20``), a zero block in every seventh row.  ``(1, 32)`` one lane; ``(130,
160)``, ``(257, 416)`` pad bytes, rows straddling waves, a partial last wave;
``(8192, 768)`` 196608 scale bytes on 131072 lanes: the grid-stride step and
its carry (131072 mod 24 = 8).  ``(2, 160)``: ``test_mx_quant.py``'s blocks."""

import pytest
import torch

from distributed_sigmoid_loss_amd import ops
from test_mx_quant import _tensor

pytestmark = pytest.mark.gpu
U8 = torch.uint8

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)


@pytest.mark.parametrize("rows,d", [(1, 32), (130, 160), (257, 416),
                                    (8192, 768), (2, 160)])
def test_kernel_is_byte_equal_with_the_composite(rows, d):
    if (rows, d) == (2, 160):
        x = _tensor()
    else:
        gen = torch.Generator().manual_seed(rows * 7919 + d)
        r = torch.randint(-10, 11, (rows, 1, 1), generator=gen)
        c = torch.randint(-10, 11, (rows, d // 32, 1), generator=gen)
        x = torch.randn(rows, d // 32, 32, generator=gen) * torch.exp2(r + c)
        x[::7, 0] = 0.0
        x = x.reshape(rows, d).bfloat16()
    want_q, want_e8 = ops.quantize_mx(x)                     # CPU: composite
    q, e8 = ops.quantize_mx(x.cuda())
    assert (q.dtype, e8.dtype, e8.shape) == (want_q.dtype, U8, want_e8.shape)
    assert torch.equal(e8.cpu(), want_e8)
    assert torch.equal(q.cpu().view(U8), want_q.view(U8))
