"""``ops.sigmoid_ids_e4m3`` against float64 from the same bf16 inputs; regime,
ids and reference of ``test_gpu_id_labels.py``.  ``(128, 128, 64)`` one tile;
``(256, 384, 200)`` several, K tail of 8 (one unmasked row gets an id no text
carries: as drawn each has a positive); ``(300, 333, 72)`` ragged, no
multiples of 4.  ``"ignore"`` at offsets 1 and 400 (off every block).  Codes:
the bound of ``test_gpu_tile_exact.py`` for the positional slab pair."""

import functools

import pytest
import torch

from distributed_sigmoid_loss_amd import ops
from test_gpu_id_labels import _case, _reference   # skips without a GPU

pytestmark = pytest.mark.gpu
E4M3, U8 = torch.float8_e4m3fn, torch.uint8
SHAPES = [(128, 128, 64), (256, 384, 200), (300, 333, 72)]
MODES = [("positive", None), ("ignore", 1), ("ignore", 400)]


def _ordinal(codes):     # e4m3 byte → signed position on the value line
    mag = (codes & 0x7F).to(torch.int16)
    return torch.where(codes >= 128, -mag, mag)


@functools.lru_cache(maxsize=None)
def _setup(b, n, d, duplicates="positive", diag=None):
    c = _case(b, n, d)
    img_ids = c.img_ids.clone()
    if (b, n, d) == SHAPES[1]:
        img_ids[int((img_ids >= 0).nonzero()[0])] = 10 ** 6
    npos = _reference(c, img_ids, c.txt_ids).pos.sum(dim=1)
    assert bool((npos > 1).any()), "no row with several positives"
    assert bool(((npos == 0) & (img_ids >= 0)).any()), "no unmasked empty row"
    assert bool((img_ids < 0).any()) and bool((c.txt_ids < 0).any())
    args = (c.zi, c.zt, c.tp, c.bias, img_ids, c.txt_ids, duplicates, diag)
    return args, _reference(c, img_ids, c.txt_ids, duplicates, diag)


@pytest.mark.parametrize("b,n,d", SHAPES)
@pytest.mark.parametrize("duplicates,diag", MODES)
def test_codes_transpose_masks_and_partials(b, n, d, duplicates, diag):
    args, ref = _setup(b, n, d, duplicates, diag)
    partials, g, gt = ops.sigmoid_ids_e4m3(*args)
    assert (g.dtype, g.shape, gt.shape) == (gt.dtype, (b, n), (n, b))
    codes = g.view(U8)
    want = (448.0 * ref.g).float().contiguous().to(E4M3).view(U8)
    diff = (_ordinal(codes) - _ordinal(want)).abs()
    assert int(diff.max()) <= 1 and float((diff != 0).double().mean()) <= 1e-3
    assert torch.equal(gt.view(U8), codes.T)
    assert bool((codes[ref.masked] == 0).all()), "masked pair not 0x00"
    nz = (codes & 0x7F) != 0
    assert torch.equal(codes[nz] >= 128, ref.g[nz] < 0), "sign of a code"
    assert torch.equal(partials, ops.sigmoid_ids(*args)[0])
    for x, y in zip(ops.sigmoid_ids_e4m3(*args), (partials, g, gt)):
        assert torch.equal(x.view(U8), y.view(U8)), "run to run"


def test_views_into_wider_slabs_are_contained():
    (b, n, _), (args, _) = SHAPES[2], _setup(*SHAPES[2])   # byte-store path
    partials, g, gt = ops.sigmoid_ids_e4m3(*args)
    wide = torch.full((b, n + 8), 0x7F, device="cuda", dtype=U8)
    wide_t = torch.full((n + 7, b + 3), 0x7F, device="cuda", dtype=U8)
    gv, gtv = wide[:, 3:3 + n], wide_t[5:5 + n, 1:1 + b]
    p2, _, _ = ops.sigmoid_ids_e4m3(*args, g=gv.view(E4M3), gt=gtv.view(E4M3))
    assert torch.equal(p2, partials) and torch.equal(gv, g.view(U8))
    assert torch.equal(gtv, gt.view(U8))
    for buf, view in ((wide, gv), (wide_t, gtv)):
        view.fill_(0x7F)
        assert bool((buf == 0x7F).all()), "a byte outside the view changed"


@pytest.mark.parametrize("name,slab", [
    ("g", lambda: torch.empty((128, 128), device="cuda")),                # dtype
    ("gt", lambda: torch.empty((128, 129), device="cuda", dtype=E4M3)),   # shape
    ("g", lambda: torch.empty((128, 128), device="cuda", dtype=E4M3).T),  # stride
    ("gt", lambda: torch.empty((128, 128), dtype=E4M3)),                  # device
])
def test_bad_slabs_raise_before_launch(name, slab):
    with pytest.raises(RuntimeError, match=f"{name} must be a float8_e4m3fn"):
        ops.sigmoid_ids_e4m3(*_setup(*SHAPES[0])[0], **{name: slab()})
