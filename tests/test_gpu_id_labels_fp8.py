"""``ops.sigmoid_ids_fp8`` against float64 in kernel units: the e4m3 pair of
``ops.quantize_fp8_pair``, whose float64 dot is exact, ``t' = log(1.5 /
std(true dot)) + log si + log st`` (the per-tensor convention of
``test_gpu_tile_exact.py``), ``bias = −0.5``; ids, reference and scalar bound
of ``test_gpu_id_labels.py``.  ``(128, 128, 64)`` one tile, K half a 128-step;
``(256, 384, 208)`` several tiles, one step plus a tail of five chunks (one
unmasked row gets an id no text carries); ``(300, 333, 144)`` ragged, no
multiples of 4, a one-chunk tail.  Codes: the bound of
``test_gpu_id_labels_e4m3.py``."""

import functools
import math

import pytest
import torch

from distributed_sigmoid_loss_amd import ops
from test_gpu_id_labels import (BIAS, _Case, _check, _draw_ids, _reference,
                                _unit_rows)          # skips without a GPU
from test_gpu_id_labels_e4m3 import _ordinal

pytestmark = pytest.mark.gpu
E4M3, U8 = torch.float8_e4m3fn, torch.uint8
SHAPES = [(128, 128, 64), (256, 384, 208), (300, 333, 144)]
MODES = [("positive", None), ("ignore", 1), ("ignore", 400)]


@functools.lru_cache(maxsize=None)
def _setup(b, n, d, duplicates="positive", diag=None):
    gen = torch.Generator().manual_seed(b * 1000003 + n * 7919 + d)
    qc = ops.quantize_fp8_pair(_unit_rows(b, d, gen), _unit_rows(n, d, gen))
    s = qc.zi_q.float().double() @ qc.zt_q.float().double().T    # exact
    # log(1.5 / std(si·st·s)) + log si + log st
    tp = torch.tensor(math.log(1.5 / float(s.std())), device="cuda")
    bias = torch.tensor(BIAS, device="cuda")
    values = min(b, n) // 3
    img_ids, txt_ids = (_draw_ids(r, values, gen).cuda() for r in (b, n))
    if (b, n, d) == SHAPES[1]:
        img_ids[int((img_ids >= 0).nonzero()[0])] = 10 ** 6
    c = _Case(qc.zi_q, qc.zt_q, tp, bias, s, s * float(tp.double().exp()) + BIAS,
              img_ids, txt_ids)
    npos = _reference(c, img_ids, txt_ids).pos.sum(dim=1)
    assert bool((npos > 1).any()), "no row with several positives"
    assert bool(((npos == 0) & (img_ids >= 0)).any()), "no unmasked empty row"
    assert bool((img_ids < 0).any()) and bool((txt_ids < 0).any())
    args = (c.zi, c.zt, tp, bias, img_ids, txt_ids, duplicates, diag)
    return args, _reference(c, img_ids, txt_ids, duplicates, diag)


@pytest.mark.parametrize("b,n,d", SHAPES)
@pytest.mark.parametrize("duplicates,diag", MODES)
def test_codes_transpose_masks_and_partials(b, n, d, duplicates, diag):
    args, ref = _setup(b, n, d, duplicates, diag)
    partials, g, gt = ops.sigmoid_ids_fp8(*args)
    assert (g.dtype, g.shape, gt.shape) == (gt.dtype, (b, n), (n, b))
    codes = g.view(U8)
    want = (448.0 * ref.g).float().contiguous().to(E4M3).view(U8)
    diff = (_ordinal(codes) - _ordinal(want)).abs()
    print(f"ID_FP8 {b}x{n}x{d}-{duplicates}{diag} code_diff max="
          f"{int(diff.max())} share={float((diff != 0).double().mean()):.2e}")
    assert int(diff.max()) <= 1 and float((diff != 0).double().mean()) <= 1e-3
    assert torch.equal(gt.view(U8), codes.T)
    assert bool((codes[ref.masked] == 0).all()), "masked pair not 0x00"
    nz = (codes & 0x7F) != 0
    assert torch.equal(codes[nz] >= 128, ref.g[nz] < 0), "sign of a code"
    _check(None, partials, ref, f"fp8-{b}x{n}x{d}-{duplicates}{diag}")
    loss_only = ops.sigmoid_ids_fp8(*args, want_g=False)
    assert loss_only[1] is None and loss_only[2] is None
    assert torch.equal(loss_only[0], partials), "loss-only kernel's partials"
    assert torch.equal(ops.sigmoid_ids_fp8(*args, want_g=False)[0], partials)
    for x, y in zip(ops.sigmoid_ids_fp8(*args), (partials, g, gt)):
        assert torch.equal(x.view(U8), y.view(U8)), "run to run"


def test_views_into_wider_slabs_are_contained():
    (b, n, _), (args, _) = SHAPES[2], _setup(*SHAPES[2])   # byte-store path
    partials, g, gt = ops.sigmoid_ids_fp8(*args)
    wide = torch.full((b, n + 8), 0x7F, device="cuda", dtype=U8)
    wide_t = torch.full((n + 7, b + 3), 0x7F, device="cuda", dtype=U8)
    gv, gtv = wide[:, 3:3 + n], wide_t[5:5 + n, 1:1 + b]
    p2, _, _ = ops.sigmoid_ids_fp8(*args, g=gv.view(E4M3), gt=gtv.view(E4M3))
    assert torch.equal(p2, partials) and torch.equal(gv, g.view(U8))
    assert torch.equal(gtv, gt.view(U8))
    for buf, view in ((wide, gv), (wide_t, gtv)):
        view.fill_(0x7F)
        assert bool((buf == 0x7F).all()), "a byte outside the view changed"


def _slab(dtype=E4M3):
    return torch.empty((128, 128), device="cuda", dtype=dtype)


@pytest.mark.parametrize("match,edit", [
    ("float8_e4m3fn", lambda a, kw: a.__setitem__(0, a[0].to(torch.bfloat16))),
    ("multiple of 16", lambda a, kw: a.__setitem__(
        slice(0, 2), [x.view(U8)[:, :8].repeat(1, 9).view(E4M3) for x in a[:2]])),
    ("together", lambda a, kw: kw.update(g=_slab())),
    ("g must be a float8_e4m3fn",
     lambda a, kw: kw.update(g=_slab(torch.bfloat16), gt=_slab())),
])
def test_bad_inputs_raise_before_launch(match, edit):
    args, kw = list(_setup(*SHAPES[0])[0]), {}
    edit(args, kw)                      # the second case: d = 72
    with pytest.raises(RuntimeError, match=match):
        ops.sigmoid_ids_fp8(*args, **kw)
