"""``ops.sigmoid_ids_mx`` against float64 computed from the dequantised MX
operands ``q·2^(code − 127)``, whose float64 dot is exact; ``t' = log(1.5 /
std(s))``, ``bias = −0.5``; ids, reference, regime preconditions and scalar
bound of ``test_gpu_id_labels_fp8.py`` (every shape gives one unmasked row an
id no text carries), codes: the bound of ``test_gpu_id_labels_e4m3.py``.
``(17, 15)`` one ragged tile, ``(130, 257)`` and ``(300, 520)`` several with
ragged edges; ``d = 32`` a quarter K-step, ``160`` one step plus a one-block
tail, ``416`` three steps plus one.  Every (row, K-block) of the unit rows is
multiplied by ``2^k``, ``k`` drawn from ``−6 … 6``, before quantising; each
operand must carry at least 8 distinct scale bytes and some scale row two
different bytes (at ``d = 32`` the second is a pad byte)."""

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
BLOCKS = [(17, 15), (130, 257), (300, 520)]
DIMS = [32, 160, 416]
MODES = [("positive", None), ("ignore", 1)]


def _mx_operand(r, d, gen):
    k = (torch.randperm(r * (d // 32), generator=gen) % 13 - 6).view(r, -1, 1)
    x = _unit_rows(r, d, gen).view(r, d // 32, 32)
    q, e8 = ops.quantize_mx((x * torch.exp2(k.float()).bfloat16().cuda())
                            .reshape(r, d))
    real = e8[:, :d // 32]
    assert len(real.unique()) >= 8, "fewer than 8 distinct scale bytes"
    assert bool((e8 != e8[:, :1]).any()), "no row with two scale bytes"
    scale = torch.exp2(real.double() - 127).repeat_interleave(32, dim=1)
    return q, e8, q.float().double() * scale


@functools.lru_cache(maxsize=None)
def _setup(b, n, d, duplicates="positive", diag=None):
    gen = torch.Generator().manual_seed(b * 1000003 + n * 7919 + d)
    (zi_q, zi_e8, zi), (zt_q, zt_e8, zt) = (_mx_operand(r, d, gen)
                                            for r in (b, n))
    s = zi @ zt.T                                                # exact
    tp = torch.tensor(math.log(1.5 / float(s.std())), device="cuda")
    bias = torch.tensor(BIAS, device="cuda")
    values = min(b, n) // 3
    img_ids, txt_ids = (_draw_ids(r, values, gen).cuda() for r in (b, n))
    img_ids[int((img_ids >= 0).nonzero()[0])] = 10 ** 6
    c = _Case(zi_q, zt_q, tp, bias, s, s * float(tp.double().exp()) + BIAS,
              img_ids, txt_ids)
    npos = _reference(c, img_ids, txt_ids).pos.sum(dim=1)
    assert bool((npos > 1).any()), "no row with several positives"
    assert bool(((npos == 0) & (img_ids >= 0)).any()), "no unmasked empty row"
    assert bool((img_ids < 0).any()) and bool((txt_ids < 0).any())
    args = (zi_q, zi_e8, zt_q, zt_e8, tp, bias, img_ids, txt_ids, duplicates,
            diag)
    return args, _reference(c, img_ids, txt_ids, duplicates, diag)


@pytest.mark.parametrize("b,n", BLOCKS)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("duplicates,diag", MODES)
def test_codes_transpose_masks_and_partials(b, n, d, duplicates, diag):
    args, ref = _setup(b, n, d, duplicates, diag)
    partials, g, gt = ops.sigmoid_ids_mx(*args)
    assert (g.dtype, g.shape, gt.shape) == (gt.dtype, (b, n), (n, b))
    codes = g.view(U8)
    want = (448.0 * ref.g).float().contiguous().to(E4M3).view(U8)
    diff = (_ordinal(codes) - _ordinal(want)).abs()
    assert int(diff.max()) <= 1 and float((diff != 0).double().mean()) <= 1e-3
    assert torch.equal(gt.view(U8), codes.T)
    assert bool((codes[ref.masked] == 0).all()), "masked pair not 0x00"
    nz = (codes & 0x7F) != 0
    assert torch.equal(codes[nz] >= 128, ref.g[nz] < 0), "sign of a code"
    _check(None, partials, ref, f"mx-{b}x{n}x{d}-{duplicates}{diag}")
    lo = ops.sigmoid_ids_mx(*args, want_g=False)          # loss-only kernel
    assert lo[1] is None and lo[2] is None and torch.equal(lo[0], partials)
    for x, y in zip(ops.sigmoid_ids_mx(*args), (partials, g, gt)):
        assert torch.equal(x.view(U8), y.view(U8)), "run to run"


def test_views_into_wider_slabs_are_contained():
    (b, n), (args, _) = BLOCKS[2], _setup(*BLOCKS[2], DIMS[2])
    partials, g, gt = ops.sigmoid_ids_mx(*args)
    wide = torch.full((b, n + 9), 0x7F, device="cuda", dtype=U8)
    wide_t = torch.full((n + 7, b + 3), 0x7F, device="cuda", dtype=U8)
    gv, gtv = wide[:, 3:3 + n], wide_t[5:5 + n, 1:1 + b]   # byte-store path
    p2, _, _ = ops.sigmoid_ids_mx(*args, g=gv.view(E4M3), gt=gtv.view(E4M3))
    assert torch.equal(p2, partials) and torch.equal(gv, g.view(U8))
    assert torch.equal(gtv, gt.view(U8))
    for buf, view in ((wide, gv), (wide_t, gtv)):
        view.fill_(0x7F)
        assert bool((buf == 0x7F).all()), "a byte outside the view changed"


@pytest.mark.parametrize("d", DIMS)
def test_unit_scales_give_the_fp8_kernels_bits(d):
    args = list(_setup(*BLOCKS[1], d)[0])
    args[1], args[3] = (torch.full_like(e8, 0x7F) for e8 in (args[1], args[3]))
    fp8_args = [args[0], args[2], *args[4:]]
    for want_g in (True, False):
        got = ops.sigmoid_ids_mx(*args, want_g=want_g)[:1 + 2 * want_g]
        ref = ops.sigmoid_ids_fp8(*fp8_args, want_g=want_g)
        assert all(torch.equal(x.view(U8), y.view(U8)) for x, y in zip(got, ref))


@pytest.mark.parametrize("match,edit", [
    ("multiple of 32", lambda a: a.__setitem__(
        slice(0, 4), [a[0][:, :48].contiguous(), a[1][:, :4].contiguous(),
                      a[2][:, :48].contiguous(), a[3][:, :4].contiguous()])),
    ("ztxt_e8 must have shape", lambda a: a.__setitem__(3, a[3][:, :4].contiguous())),
    ("zimg_e8 must be a contiguous torch.uint8",
     lambda a: a.__setitem__(1, a[1].view(torch.int8))),
    ("ztxt_e8 must be 4-byte aligned", lambda a: a.__setitem__(    # a view
        3, torch.empty(a[3].numel() + 4, device="cuda", dtype=U8)[1:-3]
        .view(a[3].shape))),
])
def test_bad_inputs_raise_before_launch(match, edit):
    args = list(_setup(*BLOCKS[1], DIMS[1])[0])
    edit(args)
    with pytest.raises(RuntimeError, match=match):
        ops.sigmoid_ids_mx(*args)
