"""The sample-ID sigmoid kernel (``ops.sigmoid_ids``) on its own, against
float64 computed from the same bf16 inputs with explicit ``(b, n)`` label and
mask matrices.

Shapes — the smallest at which each mechanism can fail: ``(1, 1, 8)``;
``(128, 128, 64)`` one full tile and one K-step; ``(129, 257, 72)`` ragged in
both directions plus a K tail; ``(1157, 130, 64)`` 10 tile-rows against the
block walk's locality group of 8 and 20 workgroups, not a multiple of the 8
XCDs.

Informative regime (the rule of ``test_gpu_tile_exact.py``): L2-normalised
Gaussian rows, ``t' = log(1.5 / std(s))`` and ``bias = −0.5``; ids uniform
over ``max(1, min(b, n) // 3)`` values with 10 % of each side set to ``−1``
(none at ``(1, 1, 8)``).  Every reference first asserts that at least 90 % of
``|g|`` over the unmasked pairs lies in ``[0.05, 0.95]`` and, at the three
larger shapes, that there is a row with several positives, an unmasked row
with none and a masked row and column.  At ``(129, 257, 72)`` every unmasked
row as drawn has a positive (129 rows against 257 columns over 43 values), so
that shape gives one unmasked row an id that no text carries.

Bounds (derived in ``test_gpu_tile_exact.py``): every g element within 1 bf16
ulp of the reference — 1/2 ulp is the rounding itself, the other half covers
v_exp_f32 / v_rcp_f32 and the fp32 dot product — and each of the three
scalars (per-tile partials summed in fp64) within ``1e-4·Σ|term_ref|``.  The
sign map is exact: ``g < 0`` precisely at positives, ``g > 0`` at negatives,
``g == 0`` at masked pairs; a mislabelled pair moves its element by about 1,
thousands of ulps.
"""

import functools
import math
from typing import NamedTuple, Optional

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from distributed_sigmoid_loss_amd import ops

DEV = "cuda"
SHAPES = [(1, 1, 8), (128, 128, 64), (129, 257, 72), (1157, 130, 64)]
LARGER = SHAPES[1:]
RAGGED = [(129, 257, 72), (1157, 130, 64)]
SENTINEL = 777.0
SCALAR_RTOL = 1e-4
BIAS = -0.5


class _Case(NamedTuple):
    zi: torch.Tensor          # bf16 (b, d)
    zt: torch.Tensor          # bf16 (n, d)
    tp: torch.Tensor          # fp32 0-d, on the device
    bias: torch.Tensor        # fp32 0-d, on the device
    s: torch.Tensor           # float64 (b, n) dots
    z: torch.Tensor           # float64 (b, n) logits
    img_ids: torch.Tensor     # int64 (b,)
    txt_ids: torch.Tensor     # int64 (n,)


class _Ref(NamedTuple):
    pos: torch.Tensor         # bool (b, n)
    masked: torch.Tensor      # bool (b, n)
    g: torch.Tensor           # float64 (b, n)
    sums: torch.Tensor        # float64 (3,): Σ term, Σ g·s, Σ g
    abs_sums: torch.Tensor    # float64 (3,): Σ |·| of the same


def _unit_rows(r, d, gen):
    x = torch.randn(r, d, generator=gen)
    return (x / x.norm(dim=1, keepdim=True)).to(DEV).bfloat16()


def _draw_ids(length, values, gen):
    ids = torch.randint(0, values, (length,), generator=gen)
    off = torch.randperm(length, generator=gen)[:length // 10]
    ids[off] = -1
    return ids


@functools.lru_cache(maxsize=None)
def _case(b, n, d) -> _Case:
    gen = torch.Generator().manual_seed(b * 1000003 + n * 7919 + d)
    zi, zt = _unit_rows(b, d, gen), _unit_rows(n, d, gen)
    s = zi.double() @ zt.double().T
    std = float(s.std()) if s.numel() > 1 else float(s.abs().max())
    tp = torch.tensor(math.log(1.5 / std), device=DEV, dtype=torch.float32)
    bias = torch.tensor(BIAS, device=DEV, dtype=torch.float32)
    values = max(1, min(b, n) // 3)
    img_ids = _draw_ids(b, values, gen)
    txt_ids = _draw_ids(n, values, gen)
    if (b, n, d) == (129, 257, 72):
        # an unmasked row whose id no text carries
        img_ids[int((img_ids >= 0).nonzero()[0])] = values
    z = s * float(tp.double().exp()) + BIAS
    return _Case(zi, zt, tp, bias, s, z, img_ids.to(DEV), txt_ids.to(DEV))


def _dense_classes(img_ids, txt_ids, duplicates, diag):
    """The contract, written out on (b, n) matrices."""
    b, n = img_ids.shape[0], txt_ids.shape[0]
    eq = img_ids[:, None] == txt_ids[None, :]
    masked = (img_ids[:, None] < 0) | (txt_ids[None, :] < 0)
    if duplicates == "positive":
        return eq & ~masked, masked
    i = torch.arange(b, device=DEV)[:, None]
    j = torch.arange(n, device=DEV)[None, :]
    on_diag = (j == i + diag) if diag is not None else torch.zeros_like(eq)
    masked = masked | (eq & ~on_diag)
    return on_diag & ~masked, masked


def _reference(c: _Case, img_ids, txt_ids, duplicates="positive",
               diag: Optional[int] = None) -> _Ref:
    pos, masked = _dense_classes(img_ids, txt_ids, duplicates, diag)
    lab = torch.where(pos, 1.0, -1.0).double()
    x = -lab * c.z
    term = torch.nn.functional.softplus(x, threshold=1e9)
    g = -lab * torch.sigmoid(x)
    term = term.masked_fill(masked, 0.0)
    g = g.masked_fill(masked, 0.0)
    parts = torch.stack([term, g * c.s, g])
    on = ~masked
    if bool(on.any()):
        a = g[on].abs()
        share = float(((a >= 0.05) & (a <= 0.95)).double().mean())
        assert share >= 0.9, f"uninformative regime: {share:.3f}"
    return _Ref(pos, masked, g, parts.sum(dim=(1, 2)),
                parts.abs().sum(dim=(1, 2)))


@functools.lru_cache(maxsize=None)
def _base_reference(b, n, d) -> _Ref:
    c = _case(b, n, d)
    ref = _reference(c, c.img_ids, c.txt_ids)
    if (b, n, d) in LARGER:
        row_on = c.img_ids >= 0
        npos = ref.pos.sum(dim=1)
        assert bool((npos > 1).any()), "no row with several positives"
        assert bool(((npos == 0) & row_on).any()), "no unmasked empty row"
        assert bool((~row_on).any()) and bool((c.txt_ids < 0).any())
    return ref


def _check(g, partials, ref: _Ref, tag):
    b, n = ref.g.shape
    assert partials.dtype == torch.float32
    assert partials.shape == (-(-b // 128) * -(-n // 128), 3)
    sums = partials.double().sum(dim=0)
    err = (sums - ref.sums).abs()
    bound = SCALAR_RTOL * ref.abs_sums
    line = (f"ID_LABELS {tag} scalar_err/bound="
            + " ".join(f"{float(e / max(float(t), 1e-300)):.4f}"
                       for e, t in zip(err, bound)))
    if g is not None:
        assert g.dtype == torch.bfloat16 and g.shape == (b, n)
        got = g.double()
        ulp = torch.exp2(torch.floor(torch.log2(ref.g.abs())) - 7)
        off = (got - ref.g).abs()
        worst = float((off / ulp.clamp_min(1e-300))[~ref.masked].max()) \
            if bool((~ref.masked).any()) else 0.0
        line += f" g_ulp={worst:.4f}"
    print(line)
    if g is not None:
        assert bool((off <= ulp).all()), f"{tag}: g off by {worst:.3f} ulp"
        # the sign map, exactly
        assert torch.equal(got < 0, ref.pos), f"{tag}: positives"
        assert torch.equal(got == 0, ref.masked), f"{tag}: masked"
        assert torch.equal(got > 0, ~ref.pos & ~ref.masked), f"{tag}: neg"
    assert bool((err <= bound).all()), (tag, err.tolist(), bound.tolist())


@pytest.mark.parametrize("b,n,d", SHAPES)
def test_positive_mode_elements_scalars_and_instantiations(b, n, d):
    c, ref = _case(b, n, d), _base_reference(b, n, d)
    partials, g = ops.sigmoid_ids(c.zi, c.zt, c.tp, c.bias, c.img_ids,
                                  c.txt_ids)
    _check(g, partials, ref, f"{b}x{n}x{d}")
    # the loss-only instantiation: no g, the same bits
    p0, none = ops.sigmoid_ids(c.zi, c.zt, c.tp, c.bias, c.img_ids,
                               c.txt_ids, want_g=False)
    assert none is None
    assert torch.equal(p0, partials)
    # and both are reproducible
    p2, g2 = ops.sigmoid_ids(c.zi, c.zt, c.tp, c.bias, c.img_ids, c.txt_ids)
    assert torch.equal(p2, partials) and torch.equal(g2, g)
    p3, _ = ops.sigmoid_ids(c.zi, c.zt, c.tp, c.bias, c.img_ids, c.txt_ids,
                            want_g=False)
    assert torch.equal(p3, p0)


@pytest.mark.parametrize("b,n,d", LARGER)
def test_ids_are_compared_as_64_bit(b, n, d):
    c, ref = _case(b, n, d), _base_reference(b, n, d)
    base_p, base_g = ops.sigmoid_ids(c.zi, c.zt, c.tp, c.bias, c.img_ids,
                                     c.txt_ids)
    # 2^40 on every real id: the same classes, so the same bits
    hi = 1 << 40
    img_hi = torch.where(c.img_ids >= 0, c.img_ids + hi, c.img_ids)
    txt_hi = torch.where(c.txt_ids >= 0, c.txt_ids + hi, c.txt_ids)
    p, g = ops.sigmoid_ids(c.zi, c.zt, c.tp, c.bias, img_hi, txt_hi)
    _check(g, p, ref, f"{b}x{n}x{d}+2^40")
    assert torch.equal(g, base_g) and torch.equal(p, base_p)
    # 2^32 on the image side of every other row: equal low words, different
    # samples — those rows' positives become negatives
    odd = (torch.arange(b, device=DEV) % 2 == 1) & (c.img_ids >= 0)
    img_split = torch.where(odd, c.img_ids + (1 << 32), c.img_ids)
    ref2 = _reference(c, img_split, c.txt_ids)
    lost = ref.pos & ~ref2.pos
    assert bool(lost.any()) and bool((ref.pos & ref2.pos).any())
    assert not bool((lost & ref2.masked).any())
    p, g = ops.sigmoid_ids(c.zi, c.zt, c.tp, c.bias, img_split, c.txt_ids)
    _check(g, p, ref2, f"{b}x{n}x{d}+2^32")


@pytest.mark.parametrize("b,n,d", SHAPES)
@pytest.mark.parametrize("diag", [0, 5, -3, None])
def test_ignore_mode(b, n, d, diag):
    c = _case(b, n, d)
    ref = _reference(c, c.img_ids, c.txt_ids, "ignore", diag)
    if (b, n, d) in LARGER:
        eq = c.img_ids[:, None] == c.txt_ids[None, :]
        real = (c.img_ids[:, None] >= 0) & (c.txt_ids[None, :] >= 0)
        i = torch.arange(b, device=DEV)[:, None]
        j = torch.arange(n, device=DEV)[None, :]
        # equal ids off the diagonal are switched off ...
        off_diag = eq & real & ~ref.pos
        assert bool(off_diag.any()) and bool(ref.masked[off_diag].all())
        if diag is not None:
            on_diag = j == i + diag
            # ... a diagonal pair is positive whatever its ids, unless an id
            # is negative
            assert bool((ref.pos & ~eq).any()), "no unequal-id diagonal pair"
            assert bool((on_diag & ~real).any()), "no masked diagonal pair"
            assert torch.equal(ref.pos, on_diag & real)
        else:
            assert not bool(ref.pos.any())
    partials, g = ops.sigmoid_ids(c.zi, c.zt, c.tp, c.bias, c.img_ids,
                                  c.txt_ids, duplicates="ignore",
                                  diag_offset=diag)
    _check(g, partials, ref, f"{b}x{n}x{d}-ignore-diag{diag}")
    p0, none = ops.sigmoid_ids(c.zi, c.zt, c.tp, c.bias, c.img_ids,
                               c.txt_ids, duplicates="ignore",
                               diag_offset=diag, want_g=False)
    assert none is None and torch.equal(p0, partials)


def test_positive_mode_ignores_diag_offset():
    b, n, d = RAGGED[0]
    c = _case(b, n, d)
    p, g = ops.sigmoid_ids(c.zi, c.zt, c.tp, c.bias, c.img_ids, c.txt_ids)
    p2, g2 = ops.sigmoid_ids(c.zi, c.zt, c.tp, c.bias, c.img_ids, c.txt_ids,
                             diag_offset=3)
    assert torch.equal(p, p2) and torch.equal(g, g2)


def test_out_of_int32_diag_offset_means_none():
    b, n, d = RAGGED[0]
    c = _case(b, n, d)
    want = ops.sigmoid_ids(c.zi, c.zt, c.tp, c.bias, c.img_ids, c.txt_ids,
                           duplicates="ignore", diag_offset=None)
    for diag in (2 ** 31, -(2 ** 31), 2 ** 40):
        got = ops.sigmoid_ids(c.zi, c.zt, c.tp, c.bias, c.img_ids, c.txt_ids,
                              duplicates="ignore", diag_offset=diag)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("b,n,d", RAGGED)
@pytest.mark.parametrize("duplicates", ["positive", "ignore"])
def test_g_band_in_a_wider_slab_stays_inside(b, n, d, duplicates):
    """g as a column band at an odd column offset inside a sentinel-filled
    slab with an odd row stride: no sentinel left inside, no guard changed."""
    c0, diag = 3, 1
    c = _case(b, n, d)
    ref = (_base_reference(b, n, d) if duplicates == "positive"
           else _reference(c, c.img_ids, c.txt_ids, "ignore", diag))
    width = c0 + n + 5
    width += 1 - width % 2
    slab = torch.full((b + 2, width), SENTINEL, device=DEV,
                      dtype=torch.bfloat16)
    view = slab[1:b + 1, c0:c0 + n]
    assert view.stride(0) % 2 == 1
    partials, g = ops.sigmoid_ids(c.zi, c.zt, c.tp, c.bias, c.img_ids,
                                  c.txt_ids, duplicates=duplicates,
                                  diag_offset=diag, g=view)
    assert g.data_ptr() == view.data_ptr()
    _check(view, partials, ref, f"{b}x{n}x{d}-{duplicates}-band")
    assert not bool((view == SENTINEL).any())
    outside = torch.ones_like(slab, dtype=torch.bool)
    outside[1:b + 1, c0:c0 + n] = False
    assert torch.equal(slab[outside],
                       torch.full_like(slab[outside], SENTINEL))
    p_dense, dense = ops.sigmoid_ids(c.zi, c.zt, c.tp, c.bias, c.img_ids,
                                     c.txt_ids, duplicates=duplicates,
                                     diag_offset=diag)
    assert torch.equal(view, dense) and torch.equal(partials, p_dense)


def test_all_masked_block_is_exactly_zero():
    b, n, d = RAGGED[0]
    c = _case(b, n, d)
    off = torch.full_like(c.img_ids, -1)
    partials, g = ops.sigmoid_ids(c.zi, c.zt, c.tp, c.bias, off, c.txt_ids)
    assert float(partials.abs().max()) == 0.0
    assert float(g.float().abs().max()) == 0.0


def test_bad_inputs_raise():
    c = _case(*SHAPES[1])
    args = (c.zi, c.zt, c.tp, c.bias)
    with pytest.raises(RuntimeError, match="img_ids"):
        ops.sigmoid_ids(*args, c.img_ids.int(), c.txt_ids)
    with pytest.raises(RuntimeError, match="txt_ids"):
        ops.sigmoid_ids(*args, c.img_ids, c.txt_ids[:-1])
    with pytest.raises(RuntimeError, match="txt_ids"):
        ops.sigmoid_ids(*args, c.img_ids,
                        torch.cat([c.txt_ids, c.txt_ids])[::2])
    with pytest.raises(RuntimeError, match="img_ids"):
        ops.sigmoid_ids(*args, c.img_ids.cpu(), c.txt_ids)
    with pytest.raises(RuntimeError, match="bf16"):
        ops.sigmoid_ids(c.zi.float(), c.zt, c.tp, c.bias, c.img_ids,
                        c.txt_ids)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.sigmoid_ids(c.zi[:, :4].contiguous(), c.zt[:, :4].contiguous(),
                        c.tp, c.bias, c.img_ids, c.txt_ids)
    with pytest.raises(RuntimeError, match="g must be"):
        ops.sigmoid_ids(*args, c.img_ids, c.txt_ids,
                        g=torch.empty((128, 64), device=DEV,
                                      dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="duplicates"):
        ops.sigmoid_ids(*args, c.img_ids, c.txt_ids, duplicates="keep")
