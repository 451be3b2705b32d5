"""Multi-tile checks of the persistent bf16 tile kernel and its epilogue.

The exact-test file never runs more than 15 tiles, so under the persistent
launch (one workgroup per CU, each walking several tiles) it exercises one
tile per workgroup only, and it places the diagonal at a few tile corners.
These cases force several tiles per workgroup with ``SIGLIP_TILE_WGS`` and
add, with the same float64 reference, checkers and bounds (imported, not
copied):

- multi-tile walks: 1, 3 and 8 workgroups over 16 / 10 / 10 tiles (uneven
  split, a workgroup with exactly one tile), d = 64 / 192 / 256 (one K-step;
  an odd count, so the double-buffer parity flips from tile to tile; an even
  count), all three modes, both input families;
- diagonal placement on a 4 x 4 tile grid: the block-uniform "can this tile
  hold a positive pair" test decides per tile whether the label predicate
  runs at all, so every way the diagonal can cross (or miss) a block row is
  a separate case;
- the g slab as a column view of a wider slab (``ldg > n`` with a column
  offset, as the ring strategy writes it);
- bit equality of the g slab across the default launch, every
  ``SIGLIP_TILE_WGS`` and ``SIGLIP_PERSISTENT=0`` (one tile per workgroup);
  of the scalars of two identical one-workgroup launches (fixed order); and
  of g between the LDS-staged writeback (exchanged MFMA operands, packed
  8-byte staging writes) and the general kernel's direct-store path
  (original operand order): exchanging the operands must not change a dot.

Bounds are those of ``test_gpu_tile_exact``: 1 bf16 ulp per g element, the
exact sign map, sentinel coverage and guard containment, scalars within
``1e-4 * sum|term|`` (sequential fp32 adds on the longest path: 128 per tile,
16 tiles per workgroup, 6 shuffle steps, 8 waves, 8 slots -- fewer than the
200 the bound was derived for; the one multiply of a tile's log2 sum by ln 2
adds a single rounding), and its >= 90 % informative-regime precondition,
asserted by ``_run`` for every case.
"""

import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from test_gpu_tile_exact import (  # noqa: E402
    FAMILIES, _Slabs, _launch, _operands, _reference, _run, _check_scalars,
    _check_slabs)

MODES = (0, 1, 2)
_ENV = ("SIGLIP_TILE_WGS", "SIGLIP_PERSISTENT")

# b x n: 16, 10 and 10 tiles.
_SHAPES = [(1024, 1024), (512, 1280), (1280, 512)]
_DIMS = (64, 192, 256)
_WGS = (1, 3, 8)
_MULTI = [pytest.param(b, n, d, fam, id=f"{fam}-{b}x{n}x{d}")
          for (b, n), d, fam in itertools.product(_SHAPES, _DIMS, FAMILIES)]
_baseline = {}


def _bits(slabs):
    return slabs.bits().clone()


def _default_bits(b, n, d, family, mode):
    """g slab (guards included) of the default launch, fully checked."""
    key = (b, n, d, family, mode)
    if key not in _baseline:
        with pytest.MonkeyPatch.context() as mp:
            for var in _ENV:
                mp.delenv(var, raising=False)
            _, slabs = _run("bf16", mode, family, b, n, d, 5)
        _baseline[key] = _bits(slabs)
    return _baseline[key]


@pytest.mark.parametrize("wgs", _WGS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("b,n,d,family", _MULTI)
def test_multi_tile(monkeypatch, b, n, d, family, mode, wgs):
    monkeypatch.delenv("SIGLIP_PERSISTENT", raising=False)
    monkeypatch.setenv("SIGLIP_TILE_WGS", str(wgs))
    _, slabs = _run("bf16", mode, family, b, n, d, 5)
    if mode:
        assert torch.equal(_bits(slabs), _default_bits(b, n, d, family, mode)), \
            f"g differs between SIGLIP_TILE_WGS={wgs} and the default launch"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("b,n,d,family", _MULTI)
def test_one_tile_per_workgroup(monkeypatch, b, n, d, family, mode):
    monkeypatch.delenv("SIGLIP_TILE_WGS", raising=False)
    monkeypatch.setenv("SIGLIP_PERSISTENT", "0")
    _, slabs = _run("bf16", mode, family, b, n, d, 5)
    if mode:
        assert torch.equal(_bits(slabs), _default_bits(b, n, d, family, mode)), \
            "g differs between SIGLIP_PERSISTENT=0 and the default launch"


# One workgroup adds its tiles in a fixed order: identical launches give
# identical scalars, bit for bit.
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("b,n,d,family", _MULTI[::3])
def test_one_workgroup_scalars_repeat(monkeypatch, b, n, d, family, mode):
    monkeypatch.setenv("SIGLIP_TILE_WGS", "1")
    op = _operands(family, "bf16", b, n, d)
    got = []
    for _ in range(2):
        slabs = _Slabs(b, n, False) if mode else None
        got.append(_launch(op, "bf16", mode, 5, slabs))
    assert torch.equal(got[0], got[1]), (got[0], got[1])

# 1024 x 1024 = 4 x 4 tiles.  0: the main diagonal, one tile per block row.
# 3, 259, -509: the diagonal crosses two tiles of a block row.  255 / 256 /
# -256: tile corners and exact tile shifts.  1023 / -1023: a single positive
# in a corner tile, every other block row has none.  1024 / None: none at all.
_DIAGS = (0, 3, 255, 256, -256, 259, -509, 1023, -1023, 1024, None)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k,diag", list(enumerate(_DIAGS)),
                         ids=[f"diag{d}" for d in _DIAGS])
def test_diagonal_placement(monkeypatch, k, diag, mode):
    monkeypatch.setenv("SIGLIP_TILE_WGS", "3")
    _run("bf16", mode, FAMILIES[k % 2], 1024, 1024, 64, diag)


# g written as slab[:, 256:256+n] of a wider sentinel-filled slab: nothing
# outside the view may change (checked by _check_slabs' guard test).  d = 192
# is an odd K-step count.
@pytest.mark.parametrize("mode", (1, 2))
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("b,n,d,diag", [(512, 1280, 64, 3),
                                        (1280, 512, 192, -259)])
def test_slab_view(monkeypatch, b, n, d, diag, family, mode):
    monkeypatch.setenv("SIGLIP_TILE_WGS", "3")
    _run("bf16", mode, family, b, n, d, diag, off=256, width=n + 512)


# The staged path (slab stride % 8 == 0: persistent kernel, exchanged MFMA
# operands) against the direct-store path (stride 2 mod 8: general kernel,
# original operand order).  Same dots in the same k order, so the same g bits.
@pytest.mark.parametrize("mode", (1, 2))
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("b,n,d", [(512, 768, 64), (768, 512, 192),
                                   (512, 512, 256)])
def test_staged_equals_direct(b, n, d, family, mode):
    diag = 5
    op = _operands(family, "bf16", b, n, d)
    ref = _reference(family, "bf16", b, n, d, diag)
    assert ref.informative >= 0.9
    got = {}
    for name, width in (("staged", n + 16), ("direct", n + 18)):
        slabs = _Slabs(b, n, False, off=8, width=width)
        scal = _launch(op, "bf16", mode, diag, slabs)
        tag = f"bf16-m{mode}-{family}-{b}x{n}x{d}-{name}"
        _check_scalars(scal, ref, mode, tag)
        _check_slabs(slabs, op, ref, "bf16", tag)
        got[name] = slabs.g.contiguous().view(torch.int16)
    assert torch.equal(got["staged"], got["direct"]), \
        "g differs between the staged and the direct-store path"
