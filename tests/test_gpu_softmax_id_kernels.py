"""The sample-ID softmax kernels, each on its own, against float64 computed
from the same bf16 inputs: ``ops.pair_lse_ids`` (masked LSE, positive-logit
sums and positive counts) and ``ops.softmax_g_ids`` (dL/dlogit slab + per-tile
``Σ g·s``).

Shapes — those of ``test_gpu_softmax_kernels.py``, the smallest at which each
mechanism can fail: ``(1, 1, 8)``; ``(128, 128, 64)`` one full tile and one
K-step; ``(129, 257, 72)`` ragged in both directions, a K tail and the
positives of one row in different column tiles; ``(1157, 130, 64)`` 10
tile-rows against the block walk's locality group of 8 and 20 workgroups, not
a multiple of the 8 XCDs.

Inputs: L2-normalised Gaussian rows in bf16 and ``t' = log(1.5 / std(s))``
(the informative-regime rule); ids uniform over ``ceil(max(b, n) / 3)``
values, about 1 in 32 of each side set to −1 (at least one on a side of 32 or
more), then one unmasked row and one unmasked column given an id nobody else
has.  Every case first asserts on the float64 reference that at least 90 % of
the unmasked rows and columns have a largest masked-softmax probability below
0.9 — a wrongly masked, dropped or doubled element then moves an LSE by about
``1/n``, far outside the bound — and that the batch holds what the kernel
must tell apart: a masked row and a masked column; where the ids decide
(``"positive"``), a row and a column with two or more positives and an
unmasked row and column with none (the unique ids); where the position
decides (``"ignore"``), a pair with equal ids off the diagonal that must
count for nothing.  (At ``(1, 1, 8)`` only what exists is checked.)

Bounds (derived, not measured).  With ``ε_dot = t·d·2⁻²³·max_ij Σ_k |a_ik
b_jk|`` — the fp32 accumulation of d exact bf16 products and the scale by t,
with a factor 2 of slack — and max / min over the unmasked elements:

    |Δlse| ≤ ε = ε_dot + 2⁻²⁰·(1 + max z − min z)

as derived in ``test_gpu_softmax_kernels.py``; a fully masked row or column
is exactly −inf.  Counts are exact.  Positive sums:

    |Δpos| ≤ cnt·ε_dot + cnt·2⁻²³·Σ_p |z_p|

the dot error of each term plus the fp32 summation of ``cnt`` terms (at most
``cnt`` roundings at 2⁻²⁴ of a partial sum bounded by ``Σ|z_p|``, the scale by
t included), with a factor 2 of slack.  g:

    |Δg| ≤ 1 bf16 ulp of g_ref + (row_w_i + col_w_j)·ε_dot
           + (row_pw_i + col_pw_j)·2⁻²³

the rounding of the stored value, the two exponentials — each moves by at
most ``Δz`` relative — and the fp32 roundings of the subtrahend and of the
difference.  The LSEs and weights the kernel reads are float64 ones rounded to
fp32 and the reference uses those same rounded values, so the g test does not
depend on the LSE kernel.  Masked elements are exactly 0.  Per-tile scalars,
summed: ``1e-4·Σ|g·s|``, the project's scalar bound, plus the fp32 resolution
of the positive pairs derived in ``test_gpu_softmax_kernels.py`` with the
positive weights in place of the side weights:
``(row_pw + col_pw)·(6 + 2|z|)·2⁻²⁴·|s|`` per positive pair.
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
RAGGED = [(129, 257, 72), (1157, 130, 64)]
# duplicates, diag_offset ("n": every positional positive outside the block)
MODES = [("positive", None), ("ignore", 0), ("ignore", -3), ("ignore", 5),
         ("ignore", "n")]
SENTINEL = 777.0
INF = math.inf


class _Case(NamedTuple):
    zi: torch.Tensor          # bf16 (b, d)
    zt: torch.Tensor          # bf16 (n, d)
    tp: torch.Tensor          # fp32 0-d, on the device
    t: float
    s: torch.Tensor           # float64 (b, n) dots
    z: torch.Tensor           # float64 (b, n) logits
    eps_dot: float
    iid: torch.Tensor         # int64 (b,)
    tid: torch.Tensor         # int64 (n,)


class _Ref(NamedTuple):
    dup: str
    diag: Optional[int]
    pos: torch.Tensor         # bool (b, n), unmasked positives
    masked: torch.Tensor      # bool (b, n)
    row_lse: torch.Tensor     # float64, −inf for a fully masked row
    row_pos: torch.Tensor
    row_cnt: torch.Tensor     # int64
    row_abs: torch.Tensor     # Σ_p |z_p|
    col_lse: torch.Tensor
    col_pos: torch.Tensor
    col_cnt: torch.Tensor
    col_abs: torch.Tensor
    eps: float                # the LSE bound


def _classes(iid, tid, dup, diag):
    b, n = iid.shape[0], tid.shape[0]
    eq = iid[:, None] == tid[None, :]
    masked = (iid < 0)[:, None] | (tid < 0)[None, :]
    if dup == "positive":
        pos = eq
    else:
        pos = torch.zeros((b, n), dtype=torch.bool, device=iid.device)
        if diag is not None:
            pos = (torch.arange(n, device=iid.device)[None, :]
                   == torch.arange(b, device=iid.device)[:, None] + diag)
        masked = masked | (eq & ~pos)
    return pos & ~masked, masked


def _case(zi, zt, tp, iid, tid) -> _Case:
    a, bm = zi.double(), zt.double()
    s = a @ bm.T
    t = float(tp.double().exp())
    absdot = float((a.abs() @ bm.abs().T).max())
    return _Case(zi, zt, tp, t, s, s * t,
                 t * zi.shape[1] * 2.0 ** -23 * absdot, iid.to(DEV),
                 tid.to(DEV))


def _ref(c: _Case, dup, diag, iid=None, tid=None) -> _Ref:
    iid = c.iid if iid is None else iid
    tid = c.tid if tid is None else tid
    pos, masked = _classes(iid, tid, dup, diag)
    zm = c.z.masked_fill(masked, -INF)
    zp = torch.where(pos, c.z, torch.zeros_like(c.z))
    span = 0.0
    if not bool(masked.all()):
        live = c.z[~masked]
        span = float(live.max()) - float(live.min())
    return _Ref(dup, diag, pos, masked,
                torch.logsumexp(zm, 1), zp.sum(1), pos.sum(1), zp.abs().sum(1),
                torch.logsumexp(zm, 0), zp.sum(0), pos.sum(0), zp.abs().sum(0),
                c.eps_dot + 2.0 ** -20 * (1.0 + span))


def _unit_rows(r, d, gen):
    x = torch.randn(r, d, generator=gen)
    return (x / x.norm(dim=1, keepdim=True)).to(DEV).bfloat16()


def _make_ids(b, n, gen):
    k = -(-max(b, n) // 3)
    out = []
    for m, unique in ((b, k + 1), (n, k + 2)):
        ids = torch.randint(0, k, (m,), generator=gen)
        if m >= 32:
            off = torch.rand(m, generator=gen) < 1.0 / 32
            if not bool(off.any()):
                off[int(torch.randint(0, m, (1,), generator=gen))] = True
            ids[off] = -1
            # one unmasked entry with an id nobody else has
            ids[int((~off).nonzero()[0])] = unique
        out.append(ids)
    return out


@functools.lru_cache(maxsize=None)
def _informative(b, n, d) -> _Case:
    gen = torch.Generator().manual_seed(b * 1000003 + n * 7919 + d)
    zi, zt = _unit_rows(b, d, gen), _unit_rows(n, d, gen)
    s = zi.double() @ zt.double().T
    std = float(s.std()) if s.numel() > 1 else float(s.abs().max())
    tp = torch.tensor(math.log(1.5 / std), device=DEV, dtype=torch.float32)
    return _case(zi, zt, tp, *_make_ids(b, n, gen))


def _diag(n, diag):
    return n if diag == "n" else diag


@functools.lru_cache(maxsize=None)
def _reference(b, n, d, dup, diag) -> _Ref:
    """The float64 reference of a test shape, with the preconditions."""
    c = _informative(b, n, d)
    r = _ref(c, dup, diag)
    live_r, live_c = ~r.masked.all(1), ~r.masked.all(0)
    zm = c.z.masked_fill(r.masked, -INF)
    if n > 1:
        p = torch.exp(zm.max(1).values - r.row_lse)[live_r]
        assert float((p < 0.9).double().mean()) >= 0.9, "uninformative rows"
    if b > 1:
        p = torch.exp(zm.max(0).values - r.col_lse)[live_c]
        assert float((p < 0.9).double().mean()) >= 0.9, "uninformative cols"
    if min(b, n) >= 32:
        assert bool((~live_r).any()) and bool((~live_c).any()), "no mask"
        if dup == "positive":
            # the ids decide: the unique ids give the rows without a positive
            assert bool((live_r & (r.row_cnt == 0)).any()), "no empty row"
            assert bool((live_c & (r.col_cnt == 0)).any()), "no empty column"
            assert int(r.row_cnt.max()) >= 2 and int(r.col_cnt.max()) >= 2
        else:
            # the position decides: at most one positive, and a pair with
            # equal ids off the diagonal that must count for nothing
            assert int(r.row_cnt.max()) <= 1 and int(r.col_cnt.max()) <= 1
            eq = c.iid[:, None] == c.tid[None, :]
            assert bool((eq & ~r.pos & (c.iid >= 0)[:, None]).any()), \
                "no ignored duplicate"
        if dup == "positive" and n > 128:
            tiles = torch.stack([r.pos[:, j:j + 128].any(1)
                                 for j in range(0, n, 128)]).sum(0)
            assert int(tiles.max()) >= 2, "no row with positives in 2 tiles"
    return r


# ---------------------------------------------------------------------------
# LSE, positive sums and counts
# ---------------------------------------------------------------------------

def _assert_lse(got, ref, eps):
    assert not bool(torch.isnan(got).any())
    dead = torch.isinf(ref)
    assert torch.equal(got[dead], ref[dead].float())      # exactly −inf
    err = (got.double() - ref)[~dead].abs()
    worst = float(err.max()) if err.numel() else 0.0
    assert worst <= eps, (worst, eps)
    return worst / eps


def _assert_pos(got, ref, cnt, zabs, eps_dot):
    assert not bool(torch.isnan(got).any())
    tol = cnt.double() * eps_dot + cnt.double() * 2.0 ** -23 * zabs
    err = (got.double() - ref).abs()
    assert bool((err <= tol).all()), float((err - tol).max())
    return float((err / tol.clamp_min(1e-300)).max())


def _check_lse(c: _Case, r: _Ref, tag, iid=None, tid=None):
    out = ops.pair_lse_ids(c.zi, c.zt, c.tp, c.iid if iid is None else iid,
                           c.tid if tid is None else tid, r.dup, r.diag)
    b, n = c.s.shape
    for v, m in ((out.row_lse, b), (out.row_pos, b), (out.col_lse, n),
                 (out.col_pos, n)):
        assert v.dtype == torch.float32 and v.shape == (m,)
    for v, m in ((out.row_cnt, b), (out.col_cnt, n)):
        assert v.dtype == torch.int32 and v.shape == (m,)
    assert torch.equal(out.row_cnt.long(), r.row_cnt)
    assert torch.equal(out.col_cnt.long(), r.col_cnt)
    fr = _assert_lse(out.row_lse, r.row_lse, r.eps)
    fc = _assert_lse(out.col_lse, r.col_lse, r.eps)
    pr = _assert_pos(out.row_pos, r.row_pos, r.row_cnt, r.row_abs, c.eps_dot)
    pc = _assert_pos(out.col_pos, r.col_pos, r.col_cnt, r.col_abs, c.eps_dot)
    print(f"SOFTMAX_ID_LSE {tag} eps={r.eps:.3e} row_err/eps={fr:.4f} "
          f"col_err/eps={fc:.4f} row_pos_err/bound={pr:.4f} "
          f"col_pos_err/bound={pc:.4f}")
    return out


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y)
               for x, y in zip(a, b))


@pytest.mark.parametrize("b,n,d", SHAPES)
@pytest.mark.parametrize("dup,diag", MODES)
def test_lse_informative(b, n, d, dup, diag):
    diag = _diag(n, diag)
    c, r = _informative(b, n, d), _reference(b, n, d, dup, diag)
    out = _check_lse(c, r, f"{b}x{n}x{d}-{dup}-{diag}")
    args = (c.zi, c.zt, c.tp, c.iid, c.tid, dup, diag)
    # run to run, and one side at a time: the same bits, the other side None
    assert _same(ops.pair_lse_ids(*args), out)
    r_only = ops.pair_lse_ids(*args, cols=False)
    assert r_only[3:] == (None,) * 3 and _same(r_only[:3], out[:3])
    c_only = ops.pair_lse_ids(*args, rows=False)
    assert c_only[:3] == (None,) * 3 and _same(c_only[3:], out[3:])
    assert tuple(ops.pair_lse_ids(*args, rows=False, cols=False)) == (
        None,) * 6


@pytest.mark.parametrize("b,n,d", SHAPES[1:])
def test_lse_ids_are_64_bit(b, n, d):
    c, r = _informative(b, n, d), _reference(b, n, d, "positive", None)
    base = ops.pair_lse_ids(c.zi, c.zt, c.tp, c.iid, c.tid)
    hi = 2 ** 40
    iid = torch.where(c.iid >= 0, c.iid + hi, c.iid)
    tid = torch.where(c.tid >= 0, c.tid + hi, c.tid)
    assert _same(ops.pair_lse_ids(c.zi, c.zt, c.tp, iid, tid), base)
    # +2³² on every other row: equal in the low word only
    half = (torch.arange(b, device=DEV) % 2 == 0) & (c.iid >= 0)
    iid2 = torch.where(half, iid + 2 ** 32, iid)
    r2 = _ref(c, "positive", None, iid2, tid)
    assert not torch.equal(r2.pos, r.pos)
    assert not torch.equal(r2.row_cnt, r.row_cnt)
    _check_lse(c, r2, f"{b}x{n}x{d}-hi-word", iid2, tid)


def _range_case(kind):
    b, n, d = RAGGED[0]
    gen = torch.Generator().manual_seed(3 if kind == "overflow" else 4)
    if kind == "overflow":
        # a quarter of the text rows equal their image rows and t = 100: z
        # reaches 100 and exp overflows fp32 unless the max is subtracted
        zi, zt = _unit_rows(b, d, gen), _unit_rows(n, d, gen)
        idx = torch.arange(0, b, 4, device=DEV)
        zt[idx] = zi[idx]
    else:
        # zimg_i = v, ztxt_j = −v: every z is −100·|v|²; a padding element
        # (z = 0) leaking into a ragged tile would dominate
        v = _unit_rows(1, d, gen)
        zi, zt = v.expand(b, d).contiguous(), (-v).expand(n, d).contiguous()
    tp = torch.tensor(math.log(100.0), device=DEV, dtype=torch.float32)
    return _case(zi, zt, tp, *_make_ids(b, n, gen))


@pytest.mark.parametrize("dup,diag", [("positive", None), ("ignore", 0)])
def test_lse_overflow_range(dup, diag):
    c = _range_case("overflow")
    assert float(c.z.max()) > 95.0
    _check_lse(c, _ref(c, dup, diag), f"overflow-{dup}")


@pytest.mark.parametrize("dup,diag", [("positive", None), ("ignore", 0)])
def test_lse_negative_logits_padding_does_not_leak(dup, diag):
    c = _range_case("negative")
    z0 = float(c.z[0, 0])
    assert -101.0 < z0 < -99.0
    r = _ref(c, dup, diag)
    out = _check_lse(c, r, f"negative-{dup}")
    i = int((c.iid >= 0).nonzero()[0])
    live = int((~r.masked[i]).sum())
    assert abs(float(out.row_lse[i]) - (z0 + math.log(live))) < 1e-3


@pytest.mark.parametrize("dup,diag", [("positive", None), ("ignore", 5)])
def test_lse_column_chunks(dup, diag):
    """n = 257 in chunks of 100, off the tile grid: counts exact, positive
    sums and the folded row LSE within the bounds, the column outputs the
    same bits as the unchunked call's."""
    b, n, d = RAGGED[0]
    c, r = _informative(b, n, d), _reference(b, n, d, dup, diag)
    whole = ops.pair_lse_ids(c.zi, c.zt, c.tp, c.iid, c.tid, dup, diag)
    row_lse = row_pos = row_cnt = None
    cols = []
    for j0 in range(0, n, 100):
        j1 = min(j0 + 100, n)
        o = ops.pair_lse_ids(c.zi, c.zt[j0:j1], c.tp, c.iid, c.tid[j0:j1],
                             dup, None if diag is None else diag - j0)
        if row_lse is None:
            row_lse, row_pos, row_cnt = o.row_lse, o.row_pos, o.row_cnt
        else:
            row_lse = torch.logaddexp(row_lse, o.row_lse)
            row_pos, row_cnt = row_pos + o.row_pos, row_cnt + o.row_cnt
        cols.append(o[3:])
    assert torch.equal(row_cnt.long(), r.row_cnt)
    _assert_lse(row_lse, r.row_lse, r.eps)
    _assert_pos(row_pos, r.row_pos, r.row_cnt, r.row_abs, c.eps_dot)
    for k in range(3):
        assert torch.equal(torch.cat([p[k] for p in cols]), whole[3 + k])


# ---------------------------------------------------------------------------
# g kernel
# ---------------------------------------------------------------------------

class _GRef(NamedTuple):
    row: tuple                # fp32 (lse, w, pw): what the kernel reads
    col: tuple
    g: torch.Tensor           # float64 (b, n)
    tol: torch.Tensor         # float64 (b, n) element bound
    gs: float                 # Σ g·s
    gs_abs: float             # Σ |g·s|
    gs_tol: float             # the scalar bound


def _g_ref(c: _Case, r: _Ref, rows=True, cols=True, seed=0) -> _GRef:
    b, n = c.s.shape
    gen = torch.Generator().manual_seed(b + 31 * n + seed)

    def side(m, lse, cnt):
        w = (0.5 + torch.rand(m, generator=gen)).to(DEV)
        w = torch.where(cnt > 0, w, torch.zeros_like(w))
        return lse.float(), w, w / cnt.clamp(min=1).float()

    row = side(b, r.row_lse, r.row_cnt)
    col = side(n, r.col_lse, r.col_cnt)
    g = torch.zeros_like(c.z)
    w = torch.zeros_like(c.z)
    pw = torch.zeros_like(c.z)
    if rows:
        g += row[1].double()[:, None] * torch.exp(
            c.z - row[0].double()[:, None])
        w += row[1].double()[:, None]
        pw += row[2].double()[:, None]
    if cols:
        g += col[1].double()[None, :] * torch.exp(
            c.z - col[0].double()[None, :])
        w += col[1].double()[None, :]
        pw += col[2].double()[None, :]
    g -= pw * r.pos
    g = torch.where(r.masked, torch.zeros_like(g), g)     # 0·inf → 0
    ulp = torch.exp2(torch.floor(torch.log2(g.abs())) - 7)
    gs_abs = float((g * c.s).abs().sum())
    cancel = float((pw * (6.0 + 2.0 * c.z.abs()) * 2.0 ** -24
                    * c.s.abs())[r.pos].sum())
    return _GRef(row, col, g, ulp + w * c.eps_dot + pw * 2.0 ** -23,
                 float((g * c.s).sum()), gs_abs, 1e-4 * gs_abs + cancel)


@functools.lru_cache(maxsize=None)
def _g_reference(b, n, d, dup, diag, rows=True, cols=True) -> _GRef:
    return _g_ref(_informative(b, n, d), _reference(b, n, d, dup, diag),
                  rows, cols)


def _run_g(c: _Case, r: _Ref, row, col, **kw):
    return ops.softmax_g_ids(c.zi, c.zt, c.tp, c.iid, c.tid, r.dup, r.diag,
                             *row, *col, **kw)


def _check_g(got, gs, r: _Ref, ref: _GRef, tag):
    got = got.double()
    assert not bool(torch.isnan(got).any())
    assert float(got[r.masked].abs().max() if bool(r.masked.any())
                 else 0.0) == 0.0
    err = (got - ref.g).abs()
    worst = float((err / ref.tol.clamp_min(1e-300)).max())
    gs_err = abs(float(gs.double().sum()) - ref.gs)
    print(f"SOFTMAX_ID_G {tag} err/bound={worst:.4f} "
          f"gs_err/bound={gs_err / max(ref.gs_tol, 1e-300):.4f} "
          f"gs_rel={gs_err / max(ref.gs_abs, 1e-300):.3e}")
    assert bool((err <= ref.tol).all()), worst
    # A positive's sign wherever the reference is resolved.  With one
    # positive per row and column it is negative; among several, one that
    # holds more than its 1/cnt share of the softmax mass is pushed away, so
    # the sign to meet is the reference's own.
    sure = r.pos & (ref.g.abs() > ref.tol)
    assert torch.equal(got[sure] < 0, ref.g[sure] < 0)
    if int(r.row_cnt.max()) <= 1 and int(r.col_cnt.max()) <= 1:
        assert bool((got[sure] < 0).all())
    assert gs_err <= ref.gs_tol, (gs_err, ref.gs_tol, ref.gs_abs)


NONE3 = (None, None, None)


@pytest.mark.parametrize("b,n,d", SHAPES)
@pytest.mark.parametrize("dup,diag", MODES)
def test_g_elements_and_scalar(b, n, d, dup, diag):
    diag = _diag(n, diag)
    c, r = _informative(b, n, d), _reference(b, n, d, dup, diag)
    ref = _g_reference(b, n, d, dup, diag)
    g, gs = _run_g(c, r, ref.row, ref.col)
    assert g.dtype == torch.bfloat16 and g.shape == (b, n)
    assert gs.dtype == torch.float32
    assert gs.numel() == -(-b // 128) * -(-n // 128)
    _check_g(g, gs, r, ref, f"{b}x{n}x{d}-{dup}-{diag}")
    g2, gs2 = _run_g(c, r, ref.row, ref.col)
    assert torch.equal(g, g2) and torch.equal(gs, gs2)


@pytest.mark.parametrize("b,n,d", SHAPES)
@pytest.mark.parametrize("dup,diag", [("positive", None), ("ignore", 2)])
@pytest.mark.parametrize("side", ["rows", "cols"])
def test_g_side_omission(b, n, d, dup, diag, side):
    c, r = _informative(b, n, d), _reference(b, n, d, dup, diag)
    rows = side == "rows"
    ref = _g_reference(b, n, d, dup, diag, rows=rows, cols=not rows)

    def zeroed(v):
        return (v[0], torch.zeros_like(v[1]), torch.zeros_like(v[2]))

    if rows:
        one = _run_g(c, r, ref.row, NONE3)
        two = _run_g(c, r, ref.row, zeroed(ref.col))
    else:
        one = _run_g(c, r, NONE3, ref.col)
        two = _run_g(c, r, zeroed(ref.row), ref.col)
    _check_g(one[0], one[1], r, ref, f"{b}x{n}x{d}-{dup}-{side}-only")
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])


def test_g_without_sides_is_zero():
    b, n, d = RAGGED[0]
    c, r = _informative(b, n, d), _reference(b, n, d, "positive", None)
    g, gs = _run_g(c, r, NONE3, NONE3)
    assert float(g.float().abs().max()) == 0.0
    assert float(gs.abs().max()) == 0.0


@pytest.mark.parametrize("b,n,d", RAGGED)
@pytest.mark.parametrize("c0,odd", [(0, True), (8, False), (3, True)])
def test_g_strided_view_stays_inside(b, n, d, c0, odd):
    """A band of a wider slab: an odd row stride at column offsets 0 and 3
    (odd itself), and a stride and offset that keep the rows 16-byte
    aligned."""
    dup, diag = "positive", None
    c, r = _informative(b, n, d), _reference(b, n, d, dup, diag)
    ref = _g_reference(b, n, d, dup, diag)
    width = c0 + n + 5
    width = width | 1 if odd else -(-width // 8) * 8
    slab = torch.full((b + 2, width), SENTINEL, device=DEV,
                      dtype=torch.bfloat16)
    view = slab[1:b + 1, c0:c0 + n]
    g, gs = _run_g(c, r, ref.row, ref.col, g=view)
    assert g.data_ptr() == view.data_ptr()
    _check_g(view, gs, r, ref, f"{b}x{n}x{d}-c0={c0}-ld={width}")
    outside = torch.ones_like(slab, dtype=torch.bool)
    outside[1:b + 1, c0:c0 + n] = False
    assert torch.equal(slab[outside],
                       torch.full_like(slab[outside], SENTINEL))
    dense, _ = _run_g(c, r, ref.row, ref.col)
    assert torch.equal(view, dense)


@pytest.mark.parametrize("kind", ["overflow", "negative"])
def test_g_extreme_ranges(kind):
    c = _range_case(kind)
    r = _ref(c, "positive", None)
    ref = _g_ref(c, r)
    g, gs = _run_g(c, r, ref.row, ref.col)
    _check_g(g, gs, r, ref, kind)


def test_g_ids_are_64_bit():
    b, n, d = RAGGED[0]
    c, r = _informative(b, n, d), _reference(b, n, d, "positive", None)
    ref = _g_reference(b, n, d, "positive", None)
    base = _run_g(c, r, ref.row, ref.col)
    hi = 2 ** 40
    iid = torch.where(c.iid >= 0, c.iid + hi, c.iid)
    tid = torch.where(c.tid >= 0, c.tid + hi, c.tid)
    c_hi = c._replace(iid=iid, tid=tid)
    got = _run_g(c_hi, r, ref.row, ref.col)
    assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])
    half = (torch.arange(b, device=DEV) % 2 == 0) & (c.iid >= 0)
    c2 = c._replace(iid=torch.where(half, iid + 2 ** 32, iid), tid=tid)
    r2 = _ref(c2, "positive", None)
    assert not torch.equal(r2.pos, r.pos)
    ref2 = _g_ref(c2, r2)
    g, gs = _run_g(c2, r2, ref2.row, ref2.col)
    _check_g(g, gs, r2, ref2, "hi-word")


# ---------------------------------------------------------------------------
# Against the positional kernels
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("b,n,d", SHAPES)
@pytest.mark.parametrize("diag", [0, 5])
def test_arange_ids_agree_with_positional_kernels(b, n, d, diag):
    """``img_ids = arange(b) + diag``, ``txt_ids = arange(n)``: the classes
    of ``ops.pair_lse`` / ``ops.softmax_g``.  Agreement within the derived
    bounds is required; whether the bits agree is printed only (two
    separately compiled epilogues need not contract identically)."""
    c0 = _informative(b, n, d)
    c = c0._replace(iid=torch.arange(b, device=DEV) + diag,
                    tid=torch.arange(n, device=DEV))
    r = _ref(c, "positive", None)
    out = _check_lse(c, r, f"{b}x{n}x{d}-arange{diag}")
    row, col = ops.pair_lse(c.zi, c.zt, c.tp)
    assert float((out.row_lse - row).abs().max()) <= 2 * r.eps
    assert float((out.col_lse - col).abs().max()) <= 2 * r.eps
    ref = _g_ref(c, r)
    g, gs = _run_g(c, r, ref.row, ref.col)
    _check_g(g, gs, r, ref, f"{b}x{n}x{d}-arange{diag}")
    # one positive per row: w == pw, which is what the positional kernel
    # subtracts
    assert torch.equal(ref.row[1], ref.row[2])
    g0, gs0 = ops.softmax_g(c.zi, c.zt, c.tp, ref.row[0], ref.row[1],
                            ref.col[0], ref.col[1], diag)
    assert bool(((g.double() - g0.double()).abs() <= 2 * ref.tol).all())
    assert abs(float(gs.double().sum() - gs0.double().sum())) <= 2 * ref.gs_tol
    print(f"SOFTMAX_ID_VS_POSITIONAL {b}x{n}x{d}-diag{diag} "
          f"row_lse_bits={torch.equal(out.row_lse, row)} "
          f"col_lse_bits={torch.equal(out.col_lse, col)} "
          f"g_bits={torch.equal(g, g0)} gs_bits={torch.equal(gs, gs0)}")


# ---------------------------------------------------------------------------
# Bad inputs: each raises before any launch
# ---------------------------------------------------------------------------

def test_validation_errors():
    b, n, d = SHAPES[1]
    c = _informative(b, n, d)
    lse = ops.pair_lse_ids
    with pytest.raises(RuntimeError, match="bf16"):
        lse(c.zi.float(), c.zt, c.tp, c.iid, c.tid)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        lse(c.zi[:, :4], c.zt[:, :4], c.tp, c.iid, c.tid)
    with pytest.raises(RuntimeError, match="img_ids"):
        lse(c.zi, c.zt, c.tp, c.iid.int(), c.tid)
    with pytest.raises(RuntimeError, match="txt_ids"):
        lse(c.zi, c.zt, c.tp, c.iid, c.tid[:-1])
    with pytest.raises(RuntimeError, match="img_ids"):
        lse(c.zi, c.zt, c.tp, c.iid.cpu(), c.tid)
    with pytest.raises(RuntimeError, match="txt_ids"):
        lse(c.zi, c.zt, c.tp, c.iid, c.tid.repeat(2)[::2])
    with pytest.raises(ValueError, match="duplicates"):
        lse(c.zi, c.zt, c.tp, c.iid, c.tid, "drop")

    v = torch.zeros(128, device=DEV)
    ids = (c.iid, c.tid, "positive", None)

    def g(*a, **kw):
        return ops.softmax_g_ids(c.zi, c.zt, c.tp, *a, **kw)

    with pytest.raises(RuntimeError, match="img_ids"):
        g(c.iid.int(), c.tid, "positive", None, v, v, v, v, v, v)
    with pytest.raises(ValueError, match="duplicates"):
        g(c.iid, c.tid, "drop", None, v, v, v, v, v, v)
    for side in ((None, v, v), (v, None, v), (v, v, None)):
        with pytest.raises(RuntimeError, match="together"):
            g(*ids, *side, None, None, None)
        with pytest.raises(RuntimeError, match="together"):
            g(*ids, v, v, v, *side)
    with pytest.raises(RuntimeError, match="row_pw"):
        g(*ids, v, v, v[:5], None, None, None)
    with pytest.raises(RuntimeError, match="g must be"):
        g(*ids, v, v, v, None, None, None,
          g=torch.empty((128, 64), device=DEV, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ops.softmax_g_ids(c.zi[:, :4], c.zt[:, :4], c.tp, *ids, v, v, v,
                          None, None, None)
