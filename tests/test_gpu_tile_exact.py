"""Exact per-element checks of the 256x256 tile kernel.

Every output of ``siglip_tile`` -- each g / g-transpose slab element and the
three scalars -- is compared with a float64 reference computed from exactly
what the kernel reads (the bf16 values, or the e4m3 bytes and their scales).

The inputs sit in an *informative regime*: ``t' = log(1.5 / std(dot))`` and
``bias = -0.5`` put at least 90 % of ``|g|`` inside [0.05, 0.95] (asserted as
a precondition of every case), so a wrong negative pair moves a slab element
by many ulps and the loss by far more than the scalar bound.  With the usual
``t = 10, bias = -10`` a negative pair has ``g ~ 4.5e-5`` and a slab with all
negatives zero passes any bf16-class tolerance.

Bounds (derived, not measured):

- bf16 g: 1 bf16 ulp of the reference (1/2 ulp is the rounding itself; the
  other 1/2 ulp ~ 2^-9 relative covers ``__expf`` / ``v_rcp_f32`` and the fp32
  dot, which are ~1e-6).
- e4m3 g and g-transpose: against ``(448 * expected).to(float8_e4m3fn)`` no
  element more than one adjacent code away, at most 0.1 % different at all;
  g-transpose bit-equal to g transposed for the per-tensor / mixed policies.
- sign map: ``g < 0`` exactly at ``j == i + diag``, ``g > 0`` elsewhere.
- coverage / containment: slabs are prefilled with a sentinel (bf16 NaN,
  e4m3 byte 0x7F, which the saturating conversion never produces) and live
  inside wider buffers; no sentinel may remain inside and no guard may change.
- scalars: ``|got - ref| <= 1e-4 * sum|term_ref|`` -- 8x the worst-case fp32
  bound 200 * 2^-24 of the <= 200 sequential adds on any path (128 per lane,
  then the wave, block and slot sums).

For per-tensor fp8 the reference works in the kernel's units: the dot is of
the e4m3 values themselves and the scales ride the temperature the kernel
reads (``t' + log s_img + log s_txt``, as ``_logit_operands`` folds them), which
is ``z = (q s_img)(q s_txt)^T e^{t'} + bias`` up to that fp32 sum.
"""

import functools
import itertools
import math
from typing import NamedTuple, Optional

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from distributed_sigmoid_loss_amd import ops

DEV = "cuda"
E4M3 = torch.float8_e4m3fn
SENTINEL8 = 0x7F                      # e4m3fn NaN; |448 g| <= 448 = 0x7E
NANBITS = int(torch.tensor(float("nan"), dtype=torch.bfloat16)
              .view(torch.int16))
SCALAR_RTOL = 1e-4
FAMILIES = ("dyadic", "normalized")

# (policy, mode) for the eight instantiations plus row-wise fp8 (modes 0, 2).
# policy: bf16 = (eb 2, eb_g 2), mixed = (2, 1), fp8 = (1, 1) per-tensor,
# fp8row = (1, 1) with per-row e8m0 scales.
COMBOS = [("bf16", 0), ("bf16", 1), ("bf16", 2), ("mixed", 1), ("mixed", 2),
          ("fp8", 0), ("fp8", 1), ("fp8", 2), ("fp8row", 0), ("fp8row", 2)]


def _kind(policy):
    return "bf16" if policy in ("bf16", "mixed") else policy


def _quant(policy):
    return {"bf16": "bf16", "mixed": "mixed"}.get(policy, "fp8")


# ---------------------------------------------------------------------------
# Inputs and the float64 reference (computed once per key, never modified).
# ---------------------------------------------------------------------------

class _Op(NamedTuple):
    src_i: torch.Tensor           # bf16 embeddings
    src_t: torch.Tensor
    qc: Optional[ops.QuantCache]
    tp: torch.Tensor              # the caller's t'
    bias: torch.Tensor
    zi_k: torch.Tensor            # what the kernel reads
    zt_k: torch.Tensor
    tp_k: torch.Tensor
    rowscales: Optional[tuple]
    dot: torch.Tensor             # float64 (b, n), in the units of tp_k


class _Ref(NamedTuple):
    pos: torch.Tensor             # bool (b, n): j == i + diag
    g: torch.Tensor               # float64 (b, n)
    sums: torch.Tensor            # float64 [loss, sum g*dot, sum g]
    abs_sums: torch.Tensor        # float64 sums of |term|
    informative: float            # fraction of |g| in [0.05, 0.95]


def _rows(family, r, d, gen, rowscale):
    if family == "zeros":
        return torch.zeros(r, d)
    if family == "dyadic":
        vals = torch.tensor([0.0, 0.25, -0.25, 0.5, -0.5, 1.0, -1.0])
        x = vals[torch.randint(0, 7, (r, d), generator=gen)]
    else:
        x = torch.randn(r, d, generator=gen)
        x = x / x.norm(dim=1, keepdim=True)
    if rowscale:
        x = x * torch.exp2(torch.randint(-6, 7, (r, 1), generator=gen).float())
    return x


def _f64(q):
    return q.float().double()


@functools.lru_cache(maxsize=4)
def _operands(family, kind, b, n, d):
    gen = torch.Generator().manual_seed(b * 1000003 + n * 7919 + d)
    rowscale = kind == "fp8row"
    src_i = _rows(family, b, d, gen, rowscale).to(DEV).bfloat16()
    src_t = _rows(family, n, d, gen, rowscale).to(DEV).bfloat16()
    qc = None
    if kind == "bf16":
        a, bm = src_i.double(), src_t.double()
    elif kind == "fp8":
        qc = ops.quantize_fp8_pair(src_i, src_t)
        a = _f64(qc.zi_q) * qc.si.double()
        bm = _f64(qc.zt_q) * qc.st.double()
    else:
        qc = ops.quantize_fp8_rowwise_pair(src_i, src_t)
        a = _f64(qc.zi_q) * torch.exp2(qc.zi_e8.double() - 127)[:, None]
        bm = _f64(qc.zt_q) * torch.exp2(qc.zt_e8.double() - 127)[:, None]
        for e8, ratio in ((qc.zi_e8, qc.zi_ratio), (qc.zt_e8, qc.zt_ratio)):
            assert torch.equal(ratio.double(),
                               torch.exp2(e8.double() - e8.double().max()))
    dot = a @ bm.T
    s = float(dot.std()) if dot.numel() > 1 else float(dot.abs().max())
    if not (s > 0.0 and math.isfinite(s)):
        s = 1.0
    tp = torch.tensor(math.log(1.5 / s), device=DEV, dtype=torch.float32)
    bias = torch.tensor(0.0 if family == "zeros" else -0.5, device=DEV)
    zi_k, zt_k, tp_k, rowscales = ops._logit_operands(
        "bf16" if kind == "bf16" else "fp8", src_i, src_t, tp, qc)
    if kind == "fp8":
        dot = _f64(qc.zi_q) @ _f64(qc.zt_q).T
    return _Op(src_i, src_t, qc, tp, bias, zi_k, zt_k, tp_k, rowscales, dot)


def _pos_mask(b, n, diag):
    if diag is None:
        return torch.zeros((b, n), dtype=torch.bool, device=DEV)
    i = torch.arange(b, device=DEV)[:, None]
    j = torch.arange(n, device=DEV)[None, :]
    return j == i + diag


@functools.lru_cache(maxsize=4)
def _reference(family, kind, b, n, d, diag):
    op = _operands(family, kind, b, n, d)
    z = op.dot * op.tp_k.double().exp() + op.bias.double()
    pos = _pos_mask(b, n, diag)
    x = torch.where(pos, -z, z)                      # -l * z
    terms = torch.logaddexp(x, torch.zeros_like(x))  # softplus
    sig = torch.sigmoid(x)
    g = torch.where(pos, -sig, sig)                  # -l * sigma(x)
    gd = g * op.dot
    sums = torch.stack([terms.sum(), gd.sum(), g.sum()])
    abs_sums = torch.stack([terms.sum(), gd.abs().sum(), g.abs().sum()])
    inf = float(((sig >= 0.05) & (sig <= 0.95)).double().mean())
    return _Ref(pos, g, sums, abs_sums, inf)


# ---------------------------------------------------------------------------
# Sentinel-filled output slabs inside wider buffers.
# ---------------------------------------------------------------------------

class _Slabs:
    """g is the column view ``[:b, off:off+n]`` of a ``(b + 8, width)`` slab;
    g-transpose (e4m3 only) is the middle of a flat byte buffer with
    ``16 b + 64`` guard bytes on both sides."""

    def __init__(self, b, n, e4, off=None, width=None):
        self.b, self.n, self.e4 = b, n, e4
        self.off = off = (16 if e4 else 8) if off is None else off
        # default width: a multiple of 16, so aligned shapes stay aligned
        self.width = width = (-(-(n + 2 * off) // 16) * 16
                              if width is None else width)
        assert width >= off + n
        self.gt = self.flat = None
        if e4:
            self.wide = torch.full((b + 8, width), SENTINEL8, device=DEV,
                                   dtype=torch.uint8)
            typed = self.wide.view(E4M3)
            self.guard = 16 * b + 64
            self.flat = torch.full((2 * self.guard + n * b,), SENTINEL8,
                                   device=DEV, dtype=torch.uint8)
            self.gt = self.flat[self.guard:self.guard + n * b].view(
                n, b).view(E4M3)
        else:
            typed = self.wide = torch.full((b + 8, width), float("nan"),
                                           device=DEV, dtype=torch.bfloat16)
        self.g_slab = typed[:b]                   # what siglip_fwd_g takes
        self.g = typed[:b, off:off + n]

    def gt_slab(self):
        """(off + n, b) slab whose rows off: are the g-transpose region."""
        lo = self.guard - self.off * self.b
        return self.flat[lo:self.guard + self.n * self.b].view(
            self.off + self.n, self.b).view(E4M3)

    def bits(self):
        return self.wide if self.e4 else self.wide.view(torch.int16)

    def check_sentinels(self):
        b, n, off = self.b, self.n, self.off
        bits = self.bits()
        sent = SENTINEL8 if self.e4 else NANBITS
        inside = torch.zeros_like(bits, dtype=torch.bool)
        inside[:b, off:off + n] = True
        left = int((bits[:b, off:off + n] == sent).sum())
        assert left == 0, f"{left} g elements never written"
        hit = int((bits[~inside] != sent).sum())
        assert hit == 0, f"{hit} g guard elements overwritten"
        if self.e4:
            mid = self.flat[self.guard:self.guard + n * b]
            left = int((mid == SENTINEL8).sum())
            assert left == 0, f"{left} gt elements never written"
            hit = int((self.flat[:self.guard] != SENTINEL8).sum()
                      + (self.flat[self.guard + n * b:] != SENTINEL8).sum())
            assert hit == 0, f"{hit} gt guard bytes overwritten"


# ---------------------------------------------------------------------------
# Launch and checks.
# ---------------------------------------------------------------------------

def _launch(op, policy, mode, diag, slabs, via="tile"):
    """Run one mode; returns the reduced float64 [loss, sum g*dot, sum g]."""
    quant = _quant(policy)
    if via == "tile":
        out = ops._out_buf(DEV)
        ops._launch_tile(mode, quant, op.zi_k, op.zt_k, op.tp_k, op.bias, out,
                         g=slabs.g if mode else None,
                         gt=slabs.gt if mode else None,
                         diag_offset=diag, rowscales=op.rowscales)
    elif mode == 0:
        loss = ops.siglip_fwd(op.src_i, op.src_t, op.tp, op.bias, diag,
                              quant=quant, qcache=op.qc)
        return torch.stack([loss.double(), loss.double() * 0,
                            loss.double() * 0])
    else:
        assert mode == 2
        out, _, _ = ops.siglip_fwd_g(
            op.src_i, op.src_t, op.tp, op.bias, diag, quant=quant,
            qcache=op.qc, g_slab=slabs.g_slab,
            gt_slab=slabs.gt_slab() if slabs.e4 else None, col0=slabs.off)
    assert int((out[:, 3:] != 0).sum()) == 0, "scalar buffer padding written"
    return ops.reduce_out3(out).double()


def _check_scalars(got, ref, mode, tag):
    idx = {0: (0,), 1: (1, 2), 2: (0, 1, 2)}[mode]
    err = (got - ref.sums).abs() / ref.abs_sums.clamp_min(1e-300)
    print(f"TILE_EXACT scalars {tag} "
          + " ".join(f"rel{i}={float(err[i]):.3e}" for i in idx))
    for i in range(3):
        if i in idx:
            assert float((got[i] - ref.sums[i]).abs()) <= \
                SCALAR_RTOL * float(ref.abs_sums[i]), \
                (i, float(got[i]), float(ref.sums[i]), float(err[i]))
        else:
            assert float(got[i]) == 0.0, (i, float(got[i]))


def _ordinal(codes):
    """e4m3 byte -> signed position on the value line (+-0 both 0)."""
    mag = (codes & 0x7F).to(torch.int16)
    return torch.where(codes >= 128, -mag, mag)


def _check_codes(codes, expected, pos, rowwise, tag):
    """``codes``: uint8 e4m3 slab; ``expected``: float64 values before x448."""
    exp_codes = (448.0 * expected).float().contiguous().to(E4M3).view(
        torch.uint8)
    got_o, exp_o = _ordinal(codes), _ordinal(exp_codes)
    diff = (got_o - exp_o).abs()
    frac = float((diff != 0).double().mean())
    print(f"TILE_EXACT e4m3 {tag} maxcode={int(diff.max())} frac={frac:.3e}")
    assert int(diff.max()) <= 1, f"{tag}: {int(diff.max())} codes away"
    assert frac <= 1e-3, f"{tag}: {frac:.3%} of elements differ"
    if rowwise:
        # ratios down to 2^-12 may flush an element to +-0: the sign sets
        # are those of the expected codes (the diagonal wherever nonzero)
        neg, plus = exp_o < 0, exp_o > 0
        assert bool(((exp_o >= 0) | pos).all())
    else:
        neg, plus = pos, ~pos
    assert torch.equal(got_o < 0, neg), f"{tag}: negative set != diagonal"
    assert torch.equal(got_o > 0, plus), f"{tag}: positive set != complement"


def _check_slabs(s, op, ref, policy, tag):
    b, n, off = s.b, s.n, s.off
    s.check_sentinels()
    if policy == "bf16":
        got = s.g.double()
        ulp = torch.exp2(torch.floor(torch.log2(ref.g.abs())) - 7)
        worst = float(((got - ref.g).abs() / ulp).max())
        print(f"TILE_EXACT bf16 {tag} ulp={worst:.4f}")
        assert worst <= 1.0, f"{tag}: g off by {worst:.3f} bf16 ulp"
        assert torch.equal(got < 0, ref.pos), "negative set != diagonal"
        assert torch.equal(got > 0, ~ref.pos), "positive set != complement"
        return
    rowwise = policy == "fp8row"
    codes = s.wide[:b, off:off + n]
    gt_codes = s.flat[s.guard:s.guard + n * b].view(n, b)
    if rowwise:
        _check_codes(codes, ref.g * op.qc.zt_ratio.double()[None, :],
                     ref.pos, True, tag + " g")
        _check_codes(gt_codes, (ref.g * op.qc.zi_ratio.double()[:, None]).T,
                     ref.pos.T, True, tag + " gt")
    else:
        _check_codes(codes, ref.g, ref.pos, False, tag + " g")
        assert torch.equal(gt_codes, codes.T), "gt != g transposed"


def _run(policy, mode, family, b, n, d, diag, via="tile", off=None,
         width=None):
    tag = f"{policy}-m{mode}-{family}-{b}x{n}x{d}-diag{diag}-{via}"
    kind = _kind(policy)
    op = _operands(family, kind, b, n, d)
    ref = _reference(family, kind, b, n, d, diag)
    assert ref.informative >= 0.9, \
        f"uninformative inputs: {ref.informative:.3f} of |g| in [.05, .95]"
    slabs = _Slabs(b, n, policy != "bf16", off, width) if mode else None
    got = _launch(op, policy, mode, diag, slabs, via)
    _check_scalars(got, ref, mode, tag)
    if mode:
        _check_slabs(slabs, op, ref, policy, tag)
    return got, slabs


def _cases(bf16_shapes, fp8_shapes, combos=COMBOS, families=FAMILIES,
           diags=(0,)):
    """(policy, mode, family, b, n, d, diag) over shapes x combos, shape
    outermost so the cached reference is shared; the e4m3 slab pair needs
    b % 4 == 0 (packed g-transpose stores), so those combos keep such b."""
    out = []
    for kind, shapes in (("bf16", bf16_shapes), ("fp8", fp8_shapes)):
        for (b, n, d), family, diag in itertools.product(
                shapes, families, diags):
            for policy, mode in combos:
                if (_kind(policy) == "bf16") != (kind == "bf16"):
                    continue
                if policy != "bf16" and mode != 0 and b % 4:
                    continue
                out.append(pytest.param(
                    policy, mode, family, b, n, d, diag,
                    id=f"{policy}-m{mode}-{family}-{b}x{n}x{d}-diag{diag}"))
    return out


_ARGS = "policy,mode,family,b,n,d,diag"


# Interior-only kernel: every tile full, one and three K-steps (odd count:
# the double-buffer toggle ends on the other buffer).
@pytest.mark.parametrize(_ARGS, _cases(
    [(256, 256, 64), (256, 256, 192), (512, 256, 64), (512, 256, 192)],
    [(256, 256, 128), (256, 256, 384), (512, 256, 128), (512, 256, 384)]))
def test_interior_only(policy, mode, family, b, n, d, diag):
    _run(policy, mode, family, b, n, d, diag)


# A K tail sends full tiles down the guarded, zero-filling staging path.
@pytest.mark.parametrize(_ARGS, _cases(
    [(256, 256, d) for d in (8, 24, 72, 136)],
    [(256, 256, d) for d in (16, 112, 144)]))
def test_k_tail(policy, mode, family, b, n, d, diag):
    _run(policy, mode, family, b, n, d, diag)


# Ragged edges in both directions (with a K tail on top).
_RAGGED = [(1, 1), (255, 257), (257, 513), (300, 260), (260, 257), (4, 513)]


@pytest.mark.parametrize(_ARGS, _cases(
    [(b, n, 72) for b, n in _RAGGED], [(b, n, 144) for b, n in _RAGGED]))
def test_ragged_edges(policy, mode, family, b, n, d, diag):
    _run(policy, mode, family, b, n, d, diag)


# Interior blocks inside the general kernel, LDS-staged writeback
# (GT_ALIGNED): b = 272 and the slab stride are 16-aligned.
@pytest.mark.parametrize(_ARGS, _cases([(272, 520, 64)], [(272, 520, 128)]))
def test_general_kernel_interior_block_staged(policy, mode, family, b, n, d,
                                              diag):
    _run(policy, mode, family, b, n, d, diag)


# ... and the direct-store path.  bf16: n = 264 inside a slab of stride 268
# (268 % 8 != 0; the stride leaves room for two guard columns per side, not
# eight).  e4m3: b = 260 is a multiple of 4 but not of 16.
@pytest.mark.parametrize(_ARGS, _cases(
    [(272, 264, 64)], [], combos=[("bf16", 1), ("bf16", 2)]))
def test_general_kernel_interior_block_direct_bf16(policy, mode, family, b, n,
                                                   d, diag):
    _run(policy, mode, family, b, n, d, diag, off=2, width=268)


@pytest.mark.parametrize(_ARGS, _cases(
    [(260, 512, 64)], [(260, 512, 128)],
    combos=[c for c in COMBOS if c[0] != "bf16" and c[1] != 0]))
def test_general_kernel_interior_block_direct_e4m3(policy, mode, family, b, n,
                                                   d, diag):
    _run(policy, mode, family, b, n, d, diag)


# Diagonals: tile corners (0, 255, 256, -256), a single positive in a corner
# (n - 1, -(b - 1)), none at all (>= n, <= -b, None).  (512, 512) runs the
# interior-only kernel, (260, 516) the general one with ragged edges.
def _diag_cases():
    out = []
    for (b, n), combos in (((512, 512), COMBOS),
                           ((260, 516), [c for c in COMBOS if c[1] == 2])):
        diags = (0, 255, 256, -256, n - 1, -(b - 1), n, n + 7, -b, -b - 300,
                 None)
        d = 64 if (b, n) == (512, 512) else 72
        for k, diag in enumerate(diags):
            out += _cases([(b, n, d)], [(b, n, 2 * d)], combos=combos,
                          families=(FAMILIES[k % 2],), diags=(diag,))
    return out


@pytest.mark.parametrize(_ARGS, _diag_cases())
def test_diagonals(policy, mode, family, b, n, d, diag):
    _run(policy, mode, family, b, n, d, diag)


# The public entry points reach the same kernels with the same operands.
@pytest.mark.parametrize(_ARGS, _cases(
    [(256, 256, 64), (300, 260, 72)], [(256, 256, 128), (300, 260, 144)],
    combos=[c for c in COMBOS if c[1] != 1], families=("normalized",),
    diags=(-3,)))
def test_public_entry_points(policy, mode, family, b, n, d, diag):
    _run(policy, mode, family, b, n, d, diag, via="public")


# Counting: all-zero embeddings and bias = 0 make every g = +-1/2 and every
# loss term ln 2 -- "every pair exactly once", independent of the matmul.
@pytest.mark.parametrize("b,n,diag", [(512, 256, 0), (300, 260, -3),
                                      (260, 513, 7), (257, 255, None)])
@pytest.mark.parametrize("policy,mode", COMBOS)
def test_counting_all_zero(policy, mode, b, n, diag):
    if policy != "bf16" and mode != 0 and b % 4:
        b += 3      # the e4m3 slab pair needs b % 4 == 0
    d = 64 if _kind(policy) == "bf16" else 128
    got, _ = _run(policy, mode, "zeros", b, n, d, diag)
    n_pos = int(_pos_mask(b, n, diag).sum())
    if mode != 0:
        assert abs(float(got[2]) - (b * n - 2 * n_pos) / 2) < 0.25
    if mode != 1:
        full = b * n * math.log(2.0)
        assert abs(float(got[0]) - full) <= SCALAR_RTOL * full


# Block-remap flags: every combination selects a tile -> block map (and, for
# SIGLIP_NT_G, another store instantiation); each must be a bijection.  Grids:
# 5x3 interior blocks, the same with ragged edges, and 17x2 / 18x3 so that
# GROUP_M = 16 has a short last group.
_FLAG_VARS = ("SIGLIP_XCD_SWZ", "SIGLIP_GROUP_SWZ", "SIGLIP_GROUP_M",
              "SIGLIP_NT_G")
_FLAG_GRIDS = [("bf16", "dyadic", 1280, 768, 64),
               ("bf16", "normalized", 1281, 770, 72),
               ("bf16", "dyadic", 4352, 512, 8),
               ("bf16", "normalized", 4353, 513, 8),
               ("fp8", "normalized", 1280, 768, 128),
               ("fp8", "dyadic", 1284, 770, 144)]
_FLAG_DIAG = 5
_flag_baselines = {}


def _flag_baseline(grid):
    """The default-flags mode-2 run of ``grid``, fully checked, made once."""
    if grid not in _flag_baselines:
        policy, family, b, n, d = grid
        with pytest.MonkeyPatch.context() as mp:
            for var in _FLAG_VARS:
                mp.delenv(var, raising=False)
            _, slabs = _run(policy, 2, family, b, n, d, _FLAG_DIAG)
        _flag_baselines[grid] = slabs
    return _flag_baselines[grid]


@pytest.mark.parametrize("xcd,grp,gm,nt", list(itertools.product(
    (0, 1), (0, 1), (1, 4, 8, 16), (0, 1))))
@pytest.mark.parametrize("grid", _FLAG_GRIDS,
                         ids=lambda g: f"{g[0]}-{g[2]}x{g[3]}x{g[4]}")
def test_block_remap_flags(monkeypatch, grid, xcd, grp, gm, nt):
    policy, family, b, n, d = grid
    base = _flag_baseline(grid)
    for var, val in zip(_FLAG_VARS, (xcd, grp, gm, nt)):
        monkeypatch.setenv(var, str(val))
    tag = f"{policy}-{b}x{n}x{d}-flags{xcd}{grp}-{gm}-{nt}"
    op = _operands(family, policy, b, n, d)
    ref = _reference(family, policy, b, n, d, _FLAG_DIAG)
    slabs = _Slabs(b, n, policy != "bf16")
    got = _launch(op, policy, 2, _FLAG_DIAG, slabs)
    _check_scalars(got, ref, 2, tag + "-m2")
    # guards included: bit-identical output and nothing outside it
    assert torch.equal(slabs.bits(), base.bits()), "g differs from default"
    if slabs.e4:
        assert torch.equal(slabs.flat, base.flat), "gt differs from default"
    got = _launch(op, policy, 0, _FLAG_DIAG, None)
    _check_scalars(got, ref, 0, tag + "-m0")
