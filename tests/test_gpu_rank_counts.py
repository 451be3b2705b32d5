"""GPU tests for the fused rank-count kernel (``ops.pair_rank_counts``) and
the retrieval metrics built on it (``retrieval_ranks(impl="hip")``).

Every comparison is exact (``torch.equal``).  That is possible because the
inputs are chosen so that the kernel's fp32 MFMA accumulation cannot change a
comparison: either the scores are small integers (exact in fp32 in any
summation order, so even ties are reproduced), or every threshold sits in the
middle of a gap between adjacent scores that is wider than four times a loose
bound on the fp32 accumulation error,

    eps_ij = d · 2^-23 · sum_k |a_ik| |b_jk|,

and the test asserts that precondition on the float64 reference before it
looks at the kernel's result.
"""

import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from distributed_sigmoid_loss_amd import ops, retrieval_ranks

DEV = "cuda"

# below one MFMA fragment, ragged on both sides of a tile edge, d not a
# multiple of the K-step, several tiles × several K-steps
SHAPES = [(1, 1, 8), (16, 16, 8), (17, 15, 24), (130, 257, 72),
          (256, 256, 128), (513, 129, 40), (300, 520, 768)]
RAGGED = [(17, 15, 24), (130, 257, 72), (513, 129, 40), (300, 520, 768)]


def offsets(n):
    return [None, 0, 40, -40, n + 5]


def countable(b, n, off):
    """(b, n) bool: inside the block by construction, minus the positives."""
    m = torch.ones(b, n, dtype=torch.bool, device=DEV)
    if off is not None:
        i = torch.arange(b, device=DEV)
        j = i + off
        ok = (j >= 0) & (j < n)
        m[i[ok], j[ok]] = False
    return m


def ref_counts(s64, row_thr, col_thr, off):
    """Brute-force int32 counts from float64 scores."""
    m = countable(s64.shape[0], s64.shape[1], off)
    rc = ((s64 > row_thr.double()[:, None]) & m).sum(1).int()
    cc = ((s64 > col_thr.double()[None, :]) & m).sum(0).int()
    return rc, cc


@functools.lru_cache(maxsize=None)
def integer_case(b, n, d):
    """Integer-valued bf16 embeddings in [-3, 3] (|s| ≤ 9·768: exact in fp32),
    their float64 scores, and thresholds drawn from each row's / column's own
    scores so that exact ties occur."""
    g = torch.Generator().manual_seed(1000 * b + 10 * n + d)
    zi = torch.randint(-3, 4, (b, d), generator=g).to(DEV, torch.bfloat16)
    zt = torch.randint(-3, 4, (n, d), generator=g).to(DEV, torch.bfloat16)
    s64 = zi.double() @ zt.double().T
    jr = torch.randint(0, n, (b,), generator=g).to(DEV)
    ic = torch.randint(0, b, (n,), generator=g).to(DEV)
    row_thr = s64[torch.arange(b, device=DEV), jr].float()
    col_thr = s64[ic, torch.arange(n, device=DEV)].float()
    return zi, zt, s64, row_thr, col_thr


@functools.lru_cache(maxsize=None)
def normalized_case(b, n, d):
    """L2-normalised random bf16 embeddings, float64 scores of those bf16
    values and the accumulation-error bound eps (b, n)."""
    g = torch.Generator().manual_seed(7000 * b + 13 * n + d)
    zi = torch.nn.functional.normalize(torch.randn(b, d, generator=g), dim=-1)
    zt = torch.nn.functional.normalize(torch.randn(n, d, generator=g), dim=-1)
    zi, zt = zi.to(DEV, torch.bfloat16), zt.to(DEV, torch.bfloat16)
    s64 = zi.double() @ zt.double().T
    eps = d * 2.0 ** -23 * (zi.double().abs() @ zt.double().abs().T)
    return zi, zt, s64, eps


# -- 1. exact, with ties ----------------------------------------------------

@pytest.mark.parametrize("b,n,d", SHAPES)
def test_exact_integer_scores_with_ties(b, n, d):
    zi, zt, s64, row_thr, col_thr = integer_case(b, n, d)
    # the thresholds are scores of the row / column itself: ties exist
    assert bool((s64 == row_thr.double()[:, None]).any(1).all())
    assert bool((s64 == col_thr.double()[None, :]).any(0).all())
    for off in offsets(n):
        rc, cc = ops.pair_rank_counts(zi, zt, row_thr, col_thr, off)
        ref_rc, ref_cc = ref_counts(s64, row_thr, col_thr, off)
        assert rc.dtype == torch.int32 and cc.dtype == torch.int32
        assert torch.equal(rc, ref_rc), f"rows, off={off}"
        assert torch.equal(cc, ref_cc), f"cols, off={off}"


# -- 2. masks ---------------------------------------------------------------

@pytest.mark.parametrize("b,n,d", RAGGED)
def test_masks_padding_and_positive(b, n, d):
    zi, zt, _, _ = normalized_case(b, n, d)
    ninf_r = torch.full((b,), -math.inf, device=DEV)
    ninf_c = torch.full((n,), -math.inf, device=DEV)
    for off in offsets(n):
        m = countable(b, n, off)
        rc, cc = ops.pair_rank_counts(zi, zt, ninf_r, ninf_c, off)
        # everything countable is above −inf: n minus [row has a positive]
        assert torch.equal(rc, m.sum(1).int()), f"rows, off={off}"
        assert torch.equal(cc, m.sum(0).int()), f"cols, off={off}"
        if off is None:
            assert bool((rc == n).all()) and bool((cc == b).all())
        rc, cc = ops.pair_rank_counts(zi, zt, -ninf_r, -ninf_c, off)
        assert not bool(rc.any()) and not bool(cc.any())


# -- 3. realistic magnitudes, still exact -------------------------------------

def gap_thresholds(s64, eps):
    """Per row of ``s64``: a threshold in the middle of a gap between adjacent
    sorted scores wider than 4·eps_row, as near as possible to the target
    count (cycling 0, 1, n/2, n−1, n).  Returns (thr, gap, eps_row, shift)."""
    rows, n = s64.shape
    v = s64.sort(dim=1).values
    ext = torch.cat([v[:, :1] - 1.0, v, v[:, -1:] + 1.0], dim=1)  # n + 2
    gaps = ext[:, 1:] - ext[:, :-1]               # position p: count = n − p
    eps_row = eps.max(dim=1).values
    targets = torch.tensor([0, 1, n // 2, n - 1, n], device=s64.device)
    want = n - targets[torch.arange(rows, device=s64.device) % 5].clamp(0, n)
    pos = torch.arange(n + 1, device=s64.device)
    dist = (pos[None, :] - want[:, None]).abs().double()
    dist[gaps <= 4 * eps_row[:, None]] = math.inf
    p = dist.argmin(dim=1)
    r = torch.arange(rows, device=s64.device)
    thr = 0.5 * (ext[r, p] + ext[r, p + 1])
    return thr, gaps[r, p], eps_row, dist[r, p]


@pytest.mark.parametrize("off", [None, 0])
@pytest.mark.parametrize("b,n,d", [(130, 257, 72), (64, 64, 8),
                                   (256, 256, 128), (300, 520, 768)])
def test_exact_at_realistic_magnitudes(b, n, d, off):
    zi, zt, s64, eps = normalized_case(b, n, d)
    row_thr, rgap, reps, rshift = gap_thresholds(s64, eps)
    col_thr, cgap, ceps, cshift = gap_thresholds(s64.T.contiguous(),
                                                 eps.T.contiguous())
    # the precondition that makes exactness a fair demand
    assert bool((rgap > 4 * reps).all()) and bool((cgap > 4 * ceps).all())
    assert rshift.max().item() <= 8 and cshift.max().item() <= 8
    row_thr, col_thr = row_thr.float(), col_thr.float()
    rc, cc = ops.pair_rank_counts(zi, zt, row_thr, col_thr, off)
    ref_rc, ref_cc = ref_counts(s64, row_thr, col_thr, off)
    assert torch.equal(rc, ref_rc)
    assert torch.equal(cc, ref_cc)


# -- 4. contract --------------------------------------------------------------

def test_counts_accumulate_into_given_buffers():
    zi, zt, s64, row_thr, col_thr = integer_case(130, 257, 72)
    rc, cc = ops.pair_rank_counts(zi, zt, row_thr, col_thr, 40)
    rc2, cc2 = ops.pair_rank_counts(zi, zt, row_thr, col_thr, 40,
                                    row_cnt=rc.clone(), col_cnt=cc.clone())
    assert torch.equal(rc2, 2 * rc) and torch.equal(cc2, 2 * cc)
    ref_rc, ref_cc = ref_counts(s64, row_thr, col_thr, 40)
    assert torch.equal(rc, ref_rc) and torch.equal(cc, ref_cc)


@pytest.mark.parametrize("off", [None, 0, 40, -40])
def test_column_chunks_reproduce_single_call(off):
    zi, zt, _, row_thr, col_thr = integer_case(300, 520, 768)
    n = zt.shape[0]
    rc, cc = ops.pair_rank_counts(zi, zt, row_thr, col_thr, off)
    rc_acc = torch.zeros_like(rc)
    parts = []
    for j0 in range(0, n, 200):
        j1 = min(n, j0 + 200)
        _, part = ops.pair_rank_counts(
            zi, zt[j0:j1], row_thr, col_thr[j0:j1],
            None if off is None else off - j0, row_cnt=rc_acc)
        parts.append(part)
    assert torch.equal(rc_acc, rc)
    assert torch.equal(torch.cat(parts), cc)


def test_one_sided_calls():
    zi, zt, _, row_thr, col_thr = integer_case(513, 129, 40)
    rc, cc = ops.pair_rank_counts(zi, zt, row_thr, col_thr, 0)
    r_only, none = ops.pair_rank_counts(zi, zt, row_thr=row_thr,
                                        diag_offset=0)
    assert none is None and torch.equal(r_only, rc)
    none, c_only = ops.pair_rank_counts(zi, zt, col_thr=col_thr,
                                        diag_offset=0)
    assert none is None and torch.equal(c_only, cc)
    assert ops.pair_rank_counts(zi, zt) == (None, None)


def test_bitwise_reproducible():
    zi, zt, s64, eps = normalized_case(300, 520, 768)
    thr_r, thr_c = s64[:, 0].float(), s64[0, :].float()
    first = ops.pair_rank_counts(zi, zt, thr_r, thr_c, 0)
    again = ops.pair_rank_counts(zi, zt, thr_r, thr_c, 0)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


def big_case(b, n, d, off):
    """Integer-valued operands and chunked fp32 reference counts (exact: the
    scores are small integers) for a block too tall for a float64 matmul."""
    zi = torch.empty(b, d, device=DEV, dtype=torch.bfloat16).random_(-3, 4)
    zt = torch.empty(n, d, device=DEV, dtype=torch.bfloat16).random_(-3, 4)
    row_thr = (torch.arange(b, device=DEV) % 7 - 3).float() * 20.0
    col_thr = (torch.arange(n, device=DEV) % 5 - 2).float() * 20.0
    ref_rc = torch.empty(b, device=DEV, dtype=torch.int32)
    ref_cc = torch.zeros(n, device=DEV, dtype=torch.int32)
    cols = torch.arange(n, device=DEV)
    for r0 in range(0, b, 262144):
        r1 = min(b, r0 + 262144)
        s = zi[r0:r1].float() @ zt.float().T
        pos = torch.arange(r0, r1, device=DEV) + off
        s.masked_fill_(cols[None, :] == pos[:, None], -math.inf)
        ref_rc[r0:r1] = (s > row_thr[r0:r1, None]).sum(1)
        ref_cc += (s > col_thr[None, :]).sum(0).int()
    return zi, zt, row_thr, col_thr, ref_rc, ref_cc


def test_row_offsets_past_2_to_31():
    # b·d elements exceed 2^31 (and bytes 2^32): the last rows are reachable
    # only with 64-bit offsets.  Their positives sit in the last n rows.
    b, n, d = 2_796_250, 24, 768
    assert b * d > 2 ** 31 and b % 128 != 0
    off = -(b - n)
    zi, zt, row_thr, col_thr, ref_rc, ref_cc = big_case(b, n, d, off)
    rc, cc = ops.pair_rank_counts(zi, zt, row_thr, col_thr, off)
    assert torch.equal(rc, ref_rc)
    assert torch.equal(cc, ref_cc)
    # the tail rows carry information: not all zero, not all n
    tail = ref_rc[-4096:]
    assert 0 < tail.sum().item() < 4096 * n


def test_bad_inputs_raise():
    zi, zt, _, row_thr, col_thr = integer_case(17, 15, 24)
    with pytest.raises(RuntimeError):
        ops.pair_rank_counts(zi.float(), zt.float(), row_thr, col_thr)
    with pytest.raises(RuntimeError):
        ops.pair_rank_counts(zi[:, :20].contiguous(), zt[:, :20].contiguous(),
                             row_thr, col_thr)
    with pytest.raises(RuntimeError):
        ops.pair_rank_counts(zi, zt, row_thr[:-1], col_thr)
    with pytest.raises(RuntimeError):
        ops.pair_rank_counts(zi, zt, row_thr, torch.cat([col_thr, col_thr]))
    with pytest.raises(RuntimeError):
        ops.pair_rank_counts(zi, zt, row_thr.double(), col_thr)
    with pytest.raises(RuntimeError):
        ops.pair_rank_counts(zi, zt, row_thr, col_thr,
                             row_cnt=torch.zeros(17, device=DEV))
    with pytest.raises(RuntimeError):
        ops.pair_rank_counts(zi, zt, row_thr.cpu(), col_thr)


# -- 5. end to end --------------------------------------------------------------

def brute_ranks(s64, off):
    """Float64 brute-force (i2t, t2i) ranks, −1 without a positive."""
    b, n = s64.shape
    i = torch.arange(b, device=s64.device)
    j = i + (0 if off is None else off)
    ok = (j >= 0) & (j < n) if off is not None else torch.zeros_like(i).bool()
    i, j = i[ok], j[ok]
    m = countable(b, n, off)
    i2t = torch.full((b,), -1, dtype=torch.long, device=s64.device)
    t2i = torch.full((n,), -1, dtype=torch.long, device=s64.device)
    p = s64[i, j]
    i2t[i] = ((s64[i] > p[:, None]) & m[i]).sum(1)
    t2i[j] = ((s64[:, j] > p[None, :]) & m[:, j]).sum(0)
    return i2t, t2i


@pytest.mark.parametrize("b,n,d", [(17, 15, 24), (130, 257, 72),
                                   (300, 520, 768)])
def test_retrieval_ranks_exact_on_integer_inputs(b, n, d):
    zi, zt, s64, _, _ = integer_case(b, n, d)
    for off in offsets(n):
        got = retrieval_ranks(zi, zt, off, impl="hip")
        ref_i2t, ref_t2i = brute_ranks(s64, off)
        assert got.i2t.dtype == torch.long and got.t2i.dtype == torch.long
        assert torch.equal(got.i2t, ref_i2t), f"i2t, off={off}"
        assert torch.equal(got.t2i, ref_t2i), f"t2i, off={off}"


def test_perfect_and_shifted_towers():
    b, d = 200, 256
    z = torch.zeros(b, d)
    z[torch.arange(b), torch.arange(b)] = 1.0 + (torch.arange(b) % 7).float()
    z = z.to(DEV, torch.bfloat16)
    r = retrieval_ranks(z, z, 0, impl="hip")
    assert not bool(r.i2t.any()) and not bool(r.t2i.any())
    r = retrieval_ranks(z, z.roll(1, 0), 0, impl="hip")
    assert bool((r.i2t == 1).all()) and bool((r.t2i == 1).all())


@pytest.mark.parametrize("b,n,off", [(130, 257, 0), (200, 333, 40),
                                     (256, 256, 0)])
def test_retrieval_ranks_within_float64_bracket(b, n, off):
    zi, zt, s64, eps = normalized_case(b, n, 64)
    m = countable(b, n, off)
    i = torch.arange(b, device=DEV)
    j = i + off
    ok = (j >= 0) & (j < n)
    i, j = i[ok], j[ok]
    p, pe = s64[i, j], eps[i, j]
    # surely above / possibly above the positive, both perturbed by eps
    lo_r = ((s64[i] - eps[i] > (p + pe)[:, None]) & m[i]).sum(1)
    hi_r = ((s64[i] + eps[i] >= (p - pe)[:, None]) & m[i]).sum(1)
    lo_c = ((s64[:, j] - eps[:, j] > (p + pe)[None, :]) & m[:, j]).sum(0)
    hi_c = ((s64[:, j] + eps[:, j] >= (p - pe)[None, :]) & m[:, j]).sum(0)
    # the bracket pins at least 90 % of the ranks (reference alone)
    assert (lo_r == hi_r).double().mean().item() >= 0.9
    assert (lo_c == hi_c).double().mean().item() >= 0.9
    got = retrieval_ranks(zi, zt, off, impl="hip")
    assert bool((got.i2t[i] >= lo_r).all()) and bool((got.i2t[i] <= hi_r).all())
    assert bool((got.t2i[j] >= lo_c).all()) and bool((got.t2i[j] <= hi_c).all())
    none_r = torch.ones(b, dtype=torch.bool, device=DEV)
    none_r[i] = False
    none_c = torch.ones(n, dtype=torch.bool, device=DEV)
    none_c[j] = False
    assert bool((got.i2t[none_r] == -1).all())
    assert bool((got.t2i[none_c] == -1).all())
