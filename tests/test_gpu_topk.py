"""GPU tests for the fused top-k kernel (``ops.pair_topk``) and the retrieval
API built on it (``pair_topk`` / ``merge_topk`` / ``retrieval_topk`` with
``impl="hip"``).

Every index comparison is exact.  With integer-valued embeddings the scores
are small integers, exact in fp32 in any summation order, so scores and
indices must be ``torch.equal`` to a float64 stable-sort reference — ties
included, and the reference is first checked to have ties across the
``k`` / ``k+1`` boundary, which is what pins the tie rule.  With realistic
magnitudes the list is checked property by property against the float64
scores and the rank tests' accumulation-error bound

    eps_ij = d · 2^-23 · sum_k |a_ik| |b_jk|.

On the MI355X the largest observed |score − float64 score| was 0.0164 of
eps (printed by ``test_realistic_magnitudes``).
"""

import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from distributed_sigmoid_loss_amd import (merge_topk, ops, pair_topk,
                                          retrieval_topk)
from distributed_sigmoid_loss_amd.losses.retrieval import _torch_pair_topk

DEV = "cuda"

# the rank-count tests' shapes: below one MFMA fragment, ragged on both sides
# of a tile edge, d not a multiple of the K-step, several tiles × K-steps
SHAPES = [(1, 1, 8), (16, 16, 8), (17, 15, 24), (130, 257, 72),
          (256, 256, 128), (513, 129, 40), (300, 520, 768)]
RAGGED = [(17, 15, 24), (130, 257, 72), (513, 129, 40), (300, 520, 768)]
KS = [1, 3, 8, 16]


def offsets(n):
    return [None, 0, 40, -40, n + 5]


def candidates(b, n, off):
    """(b, n) bool: the columns of every row that may be returned."""
    m = torch.ones(b, n, dtype=torch.bool, device=DEV)
    if off is not None:
        i = torch.arange(b, device=DEV)
        j = i + off
        ok = (j >= 0) & (j < n)
        m[i[ok], j[ok]] = False
    return m


def ref_topk(s64, k, off):
    """Float64 stable-sort reference → (scores fp32 (b, k), columns int32
    (b, k), sorted candidate scores (b, n) with −inf behind them)."""
    b, n = s64.shape
    m = candidates(b, n, off)
    s = s64.masked_fill(~m, -math.inf)
    top_s, top_c = torch.sort(s, dim=1, descending=True, stable=True)
    ncand = m.sum(1)
    scores = torch.full((b, k), -math.inf, device=DEV, dtype=torch.float64)
    cols = torch.full((b, k), -1, device=DEV, dtype=torch.long)
    kk = min(k, n)
    valid = torch.arange(kk, device=DEV)[None, :] < ncand[:, None]
    scores[:, :kk] = torch.where(valid, top_s[:, :kk], scores[:, :kk])
    cols[:, :kk] = torch.where(valid, top_c[:, :kk], cols[:, :kk])
    return scores.float(), cols.int(), top_s


@functools.lru_cache(maxsize=None)
def integer_case(b, n, d):
    """Integer-valued bf16 embeddings in [-3, 3] (|s| ≤ 9·768: exact in fp32)
    and their float64 scores."""
    g = torch.Generator().manual_seed(1000 * b + 10 * n + d)
    zi = torch.randint(-3, 4, (b, d), generator=g).to(DEV, torch.bfloat16)
    zt = torch.randint(-3, 4, (n, d), generator=g).to(DEV, torch.bfloat16)
    return zi, zt, zi.double() @ zt.double().T


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

@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("b,n,d", SHAPES)
def test_exact_integer_scores_with_ties(b, n, d, k):
    zi, zt, s64 = integer_case(b, n, d)
    for off in offsets(n):
        ref_s, ref_c, sorted_s = ref_topk(s64, k, off)
        if n >= 129:
            # ties straddle the k / k+1 boundary in some rows
            tie = (sorted_s[:, k - 1] == sorted_s[:, k]) \
                & torch.isfinite(sorted_s[:, k])
            assert bool(tie.any()), f"no boundary ties, off={off}"
        got_s, got_c = ops.pair_topk(zi, zt, k, off)
        assert got_s.dtype == torch.float32 and got_c.dtype == torch.int32
        assert got_s.shape == (b, k) and got_c.shape == (b, k)
        assert torch.equal(got_c, ref_c), f"columns, off={off}"
        assert torch.equal(got_s, ref_s), f"scores, off={off}"


def test_boundary_ties_are_common_at_k16():
    # the share of rows whose 16th and 17th candidates tie: 39 % and 14 %
    for (b, n, d), least in (((130, 257, 72), 0.3), ((300, 520, 768), 0.1)):
        _, _, s64 = integer_case(b, n, d)
        _, _, sorted_s = ref_topk(s64, 16, None)
        assert float((sorted_s[:, 15] == sorted_s[:, 16]).double().mean()) \
            > least


# -- 2. fill ----------------------------------------------------------------

def test_fill_past_the_last_candidate():
    zi, zt, s64 = integer_case(17, 15, 24)
    for off in (None, 0, -3):
        got_s, got_c = ops.pair_topk(zi, zt, 16, off)
        ncand = candidates(17, 15, off).sum(1)
        slot = torch.arange(16, device=DEV)[None, :]
        fill = slot >= ncand[:, None]
        assert bool(fill.any())
        assert bool((got_c[fill] == -1).all())
        assert bool((got_s[fill] == -math.inf).all())
        assert bool((got_c[~fill] >= 0).all())
        assert bool(torch.isfinite(got_s[~fill]).all())
    zi, zt, _ = integer_case(1, 1, 8)
    got_s, got_c = ops.pair_topk(zi, zt, 16, 0)     # no candidate at all
    assert bool((got_c == -1).all()) and bool((got_s == -math.inf).all())


# -- 3. realistic magnitudes --------------------------------------------------

@pytest.mark.parametrize("b,n,d", RAGGED)
def test_realistic_magnitudes(b, n, d):
    zi, zt, s64, eps = normalized_case(b, n, d)
    rows = torch.arange(b, device=DEV)
    worst = 0.0
    for k in (1, 5, 16):
        for off in offsets(n):
            got_s, got_c = ops.pair_topk(zi, zt, k, off)
            cand = candidates(b, n, off)
            ncand = cand.sum(1)
            c = got_c.long()
            valid = c >= 0
            # as many entries as there are candidates, front-packed
            slot = torch.arange(k, device=DEV)[None, :]
            assert torch.equal(valid, slot < ncand[:, None].clamp(max=k))
            assert bool((got_s[~valid] == -math.inf).all())
            cc = c.clamp(min=0)
            # in range, candidates only (never the excluded column), distinct
            assert bool((c < n).all())
            assert bool(cand.gather(1, cc)[valid].all())
            hit = torch.zeros(b, n, dtype=torch.int32, device=DEV)
            hit.scatter_add_(1, cc, valid.int())
            assert int(hit.max()) <= 1
            # each score within eps of the float64 score at its index
            err = (got_s.double() - s64.gather(1, cc)).abs()
            bound = eps.gather(1, cc)
            assert bool((err[valid] <= bound[valid]).all())
            if bool(valid.any()):
                worst = max(worst, float((err[valid] / bound[valid]).max()))
            # non-increasing, indices increasing among equal scores
            both = valid[:, 1:] & valid[:, :-1]
            assert bool((got_s[:, 1:] <= got_s[:, :-1])[both].all())
            eq = both & (got_s[:, 1:] == got_s[:, :-1])
            assert bool((c[:, 1:] > c[:, :-1])[eq].all())
            # nothing left out beats the last entry by more than eps
            full = ncand >= k
            left = cand & (hit == 0) & full[:, None]
            kth = got_s[rows, k - 1].double()
            assert bool(((s64 - eps) <= kth[:, None])[left].all())
    print(f"largest |score - s64| / eps at {(b, n, d)}: {worst:.4f}")
    assert worst <= 1.0


# -- 4. independent of the split, reproducible --------------------------------

def test_split_independence_and_reproducibility():
    b, n, d = 140, 1100, 40            # 9 column tiles
    zi, zt, _, _ = normalized_case(b, n, d)
    zi_int, zt_int, s64 = integer_case(b, n, d)
    for k, off in ((16, 0), (3, None), (8, -40)):
        base_s, base_c = ops.pair_topk(zi, zt, k, off, n_splits=1)
        for ns in (2, 3, 9, 50, None):
            got_s, got_c = ops.pair_topk(zi, zt, k, off, n_splits=ns)
            assert torch.equal(got_c, base_c), f"columns, n_splits={ns}"
            assert torch.equal(got_s.view(torch.int32),
                               base_s.view(torch.int32)), f"n_splits={ns}"
        # ties across split boundaries
        ref_s, ref_c, _ = ref_topk(s64, k, off)
        for ns in (1, 2, 3, 9, 50):
            got_s, got_c = ops.pair_topk(zi_int, zt_int, k, off, n_splits=ns)
            assert torch.equal(got_c, ref_c), f"integer, n_splits={ns}"
            assert torch.equal(got_s, ref_s), f"integer, n_splits={ns}"
    first = ops.pair_topk(zi, zt, 16, 0)
    again = ops.pair_topk(zi, zt, 16, 0)
    assert torch.equal(first[1], again[1])
    assert torch.equal(first[0].view(torch.int32), again[0].view(torch.int32))


# -- 5. column chunks -----------------------------------------------------------

@pytest.mark.parametrize("off", [None, 40])
def test_column_chunks_merge_bitwise(off):
    b, n, d = 300, 520, 768
    bounds = [(0, 100), (100, 357), (357, 520)]     # off the tile grid
    for zi, zt in (normalized_case(b, n, d)[:2], integer_case(b, n, d)[:2]):
        for k in (16, 3):
            whole = pair_topk(zi, zt, k, off, impl="hip")
            assert whole.indices.dtype == torch.long
            parts = [pair_topk(zi, zt[j0:j1], k,
                               None if off is None else off - j0,
                               col_base=j0, impl="hip")
                     for j0, j1 in bounds]
            merged = merge_topk(parts)
            assert torch.equal(merged.indices, whole.indices)
            assert torch.equal(merged.scores.view(torch.int32),
                               whole.scores.view(torch.int32))


# -- 6. the other direction -----------------------------------------------------

@pytest.mark.parametrize("b,n,d", [(130, 257, 72), (513, 129, 40)])
def test_text_to_image_direction(b, n, d):
    zi, zt, s64 = integer_case(b, n, d)
    for off in (None, 0, 40, -40):
        i2t, t2i = retrieval_topk(zi, zt, 8, off, impl="hip")
        ref_s, ref_c, _ = ref_topk(s64, 8, off)
        assert torch.equal(i2t.indices, ref_c.long())
        assert torch.equal(i2t.scores, ref_s)
        ref_s, ref_c, _ = ref_topk(s64.T.contiguous(), 8,
                                   None if off is None else -off)
        assert torch.equal(t2i.indices, ref_c.long())
        assert torch.equal(t2i.scores, ref_s)


# -- 7. 64-bit offsets ------------------------------------------------------------

def test_row_offsets_past_2_to_31():
    # zimg exceeds 2^31 bytes: the last rows are reachable only with 64-bit
    # offsets.  Their excluded positives sit in the last n rows.
    b, n, d, k = 1_398_250, 24, 768, 8
    assert b * d * 2 > 2 ** 31 and b % 128 != 0
    off = -(b - n)
    zi = torch.empty(b, d, device=DEV, dtype=torch.bfloat16).random_(-3, 4)
    zt = torch.empty(n, d, device=DEV, dtype=torch.bfloat16).random_(-3, 4)
    # fp32 is exact here (small integers): the chunked composite is a reference
    ref_s, ref_c = _torch_pair_topk(zi, zt, k, off, row_chunk=262144)
    got_s, got_c = ops.pair_topk(zi, zt, k, off)
    assert torch.equal(got_c.long(), ref_c)
    assert torch.equal(got_s, ref_s)
    # the tail rows carry information: the positive is left out there
    i = torch.arange(b - n, b, device=DEV)
    assert bool((got_c[i].long() != (i + off)[:, None]).all())
    assert got_c[-4096:].unique().numel() == n


# -- 8. bad inputs ------------------------------------------------------------------

def test_bad_inputs_raise():
    zi, zt, _ = integer_case(17, 15, 24)
    errors = (RuntimeError, ValueError)
    with pytest.raises(errors):
        pair_topk(zi, zt, 0, impl="hip")
    with pytest.raises(errors):
        ops.pair_topk(zi, zt, 0)
    with pytest.raises(errors):
        pair_topk(zi, zt, ops.pair_topk_max_k() + 1, impl="hip")
    with pytest.raises(errors):
        ops.pair_topk(zi[:, :20].contiguous(), zt[:, :20].contiguous(), 4)
    with pytest.raises(errors):
        pair_topk(zi.float(), zt.float(), 4, impl="hip")
    with pytest.raises(errors):
        ops.pair_topk(zi, zt[:, :16].contiguous(), 4)
    with pytest.raises(errors):
        ops.pair_topk(zi, zt.cpu(), 4)
    assert ops.pair_topk_max_k() == 16
    # auto: the kernel where it applies, the composite beyond its range
    big = pair_topk(zi, zt, 17)
    assert big.scores.shape == (17, 17) and bool((big.indices[:, 15:] == -1).all())
    torch.cuda.synchronize()
