"""GPU tests for the sample-ID rank kernels (``ops.pair_best_positive_ids``,
``ops.pair_rank_counts_ids``) and ``retrieval_ranks_ids(impl="hip")``.

Every comparison is exact against a float64 brute force over ``pair_classes``:
the embeddings are integer-valued bf16, so fp32 holds every score exactly.
"""

import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from distributed_sigmoid_loss_amd import (ops, retrieval_ranks,
                                          retrieval_ranks_ids)
from distributed_sigmoid_loss_amd.losses.id_labels import pair_classes

DEV = "cuda"
NINF = -math.inf
# ragged on both sides of a tile edge, d off the K-step, several tiles
SHAPES = [(17, 15, 24), (130, 257, 72), (513, 129, 40), (300, 520, 768),
          (256, 256, 128)]
CASES = [s + (lay,) for s in SHAPES for lay in ("grouped", "shuffled")]
MODES = [("positive", None), ("ignore", 0), ("ignore", 40), ("ignore", -40),
         ("ignore", "n+5")]


@functools.lru_cache(maxsize=None)
def case(b, n, d, layout):
    """Integer bf16 embeddings, their float64 scores, ids (3 images and 5
    consecutive texts per id, so groups straddle the tile edges; *shuffled*
    permutes the texts, so positives fall in off-diagonal tiles; ~10 % of
    either side masked; ids missing on either side) and thresholds drawn
    from each row's / column's own scores, so that ties occur.  Memoised and
    shared between the tests: the tensors are read-only, a test that needs
    other ids derives new tensors from them."""
    g = torch.Generator().manual_seed(1000 * b + 10 * n + d)
    zi = torch.randint(-3, 4, (b, d), generator=g).to(DEV, torch.bfloat16)
    zt = torch.randint(-3, 4, (n, d), generator=g).to(DEV, torch.bfloat16)
    img_ids, txt_ids = torch.arange(b) // 3, torch.arange(n) // 5
    if layout == "shuffled":
        txt_ids = txt_ids[torch.randperm(n, generator=g)]
    img_ids[torch.rand(b, generator=g) < 0.1] = -1
    txt_ids[torch.rand(n, generator=g) < 0.1] = -1
    img_ids[1], txt_ids[2] = -1, -1
    img_ids[-2:] = 10 ** 5                         # absent from the texts
    img_ids[0], txt_ids[0] = 10 ** 6, 10 ** 6      # one pair of its own,
    zi[0] = -zt[0]                                 # its score negative
    s64 = zi.double() @ zt.double().T
    jr = torch.randint(0, n, (b,), generator=g).to(DEV)
    ic = torch.randint(0, b, (n,), generator=g).to(DEV)
    row_thr = s64[torch.arange(b, device=DEV), jr].float()
    col_thr = s64[ic, torch.arange(n, device=DEV)].float()
    return zi, zt, s64, img_ids.to(DEV), txt_ids.to(DEV), row_thr, col_thr


def classes(img_ids, txt_ids, mode, off):
    """(positive, negative) with the masked pairs taken out, and masked."""
    off = txt_ids.shape[0] + 5 if off == "n+5" else off
    pos, masked = pair_classes(img_ids, txt_ids, mode, off)
    return pos & ~masked, ~pos & ~masked, masked, off


def ref_best(s64, pos):
    sp = s64.masked_fill(~pos, NINF)
    return sp.amax(1).float(), sp.amax(0).float()


def ref_counts(s64, keep, row_thr, col_thr):
    rc = ((s64 > row_thr.double()[:, None]) & keep).sum(1).int()
    cc = ((s64 > col_thr.double()[None, :]) & keep).sum(0).int()
    return rc, cc


@pytest.mark.parametrize("b,n,d,layout", CASES)
def test_best_positive(b, n, d, layout):
    zi, zt, s64, ii, ti, _, _ = case(b, n, d, layout)
    for mode, off in MODES:
        pos, _, _, off = classes(ii, ti, mode, off)
        rb, cb = ref_best(s64, pos)
        if mode == "positive":
            # several positives, none (unmasked), masked, a negative best
            assert bool((pos.sum(1) > 1).any())
            assert bool(((pos.sum(1) == 0) & (ii >= 0)).any())
            assert rb[1] == NINF and cb[2] == NINF
            assert bool(((rb < 0) & (rb > NINF)).any())
            if layout == "grouped" and max(b, n) > 128:   # a tile with none
                tiles = torch.nn.functional.max_pool2d(
                    pos[None, None].float(), 128, ceil_mode=True)
                assert bool((tiles == 0).any())
        k_rb, k_cb = ops.pair_best_positive_ids(zi, zt, ii, ti, mode, off)
        assert k_rb.dtype == torch.float32 and k_cb.dtype == torch.float32
        assert torch.equal(k_rb, rb), f"rows, {mode} {off}"
        assert torch.equal(k_cb, cb), f"cols, {mode} {off}"


@pytest.mark.parametrize("b,n,d,layout", CASES)
def test_counts_with_ties(b, n, d, layout):
    zi, zt, s64, ii, ti, row_thr, col_thr = case(b, n, d, layout)
    for mode, off in MODES:
        pos, neg, masked, off = classes(ii, ti, mode, off)
        rc, cc = ref_counts(s64, neg, row_thr, col_thr)
        # a wrong class predicate would show on both sides
        for wrong in (neg | pos, neg | masked):
            if bool((wrong & ~neg).any()):
                w_rc, w_cc = ref_counts(s64, wrong, row_thr, col_thr)
                assert not torch.equal(w_rc, rc) and not torch.equal(w_cc, cc)
        assert bool(masked.any()) and (bool(pos.any()) or off not in (None, 0))
        k_rc, k_cc = ops.pair_rank_counts_ids(zi, zt, row_thr, col_thr, ii, ti,
                                              mode, off)
        assert torch.equal(k_rc, rc), f"rows, {mode} {off}"
        assert torch.equal(k_cc, cc), f"cols, {mode} {off}"


@pytest.mark.parametrize("layout", ["grouped", "shuffled"])
def test_ids_are_compared_as_64_bit(layout):
    zi, zt, s64, ii, ti, row_thr, col_thr = case(130, 257, 72, layout)
    ii = torch.where(ii >= 0, ii + 2 ** 40, ii)
    ti = torch.where(ti >= 0, ti + 2 ** 40, ti)
    half = (torch.arange(130, device=DEV) % 2 == 0) & (ii >= 0)
    ii = torch.where(half, ii + 2 ** 32, ii)       # equal low words only
    pos, neg, _, _ = classes(ii, ti, "positive", None)
    assert not bool(pos[half].any()) and bool(pos.any())
    rb, cb = ref_best(s64, pos)
    rc, cc = ref_counts(s64, neg, row_thr, col_thr)
    k_rb, k_cb = ops.pair_best_positive_ids(zi, zt, ii, ti)
    k_rc, k_cc = ops.pair_rank_counts_ids(zi, zt, row_thr, col_thr, ii, ti)
    assert torch.equal(k_rb, rb) and torch.equal(k_cb, cb)
    assert torch.equal(k_rc, rc) and torch.equal(k_cc, cc)


@pytest.mark.parametrize("mode,off", [("positive", None), ("ignore", 40)])
@pytest.mark.parametrize("b,n,d", [(130, 257, 72), (300, 520, 768)])
def test_column_chunks_accumulate_and_sides_omit(b, n, d, mode, off):
    zi, zt, _, ii, ti, row_thr, col_thr = case(b, n, d, "shuffled")
    rb, cb = ops.pair_best_positive_ids(zi, zt, ii, ti, mode, off)
    rc, cc = ops.pair_rank_counts_ids(zi, zt, row_thr, col_thr, ii, ti, mode,
                                      off)
    a_rb = torch.full((b,), NINF, device=DEV)
    a_cb = torch.full((n,), NINF, device=DEV)
    a_rc = torch.zeros(b, device=DEV, dtype=torch.int32)
    a_cc = torch.zeros(n, device=DEV, dtype=torch.int32)
    for j0 in range(0, n, 100):                    # off the tile grid
        j1 = min(n, j0 + 100)
        off_j = None if off is None else off - j0
        ops.pair_best_positive_ids(zi, zt[j0:j1], ii, ti[j0:j1], mode, off_j,
                                   row_best=a_rb, col_best=a_cb[j0:j1])
        ops.pair_rank_counts_ids(zi, zt[j0:j1], row_thr, col_thr[j0:j1], ii,
                                 ti[j0:j1], mode, off_j, row_cnt=a_rc,
                                 col_cnt=a_cc[j0:j1])
    assert torch.equal(a_rb, rb) and torch.equal(a_cb, cb)
    assert torch.equal(a_rc, rc) and torch.equal(a_cc, cc)
    # one side only
    none, o_cb = ops.pair_best_positive_ids(zi, zt, ii, ti, mode, off,
                                            rows=False)
    assert none is None and torch.equal(o_cb, cb)
    o_rc, none = ops.pair_rank_counts_ids(zi, zt, row_thr, None, ii, ti, mode,
                                          off)
    assert none is None and torch.equal(o_rc, rc)


@pytest.mark.parametrize("b,n,d,layout", CASES)
def test_retrieval_ranks_ids(b, n, d, layout):
    zi, zt, s64, ii, ti, _, _ = case(b, n, d, layout)
    pos, neg, _, _ = classes(ii, ti, "positive", None)
    rb, cb = ref_best(s64, pos)
    i2t = ((s64 > rb.double()[:, None]) & neg).sum(1)
    t2i = ((s64 > cb.double()[None, :]) & neg).sum(0)
    i2t[rb == NINF], t2i[cb == NINF] = -1, -1
    got = retrieval_ranks_ids(zi, zt, ii, ti, impl="hip")
    assert torch.equal(got.i2t, i2t) and torch.equal(got.t2i, t2i)
    # distinct ids: the positional ranks
    ar_b, ar_n = torch.arange(b, device=DEV), torch.arange(n, device=DEV)
    for off in (0, 40):
        want = retrieval_ranks(zi, zt, off, impl="hip")
        got = retrieval_ranks_ids(zi, zt, ar_b + off, ar_n, impl="hip")
        assert torch.equal(got.i2t, want.i2t)
        assert torch.equal(got.t2i, want.t2i)
    for off in (-40, n + 5):
        want = retrieval_ranks(zi, zt, off, impl="hip")
        got = retrieval_ranks_ids(zi, zt, ar_b, ar_n + b, "ignore", off,
                                  impl="hip")
        assert torch.equal(got.i2t, want.i2t)
        assert torch.equal(got.t2i, want.t2i)


@pytest.mark.parametrize("bad", ["dtype", "length", "device", "half", "mode"])
def test_bad_inputs_raise_before_any_launch(bad):
    zi, zt, _, ii, ti, row_thr, col_thr = case(17, 15, 24, "grouped")
    cnt = torch.zeros(17, device=DEV, dtype=torch.int32)
    best = torch.full((17,), NINF, device=DEV)
    mode = "positive"
    if bad == "dtype":
        ii = ii.int()
    elif bad == "length":
        ti = ti[:-1]
    elif bad == "device":
        ii = ii.cpu()
    elif bad == "mode":
        mode = "drop"
    with pytest.raises((RuntimeError, ValueError)):
        ops.pair_rank_counts_ids(zi, zt, None if bad == "half" else row_thr,
                                 col_thr, ii, ti, mode, row_cnt=cnt)
    with pytest.raises((RuntimeError, ValueError)):
        ops.pair_best_positive_ids(zi, zt, ii, ti, mode, row_best=best,
                                   rows=bad != "half")
    assert int(cnt.sum()) == 0 and bool((best == NINF).all())
