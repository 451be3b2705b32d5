"""GPU tests for the sample-ID top-k kernel (``ops.pair_topk_ids``) and
``pair_topk_ids`` / ``retrieval_topk_ids`` with ``impl="hip"``.

Every comparison is exact against a float64 brute force over ``pair_classes``
(the negatives, a stable descending sort, ``−inf`` → ``(−inf, −1)``): the
embeddings are integer-valued bf16, so fp32 holds every score exactly.
"""

import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from distributed_sigmoid_loss_amd import (merge_topk, ops, pair_topk_ids,
                                          retrieval_topk_ids)
from distributed_sigmoid_loss_amd.losses.id_labels import pair_classes

DEV = "cuda"
NINF = -math.inf
# ragged on both sides of a tile edge, d off the K-step, several tiles
SHAPES = [(17, 15, 24), (130, 257, 72), (513, 129, 40), (300, 520, 768),
          (256, 256, 128)]
CASES = [s + (lay,) for s in SHAPES for lay in ("grouped", "shuffled")]
MODES = [("positive", None), ("ignore", 0), ("ignore", 40), ("ignore", -40),
         ("ignore", "n+5")]
KS = (1, 3, 8, 16)


@functools.lru_cache(maxsize=None)
def case(b, n, d, layout):
    """Integer bf16 embeddings, their float64 scores and ids: 3 images and 5
    consecutive texts per id, so groups straddle the tile edges; *shuffled*
    permutes the texts; ~10 % of either side masked; ids missing on either
    side; one pair of its own.  Memoised, shared and read-only."""
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
    return zi, zt, s64, img_ids.to(DEV), txt_ids.to(DEV)


def classes(img_ids, txt_ids, mode, off):
    """(negative, positive, masked) with masked taken out of the first two."""
    off = txt_ids.shape[0] + 5 if off == "n+5" else off
    pos, masked = pair_classes(img_ids, txt_ids, mode, off)
    return ~pos & ~masked, pos & ~masked, masked, off


def ref_topk(s64, keep, k):
    """``keep`` in order, cut or filled to ``k``, and entry ``k + 1``'s score
    (to see a tie across the boundary)."""
    s, c = torch.sort(s64.masked_fill(~keep, NINF), dim=1, descending=True,
                      stable=True)
    pad = max(0, k + 1 - s.shape[1])
    s = torch.nn.functional.pad(s, (0, pad), value=NINF)[:, :k + 1]
    c = torch.nn.functional.pad(c, (0, pad), value=-1)[:, :k + 1]
    c = torch.where(s == NINF, torch.full_like(c, -1), c)
    return s[:, :k].float(), c[:, :k].int(), s[:, k]


def check(got, want, what):
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), what


@pytest.mark.parametrize("b,n,d,layout", CASES)
def test_exact_with_ties(b, n, d, layout):
    zi, zt, s64, ii, ti = case(b, n, d, layout)
    if layout == "grouped" and max(b, n) > 128:    # both sides of the shortcut
        eq = (ii[:, None] == ti[None, :]) & (ii >= 0)[:, None]
        tiles = torch.nn.functional.max_pool2d(eq[None, None].float(), 128,
                                               ceil_mode=True)
        assert bool((tiles == 0).any()) and bool((tiles == 1).any())
    for mode, off in MODES:
        neg, pos, masked, off = classes(ii, ti, mode, off)
        for k in KS:
            ws, wc, nxt = ref_topk(s64, neg, k)
            assert bool((wc[1] == -1).all())       # a masked row is all fill
            if n >= 129:
                assert bool(((ws[:, -1] == nxt) & (nxt > NINF)).any()), "tie"
                assert not torch.equal(ref_topk(s64, neg | masked, k)[1], wc)
                if mode == "positive":
                    assert not torch.equal(ref_topk(s64, neg | pos, k)[1], wc)
            elif k == 16:                          # candidates run out
                assert bool(((wc[:, 0] >= 0) & (wc[:, -1] == -1)).any())
            got = ops.pair_topk_ids(zi, zt, k, ii, ti, mode, off)
            check(got, (ws, wc), f"{mode} {off} k={k}")


@pytest.mark.parametrize("layout", ["grouped", "shuffled"])
def test_ids_are_compared_as_64_bit(layout):
    zi, zt, s64, ii, ti = case(130, 257, 72, layout)
    ii = torch.where(ii >= 0, ii + 2 ** 40, ii)
    ti = torch.where(ti >= 0, ti + 2 ** 40, ti)
    half = (torch.arange(130, device=DEV) % 2 == 0) & (ii >= 0)
    ii = torch.where(half, ii + 2 ** 32, ii)       # equal low words only
    neg, pos, _, _ = classes(ii, ti, "positive", None)
    assert not bool(pos[half].any()) and bool(pos.any())
    check(ops.pair_topk_ids(zi, zt, 8, ii, ti), ref_topk(s64, neg, 8)[:2],
          layout)


@pytest.mark.parametrize("mode,off", [("positive", None), ("ignore", 40)])
def test_split_and_chunk_invariance(mode, off):
    b, n, d = 300, 520, 768
    zi, zt, _, ii, ti = case(b, n, d, "shuffled")
    want = ops.pair_topk_ids(zi, zt, 8, ii, ti, mode, off)
    for n_splits in (1, 2, 3, 50):
        check(ops.pair_topk_ids(zi, zt, 8, ii, ti, mode, off, n_splits), want,
              f"n_splits={n_splits}")
    parts = [pair_topk_ids(zi, zt[j0:j0 + 100], 8, ii, ti[j0:j0 + 100], mode,
                           None if off is None else off - j0, col_base=j0,
                           impl="hip")
             for j0 in range(0, n, 100)]               # off the tile grid
    merged = merge_topk(parts)
    check((merged.scores, merged.indices.int()), want, "column chunks")


@pytest.mark.parametrize("b,n,d", [(130, 257, 72), (300, 520, 768)])
def test_special_cases_equal_the_positional_kernel(b, n, d):
    zi, zt, _, _, _ = case(b, n, d, "grouped")
    ar_b, ar_n = torch.arange(b, device=DEV), torch.arange(n, device=DEV)
    for off in (0, 40):
        check(ops.pair_topk_ids(zi, zt, 16, ar_b + off, ar_n),
              ops.pair_topk(zi, zt, 16, off), f"arange {off}")
    for off in (-40, n + 5):
        check(ops.pair_topk_ids(zi, zt, 16, ar_b, ar_n + b, "ignore", off),
              ops.pair_topk(zi, zt, 16, off), f"distinct {off}")


@pytest.mark.parametrize("mode,off", [("positive", 0), ("ignore", 40)])
def test_exchanged_direction(mode, off):
    zi, zt, s64, ii, ti = case(130, 257, 72, "shuffled")
    _, t2i = retrieval_topk_ids(zi, zt, 8, ii, ti, mode, off, impl="hip")
    neg = classes(ti, ii, mode, -off)[0]
    ws, wc, _ = ref_topk(s64.T.contiguous(), neg, 8)
    assert torch.equal(t2i.scores, ws) and torch.equal(t2i.indices, wc.long())


@pytest.mark.parametrize("bad", ["dtype", "length", "device", "k0", "k17",
                                 "mode", "d"])
def test_bad_inputs_raise_before_any_launch(bad):
    zi, zt, _, ii, ti = case(17, 15, 24, "grouped")
    k, mode = 3, "positive"
    if bad == "dtype":
        ii = ii.int()
    elif bad == "length":
        ti = ti[:-1]
    elif bad == "device":
        ii = ii.cpu()
    elif bad in ("k0", "k17"):
        k = int(bad[1:])
    elif bad == "mode":
        mode = "drop"
    elif bad == "d":
        zi, zt = zi[:, :20].contiguous(), zt[:, :20].contiguous()
    with pytest.raises((RuntimeError, ValueError)):
        ops.pair_topk_ids(zi, zt, k, ii, ti, mode)
