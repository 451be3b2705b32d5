"""``ops.band_grad_gemms`` on the CPU, exactly.

Integer-valued bf16 operands make every band product and sum an integer that
bf16 and fp32 hold, so the banded result must equal the float64 one bit for
bit at every step.  ``emit`` copies a fixed ``G`` into the slab it is handed:
a driver that materialised its bands before the GEMMs would hand the last
band's slab to all of them and fail the comparison, so the laziness of the
band iterator is pinned too.
"""

import pytest
import torch

from distributed_sigmoid_loss_amd import ops

B, N, D, DIAG = 48, 200, 32, 37
STEPS = (8, 64, 100, 200, 256)


@pytest.fixture(scope="module")
def case():
    gen = torch.Generator().manual_seed(0)
    zimg = torch.randint(-2, 3, (B, D), generator=gen).to(torch.bfloat16)
    ztxt = torch.randint(-2, 3, (N, D), generator=gen).to(torch.bfloat16)
    G = torch.randint(-1, 2, (B, N), generator=gen).to(torch.bfloat16)
    dzimg = ((G.double() @ ztxt.double()) * 2.0).to(torch.bfloat16)
    dztxt = ((G.double().T @ zimg.double()) * 2.0).to(torch.bfloat16)
    return zimg, ztxt, G, dzimg, dztxt


def _run(case, step, bf16_scale=False, diag_offset=DIAG):
    zimg, ztxt, G = case[:3]
    calls, fired = [], []

    def emit(j0, j1, diag_j, g, gt):
        calls.append((j0, j1, diag_j, g, gt))
        g.copy_(G[:, j0:j1])

    grads = ops.band_grad_gemms(
        zimg, ztxt, step, emit, torch.tensor(2.0), diag_offset=diag_offset,
        on_dztxt=fired.append, bf16_scale=bf16_scale)
    return grads, calls, fired


@pytest.mark.parametrize("bf16_scale", (False, True))
@pytest.mark.parametrize("step", STEPS)
def test_banded_gradients_are_exact(case, step, bf16_scale):
    (dzimg, dztxt), _, fired = _run(case, step, bf16_scale)
    assert dzimg.dtype == dztxt.dtype == torch.bfloat16
    assert torch.equal(dzimg, case[3])
    assert torch.equal(dztxt, case[4])
    # on_dztxt fires once, with the complete text gradient.
    assert len(fired) == 1 and fired[0] is dztxt


def test_a_materialised_band_list_is_not_exact(case):
    """What the lazy iterator protects against: the same bands, all emitted
    into the one slab before ``grad_gemms`` reads any of them."""
    zimg, ztxt, G, dzimg_ref, dztxt_ref = case
    slab = torch.empty((B, 100), dtype=torch.bfloat16)
    bands = []
    for j0, j1, _ in ops.col_bands(N, 100):
        slab.copy_(G[:, j0:j1])
        bands.append(ops.GBand(slab, None, ztxt[j0:j1]))
    dzimg, dztxt = ops.grad_gemms(bands, zimg, N, torch.tensor(2.0))
    assert not torch.equal(dzimg, dzimg_ref)
    assert not torch.equal(dztxt, dztxt_ref)


@pytest.mark.parametrize("step", STEPS)
def test_slab_reuse_tail_and_diagonal(case, step):
    _, calls, _ = _run(case, step)
    width = min(step, N)
    assert [(j0, j1) for j0, j1, *_ in calls] == [
        (j0, min(j0 + width, N)) for j0 in range(0, N, width)]
    full = [g for j0, j1, _, g, _ in calls if j1 - j0 == width]
    tail = [g for j0, j1, _, g, _ in calls if j1 - j0 != width]
    # Full bands share one slab; the ragged tail has one of its own width.
    assert all(g.shape == (B, width) for g in full)
    assert len({g.data_ptr() for g in full}) == 1
    assert len(tail) == (1 if N % width else 0)
    for g in tail:
        assert g.shape == (B, N % width)
        assert g.data_ptr() != full[0].data_ptr()
    for j0, _, diag_j, _, gt in calls:
        assert diag_j == DIAG - j0 and gt is None
    if step >= N:
        assert len(calls) == 1


def test_tail_at_step_64(case):
    _, calls, _ = _run(case, 64)
    j0, j1, _, g, _ = calls[-1]
    assert (j0, j1) == (192, 200) and g.shape == (B, 8)
    assert all(c[3].data_ptr() == calls[0][3].data_ptr() for c in calls[:-1])
    assert g.data_ptr() != calls[0][3].data_ptr()


def test_no_diagonal_stays_none(case):
    _, calls, _ = _run(case, 64, diag_offset=None)
    assert len(calls) == 4 and all(c[2] is None for c in calls)


def test_col_bands_and_step_policy(monkeypatch):
    assert list(ops.col_bands(10, 4, 7)) == [(0, 4, 7), (4, 8, 3), (8, 10, -1)]
    assert list(ops.col_bands(10, 16)) == [(0, 10, None)]
    monkeypatch.delenv("SIGLIP_BANDED_STEP", raising=False)
    assert ops.g_band_step(384, 520, None) == 520
    assert ops.g_band_step(384, 520, 100) == 100
    # 2³² bytes of bf16: the whole block no longer fits one slab.
    assert ops.g_band_step(65536, 32768, None) == ops.banded_col_step(65536)
    assert ops.g_band_step(65536, 32767, None) == 32767
