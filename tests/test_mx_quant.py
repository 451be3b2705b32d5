"""``ops.quantize_mx``'s torch composite (the CPU path and the GPU tests'
reference) against a float64 spelling of the rule, on hand-picked blocks of one
``(2, 160)`` bf16 tensor — five blocks per row, so three pad bytes per scale
row.  Per block: ``amax = m·2^p``; ``e = p − 8`` if ``m ≤ 1.75`` else ``p − 7``,
clamped to ``[−127, 127]``; code ``e + 127`` (``0x7F`` if all zero); elements
``x·2^−e`` rounded to nearest even — exact in float64, so one rounding to
e4m3."""

import math

import pytest
import torch

from distributed_sigmoid_loss_amd import ops, sigmoid_contrastive_loss_ids

E4M3, U8 = torch.float8_e4m3fn, torch.uint8
# (block's first elements — the rest are 0 —, its code, its first bytes)
BLOCKS = [
    ([1.75, 0.5], 119, [0x7E, 0x70]),            # m == 1.75: e = p − 8, 448
    ([1.75 + 2.0 ** -7, -1.0], 120, [0x76, 0xF0]),     # one ulp above: e = p − 7
    ([0.0], 127, [0x00]),                        # all zero
    ([0.25, -3.0], 120, [0x60, 0xFC]),           # the maximum is negative
    # amax 1: ×256; 136 and 152 lie halfway between codes: to the even one
    ([1.0, 136 / 256, 152 / 256, -136 / 256], 119, [0x78, 0x70, 0x72, 0xF0]),
    ([2.0 ** -130], 0, [0x20]),                  # e clamped to −127: ×2^127
    ([1.5 * 2.0 ** 100, 2.0 ** 90], 219, [0x7C, 0x28]),
    ([-2.0 ** -20], 99, [0xF8]),
    ([448.0, 1.0], 127, [0x7E, 0x38]),
    ([1.875 * 2.0 ** -119], 1, [0x77]),          # m > 1.75 next to the clamp
]


def _tensor():
    x = torch.zeros(10, 32, dtype=torch.float64)
    for i, (vals, _, _) in enumerate(BLOCKS):
        x[i, :len(vals)] = torch.tensor(vals, dtype=torch.float64)
    xb = x.reshape(2, 160).bfloat16()
    assert torch.equal(xb.double(), x.reshape(2, 160)), "not bf16 values"
    return xb


def test_composite_follows_the_rule_in_float64():
    xb = _tensor()
    q, e8 = ops.quantize_mx(xb)
    assert (q.dtype, q.shape, e8.dtype, e8.shape) == (E4M3, (2, 160), U8, (2, 8))
    assert bool((e8[:, 5:] == 0x7F).all()), "pad bytes"
    blocks = xb.double().reshape(10, 32)
    codes, got = e8[:, :5].reshape(10), q.view(U8).reshape(10, 32)
    for i, (vals, code, first) in enumerate(BLOCKS):
        amax = float(blocks[i].abs().max())
        mant, exp = math.frexp(amax)              # amax = mant·2^exp = m·2^p
        e = min(max(exp - 1 - (8 if mant <= 0.875 else 7), -127), 127)
        want_code = e + 127 if amax > 0 else 0x7F
        assert want_code == code == int(codes[i]), (i, want_code, int(codes[i]))
        scaled = blocks[i] * 2.0 ** (127 - code)
        assert float(scaled.abs().max()) <= 448.0     # and exact in fp32:
        assert torch.equal(scaled.float().double(), scaled)
        want = scaled.float().to(E4M3).view(U8)
        assert torch.equal(got[i], want), (i, got[i], want)
        assert got[i, :len(first)].tolist() == first, (i, got[i, :4])
    # other dtypes take the same composite: the same bytes from fp32
    q32, e32 = ops.quantize_mx(xb.float())
    assert torch.equal(q32.view(U8), q.view(U8)) and torch.equal(e32, e8)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        ops.quantize_mx(xb[:, :48])


def test_mxfp8_needs_the_hip_path():
    z = torch.nn.functional.normalize(torch.randn(4, 32), dim=-1)
    ids = torch.arange(4)
    with pytest.raises(ValueError, match="mxfp8"):
        sigmoid_contrastive_loss_ids(z, z, torch.tensor(1.0), torch.tensor(0.0),
                                     ids, ids, impl="torch", quant="mxfp8")
