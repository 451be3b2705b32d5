"""GPU tests for the split-K weight-gradient kernel (``ops.linear_wgrad``),
its autograd wiring into ``ProjectionTower``, and the in-place bf16 scale
kernel.

The accuracy bound is relative to the library: the reference is the fp32
product ``A.float().T @ X.float()``; torch's own bf16 ``A.T @ X`` has some
max-abs / mean-abs error against it, and the native kernel may have at most
twice that (one extra bf16 rounding position, nothing more)."""

import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from distributed_sigmoid_loss_amd import ops
from distributed_sigmoid_loss_amd.models import ProjectionTower


def make_operands(batch, m, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(batch, m, generator=g).cuda().bfloat16()
    x = torch.randn(batch, n, generator=g).cuda().bfloat16()
    return a, x


def errors(out, ref):
    e = (out.float() - ref).abs()
    return e.max().item(), e.mean().item()


def assert_within_library_bound(dw, a, x, label=""):
    ref = a.float().T @ x.float()
    lib_max, lib_mean = errors(a.T @ x, ref)
    got_max, got_mean = errors(dw, ref)
    print(f"{label} max-abs {got_max:.6g} (library {lib_max:.6g})  "
          f"mean-abs {got_mean:.6g} (library {lib_mean:.6g})")
    assert got_max <= 2 * lib_max
    assert got_mean <= 2 * lib_mean


# (batch, M, N, forced slice count or None for the plan's own)
SHAPES = [
    # one tile, one k-step: with 4 slices, three are empty
    (64, 128, 128, 4),
    (64, 128, 128, None),
    # ragged K tail (not a multiple of 32), several non-square tiles
    (1000, 256, 384, None),
    (1000, 256, 384, 5),
    # workload dims, K one k-step past a slice boundary
    (4128, 768, 768, None),
    (4128, 768, 768, 8),
    # K smaller than one MFMA step
    (8, 768, 768, None),
    (8, 768, 768, 3),
]


@pytest.mark.parametrize("batch,m,n,slices", SHAPES)
def test_wgrad_matches_fp32_within_library_error(batch, m, n, slices):
    a, x = make_operands(batch, m, n)
    dw = ops.linear_wgrad(a, x, slices=slices)
    assert dw.shape == (m, n) and dw.dtype == torch.bfloat16
    assert_within_library_bound(dw, a, x, f"({batch},{m},{n},s={slices})")


def test_partial_tiles_and_asymmetric_operand():
    # M, N multiples of 8 but not of the 128-wide tile; A = identity rows so
    # dW must be exactly the first M rows of X (catches a row/column swap).
    m, n = 136, 200
    x = torch.arange(m * n, dtype=torch.float32).reshape(m, n).remainder(251.0)
    x = x.cuda().bfloat16()
    a = torch.eye(m, device="cuda", dtype=torch.bfloat16)
    assert torch.equal(ops.linear_wgrad(a, x), x)


def test_unsupported_dims_are_refused_and_fall_back():
    a, x = make_operands(64, 130, 128)
    lib = ops._require_lib()
    assert lib.linear_wgrad_plan(64, 130, 128, 256) == 0
    dw = torch.full((130, 128), 7.0, device="cuda", dtype=torch.bfloat16)
    ws = torch.full((2, 130, 128), 7.0, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    rc = lib.linear_wgrad_bf16(
        ctypes.c_void_p(stream), ctypes.c_void_p(a.data_ptr()),
        ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(ws.data_ptr()),
        ctypes.c_void_p(dw.data_ptr()), 64, 130, 128, 130, 128, 2)
    torch.cuda.synchronize()
    assert rc != 0
    assert bool((dw == 7.0).all()) and bool((ws == 7.0).all())
    # null pointer and bad slice count are refused as well
    assert lib.linear_wgrad_bf16(
        ctypes.c_void_p(stream), None, ctypes.c_void_p(x.data_ptr()),
        ctypes.c_void_p(ws.data_ptr()), ctypes.c_void_p(dw.data_ptr()),
        64, 128, 128, 128, 128, 2) != 0
    assert not ops.linear_wgrad_supported(a, x)
    assert torch.equal(ops.linear_wgrad(a, x), a.T @ x)


def test_noncontiguous_dy_matches_contiguous():
    wide, x = make_operands(1000, 512, 384)
    dy = wide[:, 128:384]          # row-strided view, read in place
    assert not dy.is_contiguous()
    assert torch.equal(ops.linear_wgrad(dy, x),
                       ops.linear_wgrad(dy.contiguous(), x))
    dyt = wide[:, :256].T.contiguous().T   # column-major: copied first
    assert dyt.stride(1) != 1
    assert torch.equal(ops.linear_wgrad(dyt, x),
                       ops.linear_wgrad(dyt.contiguous(), x))


def test_bitwise_reproducible():
    a, x = make_operands(4128, 768, 768, seed=1)
    assert torch.equal(ops.linear_wgrad(a, x), ops.linear_wgrad(a, x))


def _tower_grads(x, weight, r):
    tower = ProjectionTower(768, 768).to(device="cuda", dtype=torch.bfloat16)
    with torch.no_grad():
        tower.proj.weight.copy_(weight)
    (tower(x) * r).sum().backward()
    return tower.proj.weight.grad


def test_projection_tower_weight_grad(monkeypatch):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(256, 768, generator=g).cuda().bfloat16()
    r = torch.randn(256, 768, generator=g).cuda().bfloat16()
    w = (torch.randn(768, 768, generator=g) / 768 ** 0.5).cuda().bfloat16()

    monkeypatch.setenv("SIGLIP_NATIVE_WGRAD", "0")
    g_lib = _tower_grads(x, w, r)
    monkeypatch.delenv("SIGLIP_NATIVE_WGRAD")
    g_nat = _tower_grads(x, w, r)

    # dy of the projection, for the fp32 reference of the same product
    y = (x @ w.t()).requires_grad_()
    (ops.l2_normalize(y) * r).sum().backward()
    ref = y.grad.float().T @ x.float()
    lib_max, lib_mean = errors(g_lib, ref)
    nat_max, nat_mean = errors(g_nat, ref)
    print(f"tower max-abs {nat_max:.6g} (library {lib_max:.6g})  "
          f"mean-abs {nat_mean:.6g} (library {lib_mean:.6g})")
    assert nat_max <= 2 * lib_max
    assert nat_mean <= 2 * lib_mean


def test_input_grad_only_when_needed():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(256, 768, generator=g).cuda().bfloat16()
    w = (torch.randn(768, 768, generator=g) / 768 ** 0.5).cuda().bfloat16()
    dy = torch.randn(256, 768, generator=g).cuda().bfloat16()

    class Ctx:
        saved_tensors = (x, w)
        needs_input_grad = (False, True)

    dx, dw = ops._LinearNativeWgrad.backward(Ctx, dy)
    assert dx is None and dw is not None

    xg = x.clone().requires_grad_()
    wg = w.clone().requires_grad_()
    ops.linear_nobias(xg, wg).backward(dy)
    assert torch.equal(xg.grad, dy @ w)
    assert_within_library_bound(wg.grad, dy, x, "autograd dW")

    xn = x.clone()
    wn = w.clone().requires_grad_()
    ops.linear_nobias(xn, wn).backward(dy)
    assert xn.grad is None and torch.equal(wn.grad, wg.grad)


@pytest.mark.parametrize("numel", [8, 1000 * 66, 1000 * 66 + 3, 4096 * 768])
def test_scale_inplace_is_bitwise_torch(numel):
    g = torch.Generator().manual_seed(numel)
    x = torch.randn(numel, generator=g).cuda().bfloat16()
    s = torch.tensor(0.0123, device="cuda")
    expect = x * s.to(torch.bfloat16)
    y = x.clone()
    out = ops.scale_bf16_(y, s)
    assert out.data_ptr() == y.data_ptr()
    assert torch.equal(y, expect)
