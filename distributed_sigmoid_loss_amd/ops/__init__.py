"""HIP kernel dispatch for the fused SigLIP loss (MI355X / gfx950).

Loads the in-tree ``_siglip_hip.so`` (built by ``ops.build``) via ctypes and
exposes:

- :func:`siglip_fwd` — fused logits+logsigmoid+sum forward over a (b, n)
  block; the logits matrix never leaves MFMA accumulators.
- :func:`siglip_fwd_g` / :func:`siglip_bwd_from_g` — the default training
  pair ("saved-g"): one kernel emits loss + the dL/dlogit slab + both
  scalar partials, and backward is just the two ``(b,n)×(n,d)`` gradient
  GEMMs on the libraries (rocBLAS bf16 via ``torch.matmul``, tuned
  hipBLASLt fp8 via ``torch._scaled_mm``).
- :func:`siglip_bwd` — recompute backward for explicit ``col_chunk`` runs
  and batches whose g slab would not fit: the recompute kernel re-derives
  logit tiles and emits g slab by slab, O(b · col_chunk) workspace.
- quantization policies: ``bf16`` | ``fp8`` (e4m3 logits via the MX-scaled
  MFMA — per-tensor scales folded into the temperature, or per-row e8m0
  hardware dequant with ``SIGLIP_FP8_ROWWISE=1``) | ``mixed`` (bf16
  logits, fp8 gradient GEMMs).
- fused tower helpers: :func:`l2_normalize` (single-pass fwd/bwd) and the
  fused fp8 quantizers.
- tower backward: :func:`linear_wgrad` (split-K ``dyᵀ @ x`` with a
  deterministic two-stage reduction), wired into the projection towers by
  :func:`linear_nobias`; :func:`scale_bf16_` (in-place vectorized scale of
  the saved-g gradient products).
- retrieval metrics: :func:`pair_rank_counts` — per-row and per-column
  counts of the scores above a threshold, a second (integer) reduction over
  the same never-materialized pair grid (``losses/retrieval.py`` turns them
  into ranks and recall@k).
- softmax (InfoNCE) loss: :func:`pair_lse` — row and column log-sum-exp of
  the pair grid — and :func:`softmax_g` — its dL/dlogit slab and per-tile
  ``Σ g·s`` partials (``losses/softmax_loss.py`` builds the loss, its
  backward and the distributed form on them).
- retrieval itself: :func:`pair_topk` — the ``k`` best scoring columns of
  every row of the pair grid, optionally without the positive (hard-negative
  mining), from running per-row lists kept across column tiles
  (``losses/retrieval.py`` adds both directions, chunk merging and the
  distributed form).
- sample-ID labels: :func:`sigmoid_ids` — the sigmoid loss whose positives,
  negatives and ignored pairs come from int64 id vectors (several positives
  per row, duplicates switched off, padding rows), as per-tile
  ``(loss, Σ g·s, Σ g)`` partials plus the optional dL/dlogit slab
  (``losses/id_labels.py`` builds the loss and its two backward regimes).
- sample-ID labels for the softmax loss: :func:`pair_lse_ids` — masked row
  and column log-sum-exp plus each row's and column's positive-logit sum and
  positive count — and :func:`softmax_g_ids` — the dL/dlogit slab with
  several positives per row and masked pairs at exactly 0
  (``losses/softmax_loss.py`` builds the multi-positive InfoNCE loss on
  them).

Host structure: every tile-kernel launch goes through :func:`_launch_tile`,
the only caller of the extension's single ``siglip_tile`` entry point; every
backward regime (recompute, saved-g, banded saved-g, the fp8 ring) runs its
two gradient GEMMs through :func:`grad_gemms` and its scalar gradients
through :func:`scalar_grads`; every column-banded recompute backward (the
sigmoid, sample-ID and softmax losses) hands its g-emitting kernel to
:func:`band_grad_gemms`; a quantization made once per step travels as a
:class:`QuantCache`.

These are *loud* paths: calling them on a GPU without the built extension
raises — there is no silent eager fallback on device (CPU fallbacks live in
``losses/functional.py`` and are CPU-only by construction).
"""

from __future__ import annotations

import ctypes
import dataclasses
import os
from typing import NamedTuple, Optional

import torch

from .build import SO_PATH, build as build_extension

_DIAG_NONE = -(2 ** 31)

# Kernel scalar outputs land in a zeroed (8, 32)-float buffer — one 128-B
# cache-line slot per XCD (per-block atomics stay XCD-local; a single shared
# line measured as a serialized ~10ns/op drain).  Slot layout:
# [0] loss, [1] Σg·dot, [2] Σg.  Reduce with the helpers below.
_OUT_SLOTS, _OUT_STRIDE = 8, 32


def _out_buf(device) -> torch.Tensor:
    return torch.zeros((_OUT_SLOTS, _OUT_STRIDE), device=device,
                       dtype=torch.float32)


def reduce_out3(buf: torch.Tensor) -> torch.Tensor:
    """Sum the per-XCD slots of a kernel scalar-output buffer →
    ``[loss, Σg·dot, Σg]`` (whichever the mode wrote; others are 0)."""
    return buf[:, :3].sum(dim=0)


def _kernel_flags(default_gm: str = "4") -> int:
    # bit 0: XCD-contiguous block remap — default ON: together with the
    #        grouped walk it measured best (+4%, profiles/flag_matrix_gm4.log
    #        and profiles/README.md); SIGLIP_XCD_SWZ=0 disables.
    # bit 1: grouped block walk for L2 panel reuse (default on;
    #        SIGLIP_GROUP_SWZ=0 disables for A/B profiling).
    # bit 2: non-temporal g/gᵀ slab stores (SIGLIP_NT_G=1; default off —
    #        measured a regression on every mode, profiles round 2).
    # bits 4-5: GROUP_M locality-group height.  Per-mode defaults from the
    #        round-2 sweep (gpurun sweep2): plain fwd is fastest at gm=8
    #        (854 TF), the g-emitting modes at gm=4 (the slab stores change
    #        the L2 picture); SIGLIP_GROUP_M overrides both.
    f = 0
    if os.environ.get("SIGLIP_XCD_SWZ", "1") != "0":
        f |= 1
    if os.environ.get("SIGLIP_GROUP_SWZ", "1") != "0":
        f |= 2
    if os.environ.get("SIGLIP_NT_G", "0") == "1":
        f |= 4
    gm = os.environ.get("SIGLIP_GROUP_M", default_gm)
    f |= {"8": 0, "1": 1, "4": 2, "16": 3}.get(gm, 0) << 4
    # bits 8-23: workgroup cap of the persistent bf16 interior kernel
    #        (SIGLIP_TILE_WGS; 0 / unset = min(tiles, CUs)) — tests, sweeps.
    # bit 24: SIGLIP_PERSISTENT=0 launches the same kernel with one tile per
    #        workgroup, for A/B runs.
    f |= (int(os.environ.get("SIGLIP_TILE_WGS", "0")) & 0xffff) << 8
    if os.environ.get("SIGLIP_PERSISTENT", "1") == "0":
        f |= 1 << 24
    return f

_lib = None
_lib_err: Optional[str] = None
_tuned_loaded = False


def load_tuned_gemms() -> bool:
    """Point torch's TunableOp at the shipped MI355X-tuned GEMM table so
    ``torch._scaled_mm`` picks the tuned hipBLASLt kernel for the fp8 grad
    GEMMs (measured 0.52 vs 0.99 ms at the B=32k shape; bf16 rocBLAS
    defaults were already optimal, so this is loaded only for the
    fp8/mixed policies).  Tuning itself stays OFF — shapes missing from
    the table use the normal heuristics."""
    global _tuned_loaded
    if _tuned_loaded:
        return True
    if os.environ.get("PYTORCH_TUNABLEOP_TUNING", "0") == "1":
        # Explicit tuning session (e.g. regenerating the table): leave
        # torch's env-driven TunableOp configuration alone.
        return False
    if not torch.cuda.is_available():
        return False
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                        "tunableop_mi355x.csv")
    if not os.path.exists(path):
        return False
    try:
        t = torch.cuda.tunable
        t.enable(True)
        t.tuning_enable(False)
        t.read_file(path)
        _tuned_loaded = True
    except Exception:  # pragma: no cover - tunable API availability
        return False
    return True


_P, _I, _L = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong

# Every export of the extension, name → argument types; all return int.
_EXPORTS = {
    "siglip_ext_abi": [],
    # (stream, mode, eb, eb_g, 11 pointers, b, n, d, ldg, diag, flags)
    "siglip_tile": [_P] + [_I] * 3 + [_P] * 11 + [_I] * 6,
    "l2norm_fwd_bf16": [_P] * 4 + [_I] * 2 + [ctypes.c_float],
    "l2norm_bwd_bf16": [_P] * 5 + [_I] * 2,
    "quant_fp8_bf16": [_P] * 5 + [_L],
    "quant_fp8_rowwise_bf16": [_P] * 5 + [_I] * 2,
    "linear_wgrad_plan": [_I] * 4,
    # (stream, a, x, ws, dw, K, M, N, lda, ldx, slices)
    "linear_wgrad_bf16": [_P] * 5 + [_I] * 3 + [_L] * 2 + [_I],
    "scale_bf16_inplace": [_P] * 3 + [_L],
    # (stream, zimg, ztxt, row_thr, col_thr, row_cnt, col_cnt, b, n, d, diag)
    "pair_rank_counts_bf16": [_P] * 7 + [_I] * 4,
    "softmax_tile_dim": [],
    # (stream, zimg, ztxt, t', row_ws, col_ws, row_lse, col_lse, b, n, d)
    "softmax_lse_bf16": [_P] * 8 + [_I] * 3,
    # (stream, zimg, ztxt, t', row_lse, row_w, col_lse, col_w, g, gs_ws,
    #  b, n, d, ldg, diag)
    "softmax_g_bf16": [_P] * 10 + [_I] * 3 + [_L] + [_I],
    "pair_topk_max_k": [],
    "pair_topk_tile_dim": [],
    "pair_topk_capacity": [_I],
    # (stream, zimg, ztxt, ws_s, ws_c, out_s, out_c, b, n, d, diag, k,
    #  n_splits)
    "pair_topk_bf16": [_P] * 7 + [_I] * 6,
    "sigmoid_ids_tile_dim": [],
    # (stream, zimg, ztxt, t', bias, img_ids, txt_ids, g, ws, b, n, d, ldg,
    #  diag, mode)
    "sigmoid_ids_bf16": [_P] * 9 + [_I] * 3 + [_L] + [_I] * 2,
    "softmax_ids_tile_dim": [],
    # (stream, zimg, ztxt, t', img_ids, txt_ids, row_ws, col_ws, row_lse,
    #  row_pos, row_cnt, col_lse, col_pos, col_cnt, b, n, d, diag, mode)
    "softmax_ids_lse_bf16": [_P] * 14 + [_I] * 5,
    # (stream, zimg, ztxt, t', img_ids, txt_ids, row_lse, row_w, row_pw,
    #  col_lse, col_w, col_pw, g, gs_ws, b, n, d, ldg, diag, mode)
    "softmax_ids_g_bf16": [_P] * 14 + [_I] * 3 + [_L] + [_I] * 2,
}


def _load():
    global _lib, _lib_err
    if _lib is not None or _lib_err is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        _lib_err = (
            f"HIP extension not found at {SO_PATH}. Build it with: "
            "python -m distributed_sigmoid_loss_amd.ops.build")
        return None
    try:
        lib = ctypes.CDLL(SO_PATH)
    except OSError as e:  # pragma: no cover
        _lib_err = f"failed to load {SO_PATH}: {e}"
        return None
    # One staleness rule: a missing export, or another ABI number.
    why = next((f"no {name}" for name in _EXPORTS if not hasattr(lib, name)),
               None)
    if why is None:
        for name, argtypes in _EXPORTS.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = _I, argtypes
        if lib.siglip_ext_abi() != 13:
            why = f"ABI {lib.siglip_ext_abi()}, need 13"
    if why is not None:
        _lib_err = (f"stale HIP extension at {SO_PATH} ({why}); rebuild "
                    "with: python -m distributed_sigmoid_loss_amd.ops.build "
                    "--force")
        return None
    _lib = lib
    return _lib


def extension_available() -> bool:
    return _load() is not None


def _require_lib():
    lib = _load()
    if lib is None:
        raise RuntimeError(_lib_err)
    return lib


def _check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what} failed: hipError_t={rc}")


def _prep_scalar(p: torch.Tensor, device) -> torch.Tensor:
    t = p.detach().reshape(()).to(device=device, dtype=torch.float32)
    return t.contiguous()


def _go_scalar(grad_output: torch.Tensor, device,
               dtype=torch.float32) -> torch.Tensor:
    """A backward's upstream gradient as a 0-d ``dtype`` scalar on
    ``device``."""
    return grad_output.detach().reshape(()).to(device=device, dtype=dtype)


def _validate(zimg: torch.Tensor, ztxt: torch.Tensor, quant: str):
    if not zimg.is_cuda:
        raise RuntimeError("siglip HIP ops require GPU tensors")
    if zimg.dtype != torch.bfloat16 or ztxt.dtype != torch.bfloat16:
        raise RuntimeError(
            f"siglip HIP ops require bf16 embeddings (got {zimg.dtype}); "
            "cast with .bfloat16() or pass impl='torch'")
    if quant not in ("bf16", "fp8", "mixed"):
        raise ValueError(f"unknown quant {quant!r}")
    mult = 16 if quant == "fp8" else 8
    if zimg.shape[1] % mult != 0:
        raise RuntimeError(
            f"emb dim must be a multiple of {mult} for {quant} "
            f"(got {zimg.shape[1]})")


def _quant_fp8(x: torch.Tensor):
    """Per-tensor symmetric quantization to OCP e4m3 (max normal 448).

    Returns (q, scale): x ≈ q * scale.  The scale is folded into the
    temperature for the logit kernels (t_eff = t·s_img·s_txt), so the HIP
    side runs with unit MX block scales.  On GPU the fused two-pass HIP
    kernels run (amax + cast, no host sync — ~0.04 ms vs ~0.25 ms of stock
    kernels per pair at B=32k); elsewhere the torch composite.
    """
    if x.is_cuda and x.dtype == torch.bfloat16 and extension_available():
        lib = _require_lib()
        xd = x.detach().contiguous()
        q = torch.empty(xd.shape, device=xd.device,
                        dtype=torch.float8_e4m3fn)
        scale = torch.empty((), device=xd.device, dtype=torch.float32)
        amax_bits = torch.zeros(1, device=xd.device, dtype=torch.int32)
        stream = torch.cuda.current_stream(xd.device).cuda_stream
        _check(lib.quant_fp8_bf16(
            ctypes.c_void_p(stream), ctypes.c_void_p(xd.data_ptr()),
            ctypes.c_void_p(q.data_ptr()), ctypes.c_void_p(scale.data_ptr()),
            ctypes.c_void_p(amax_bits.data_ptr()),
            ctypes.c_longlong(xd.numel())), "quant_fp8")
        return q, scale
    amax = x.detach().abs().amax().float().clamp_(min=2.0 ** -20)
    scale = amax / 448.0
    q = (x.float() / scale).to(torch.float8_e4m3fn)
    return q, scale


def _quant_fp8_rowwise(x: torch.Tensor):
    """Per-ROW pow2 quantization for the hardware-scaled MX MFMA path.

    Returns (q, e8, ratio, s_ref): x_row ≈ q_row · 2^(e8_row−127);
    ratio_row = 2^(e8_row − e_max) ≤ 1 (the backward slab fold), and
    s_ref = 2^(e_max−127) (the per-tensor factor the GEMM scale carries).
    """
    lib = _require_lib()
    xd = x.detach().contiguous()
    b, d = xd.shape
    q = torch.empty((b, d), device=xd.device, dtype=torch.float8_e4m3fn)
    e8 = torch.empty(b, device=xd.device, dtype=torch.uint8)
    emax = torch.zeros(1, device=xd.device, dtype=torch.int32)
    stream = torch.cuda.current_stream(xd.device).cuda_stream
    _check(lib.quant_fp8_rowwise_bf16(
        ctypes.c_void_p(stream), ctypes.c_void_p(xd.data_ptr()),
        ctypes.c_void_p(q.data_ptr()), ctypes.c_void_p(e8.data_ptr()),
        ctypes.c_void_p(emax.data_ptr()), b, d), "quant_fp8_rowwise")
    emax_f = emax[0].float()
    ratio = torch.exp2(e8.float() - emax_f)
    s_ref = torch.exp2(emax_f - 127.0)
    return q, e8, ratio, s_ref


def rowwise_ok(b: int, n: int, d: int) -> bool:
    """Row-wise fp8 policy gate: needs the saved-g mm8-aligned shapes (the
    slab folds assume the fp8 GEMM path) and SIGLIP_FP8_ROWWISE=1.

    OFF by default: it costs ~14%% of fp8 step throughput (4.84 vs
    4.24 ms at B=32k — epilogue ratio folds + the row-wise quant pass)
    and the loss contract assumes unit-norm rows, where per-tensor scales
    lose nothing.  Turn it on for embeddings with per-row dynamic range
    beyond e4m3's ~2^18 (see test_rowwise_quant_keeps_per_row_precision)."""
    return (os.environ.get("SIGLIP_FP8_ROWWISE", "0") == "1"
            and _mm8_ok(b, d, n))


@dataclasses.dataclass(frozen=True, eq=False)
class QuantCache:
    """One quantization of an (image, text) embedding pair, made once and
    shared by forward and backward (``qcache=``).  Two policies:

    - per-tensor: ``x ≈ q · s`` with fp32 scalars ``si`` / ``st``;
    - row-wise (``rowwise``): per-row e8m0 exponents ``*_e8`` for the MX
      MFMA's hardware dequant, per-row ``*_ratio`` for the slab folds, and
      the tensor-max factors ``si_ref`` / ``st_ref`` the GEMM scale carries.
    """
    zi_q: torch.Tensor
    zt_q: torch.Tensor
    si: Optional[torch.Tensor] = None
    st: Optional[torch.Tensor] = None
    zi_e8: Optional[torch.Tensor] = None
    zt_e8: Optional[torch.Tensor] = None
    zi_ratio: Optional[torch.Tensor] = None
    zt_ratio: Optional[torch.Tensor] = None
    si_ref: Optional[torch.Tensor] = None
    st_ref: Optional[torch.Tensor] = None

    @property
    def rowwise(self) -> bool:
        return self.zi_e8 is not None

    @property
    def gemm_scales(self):
        """(image, text) per-tensor factors the fp8 gradient GEMMs carry."""
        return (self.si_ref, self.st_ref) if self.rowwise else (self.si,
                                                                self.st)

    def tensors(self) -> tuple:
        """The populated fields, in field order (``save_for_backward``)."""
        ts = (getattr(self, f.name) for f in dataclasses.fields(self))
        return tuple(t for t in ts if t is not None)

    @classmethod
    def from_tensors(cls, ts) -> "QuantCache":
        """Inverse of :meth:`tensors`: 4 tensors are a per-tensor cache, 8 a
        row-wise one."""
        ts = tuple(ts)
        if len(ts) == 4:
            return cls(*ts)
        if len(ts) == 8:
            return cls(ts[0], ts[1], None, None, *ts[2:])
        raise ValueError(f"QuantCache takes 4 or 8 tensors, got {len(ts)}")

    def text_rows(self, j0: int, j1: int) -> "QuantCache":
        """The same (per-tensor) cache restricted to text rows j0:j1."""
        return dataclasses.replace(self, zt_q=self.zt_q[j0:j1])


def quantize_fp8_rowwise_pair(zimg: torch.Tensor,
                              ztxt: torch.Tensor) -> QuantCache:
    zi_q, zi_e8, zi_ratio, si_ref = _quant_fp8_rowwise(zimg)
    zt_q, zt_e8, zt_ratio, st_ref = _quant_fp8_rowwise(ztxt)
    return QuantCache(zi_q, zt_q, zi_e8=zi_e8, zt_e8=zt_e8,
                      zi_ratio=zi_ratio, zt_ratio=zt_ratio,
                      si_ref=si_ref, st_ref=st_ref)


def quantize_fp8_pair(zimg: torch.Tensor, ztxt: torch.Tensor) -> QuantCache:
    """Quantize both embedding tensors once; pass the result as ``qcache`` to
    both :func:`siglip_fwd` and :func:`siglip_bwd` so an fwd+bwd step pays a
    single quantization pass."""
    zi_q, si = _quant_fp8(zimg)
    zt_q, st = _quant_fp8(ztxt)
    return QuantCache(zi_q, zt_q, si, st)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _launch_tile(mode: int, quant: str, zi: torch.Tensor, zt: torch.Tensor,
                 tp: torch.Tensor, bp: torch.Tensor, out: torch.Tensor,
                 g: Optional[torch.Tensor] = None,
                 gt: Optional[torch.Tensor] = None,
                 diag_offset: Optional[int] = None, rowscales=None,
                 default_gm: str = "4"):
    """The one call into ``lib.siglip_tile``.  ``zi``/``zt`` are the operands
    the kernel reads (bf16, or e4m3 for fp8 logits — their element size is
    ``eb``).  ``g`` ``(b, n)`` / ``gt`` ``(n, b)`` are the output slabs
    (``quant`` picks their element size ``eb_g``); they may be column / row
    VIEWS into a wider slab — the view carries the column offset and its
    row stride is the kernel's ``ldg`` — so torch's slicing, not pointer
    arithmetic here, keeps a chunk inside its slab.  ``rowscales`` is the
    row-wise policy's (a_e8, b_e8, a_rat, b_rat)."""
    lib = _require_lib()
    b, d = zi.shape
    n = zt.shape[0]
    eb_g = 1 if quant in ("fp8", "mixed") else 2
    ldg = n
    if g is not None:
        ldg = g.stride(0)
        if (g.shape != (b, n) or g.stride(1) != 1 or g.element_size() != eb_g
                or (gt is not None and (gt.shape != (n, b)
                                        or not gt.is_contiguous()))):
            raise RuntimeError("g/gt slab layout does not match the block")
        if b * ldg * eb_g >= 2 ** 32:
            raise RuntimeError(
                "g slab exceeds the kernel's 32-bit addressing; use the "
                "recompute path (save_g_enabled would have said no)")
    a_e8, b_e8, a_rat, b_rat = rowscales or (None,) * 4
    stream = torch.cuda.current_stream(zi.device).cuda_stream
    _check(lib.siglip_tile(
        ctypes.c_void_p(stream), mode, zi.element_size(), eb_g,
        _ptr(zi), _ptr(zt), _ptr(tp), _ptr(bp), _ptr(out), _ptr(g), _ptr(gt),
        _ptr(a_e8), _ptr(b_e8), _ptr(a_rat), _ptr(b_rat),
        b, n, d, ldg,
        _DIAG_NONE if diag_offset is None else int(diag_offset),
        _kernel_flags(default_gm)), f"siglip_tile(mode={mode}, {quant})")


def _logit_operands(quant, zimg, ztxt, tp, qcache):
    """What the tile kernel reads for ``quant``: (zi, zt, tp, rowscales).
    fp8 logits read the quantized pair; per-tensor scales are folded into
    the temperature (t_eff = t·s_img·s_txt), row-wise scales go to the MFMA
    as e8m0 bytes and tp stays unmodified (acc is the true dot)."""
    if quant != "fp8":
        return zimg, ztxt, tp, None
    qc = qcache if qcache is not None else quantize_fp8_pair(zimg, ztxt)
    if qc.rowwise:
        return qc.zi_q, qc.zt_q, tp, (qc.zi_e8, qc.zt_e8,
                                      qc.zi_ratio, qc.zt_ratio)
    return qc.zi_q, qc.zt_q, tp + qc.si.log() + qc.st.log(), None


def siglip_fwd(zimg: torch.Tensor, ztxt: torch.Tensor, t_prime: torch.Tensor,
               bias: torch.Tensor, diag_offset: Optional[int],
               quant: str = "bf16", qcache=None) -> torch.Tensor:
    _validate(zimg, ztxt, quant)
    if quant == "mixed":
        quant = "bf16"   # mixed = bf16 logits; fp8 applies to backward only
    dev = zimg.device
    zi_k, zt_k, tp_k, rowscales = _logit_operands(
        quant, zimg, ztxt, _prep_scalar(t_prime, dev), qcache)
    buf = _out_buf(dev)
    _launch_tile(0, quant, zi_k, zt_k, tp_k, _prep_scalar(bias, dev), buf,
                 diag_offset=diag_offset, rowscales=rowscales,
                 default_gm="8")
    return buf[:, 0].sum()


def siglip_bwd(zimg: torch.Tensor, ztxt: torch.Tensor, t_prime: torch.Tensor,
               bias: torch.Tensor, diag_offset: Optional[int],
               grad_output: torch.Tensor, col_chunk: Optional[int],
               quant: str = "bf16", on_dztxt=None, qcache=None):
    """Returns (dzimg, dztxt, dt_prime, dbias).

    Per column slab: the fused kernel recomputes logit tiles (MFMA) and
    writes g = dL/d(logit pre-scale); then dzimg += g @ ztxt_slab and
    dztxt_slab = gᵀ @ zimg on the GEMM libraries (bf16 rocBLAS, or fp8
    hipBLASLt when the policy provides e4m3 slabs).  ``on_dztxt(dztxt)`` is
    invoked as soon as the text gradient exists so distributed callers can
    overlap their reduce-scatter with the remaining image-gradient GEMM.
    """
    _validate(zimg, ztxt, quant)
    b, d = zimg.shape
    n = ztxt.shape[0]
    dev = zimg.device
    tp = _prep_scalar(t_prime, dev)
    bp = _prep_scalar(bias, dev)
    fp8g = quant in ("fp8", "mixed")   # g slabs are e4m3 (×448), plus gᵀ
    qc = None
    if fp8g:
        # Reuse the forward's quantization when provided (identical inputs
        # give identical amax, so recomputing is equivalent but wasteful).
        # fp8 logits read it through t_eff so they match the forward's;
        # mixed recomputes bf16 logits and quantizes for the GEMMs only.
        # (The recompute path is per-tensor only — row-wise caches ride the
        # saved-g path, siglip_bwd_from_g.)
        if qcache is not None and qcache.rowwise:
            raise RuntimeError(
                "row-wise fp8 qcache requires the saved-g backward")
        if b % 4 != 0:   # packed gt stores need b%4
            raise RuntimeError(f"{quant} backward requires batch % 4 == 0")
        qc = qcache if qcache is not None else quantize_fp8_pair(zimg, ztxt)
    zi_k, zt_k, tp_k, _ = _logit_operands(quant, zimg, ztxt, tp, qc)
    scal = _out_buf(dev)

    # Column slab sizing: the kernel's g-store addressing is 32-bit, so
    # b * slab * esz bytes must stay below 2^32; beyond that (and to bound
    # workspace at huge n) we chunk.
    g_esz = 1 if fp8g else 2
    g_dtype = torch.float8_e4m3fn if fp8g else torch.bfloat16
    step = col_chunk if col_chunk and col_chunk > 0 else n
    while step > 256 and (b * step * g_esz) >= 2 ** 32:
        step //= 2
    # Floor of 256 columns per slab: below that the kernel grid degenerates.
    # The 32-bit invariant must survive the floor — at bf16 that means
    # b < 2^32/(256·2) = 8.4M rows, far beyond any real shard.
    step = max(step, 256)
    if (b * step * g_esz) >= 2 ** 32:
        raise RuntimeError(
            f"batch {b} too large for the 32-bit g-slab addressing even at "
            f"the 256-column slab floor; shard the batch")

    def emit(j0, j1, diag_j, g, gt):
        _launch_tile(1, quant, zi_k, zt_k[j0:j1], tp_k, bp, scal, g=g, gt=gt,
                     diag_offset=diag_j)

    go = _go_scalar(grad_output, dev)
    # bf16_scale=False: the recompute path multiplies by the fp32 scale,
    # then casts.
    dzimg, dztxt = band_grad_gemms(
        zimg, ztxt, step, emit, go * tp.exp(), diag_offset=diag_offset,
        g_dtype=g_dtype, with_gt=fp8g, qc=qc, on_dztxt=on_dztxt,
        bf16_scale=False)
    # t_eff ≡ t for bf16/mixed; for fp8 the kernel's dot is of quantized rows.
    dt_prime, dbias = scalar_grads(reduce_out3(scal), go, tp_k.exp(),
                                   t_prime, bias)
    return dzimg, dztxt, dt_prime, dbias


# ---------------------------------------------------------------------------
# fwd+g ("saved-g") path: one kernel emits loss + g slab + scalar partials,
# so backward is pure GEMMs — the training step never computes the logits
# GEMM twice.  Used whenever the slab fits comfortably in HBM (it is 2 GiB
# at the B=32k bf16 headline config, against 288 GB); the recompute kernels
# above remain for the chunked huge-batch path (BASELINE config 3).
# ---------------------------------------------------------------------------


def save_g_enabled(b: int, n: int, quant: str) -> bool:
    """Policy: is the fwd+g saved-slab path usable/worth it for this block?

    SIGLIP_SAVE_G = auto (default) | 0 (always recompute) | 1 (force when
    addressable); SIGLIP_SAVE_G_MAX_BYTES bounds the slab workspace in auto
    mode (default 6 GiB — g plus, for fp8/mixed, its transpose).
    """
    env = os.environ.get("SIGLIP_SAVE_G", "auto")
    if env == "0":
        return False
    esz = 1 if quant in ("fp8", "mixed") else 2
    if b * n * esz >= 2 ** 32:        # kernel's 32-bit slab addressing
        return False
    if env == "1":
        return True
    need = b * n * esz * (2 if esz == 1 else 1)
    cap = int(os.environ.get("SIGLIP_SAVE_G_MAX_BYTES", str(6 * 2 ** 30)))
    return need <= cap


def save_g_banded_enabled(b: int, n: int, quant: str) -> bool:
    """Column-banded saved-g policy: when ONE slab exceeds the kernel's
    32-bit addressing but the full (b, n) g fits HBM comfortably (it is
    32 GB at 131k², against 288 GB), forward emits g in column bands and
    backward is still pure GEMMs — no logits recompute.  bf16 only (the
    fp8 slabs come in pairs and ride the single-slab path);
    SIGLIP_SAVE_G_BANDED=0 disables, SIGLIP_SAVE_G=0 disables all saving."""
    if quant != "bf16":
        return False
    if os.environ.get("SIGLIP_SAVE_G", "auto") == "0":
        return False
    if os.environ.get("SIGLIP_SAVE_G_BANDED", "auto") == "0":
        return False
    if not torch.cuda.is_available():
        return False
    total = b * n * 2
    try:
        free, _ = torch.cuda.mem_get_info()
    except Exception:  # pragma: no cover
        return False
    return total <= free * 0.5


def banded_col_step(b: int, esz: int = 2) -> int:
    """Widest 256-aligned column band whose slab stays under the kernel's
    32-bit store addressing (SIGLIP_BANDED_STEP overrides, for tests)."""
    env = os.environ.get("SIGLIP_BANDED_STEP")
    if env:
        return max(256, int(env))
    step = (2 ** 32 - 1) // (b * esz)
    return max(256, (step // 256) * 256)


def g_band_step(b: int, n: int, col_chunk: Optional[int]) -> int:
    """Columns per bf16 g band of a recompute backward: ``n`` — the whole
    block as one slab — without a ``col_chunk`` while that slab stays under
    the kernels' 32-bit addressing, else ``col_chunk`` or
    :func:`banded_col_step`."""
    if col_chunk is None and b * n * 2 < 2 ** 32:
        return n
    return int(col_chunk) if col_chunk else banded_col_step(b)


def col_bands(n: int, step: int, diag_offset: Optional[int] = None):
    """``(j0, j1, diag_j)`` of the column bands ``j0:j1`` of ``n`` columns,
    ``step`` wide but for a ragged last one; ``diag_j`` is ``diag_offset`` as
    the band's own columns see it (``None`` stays ``None``)."""
    for j0 in range(0, n, step):
        yield (j0, min(j0 + step, n),
               None if diag_offset is None else int(diag_offset) - j0)


def scaled_mm8(a8: torch.Tensor, b8_rowmajor: torch.Tensor,
               scale: torch.Tensor) -> torch.Tensor:
    """fp8 GEMM a8 (m, k) @ b8 (k, d) → bf16 via hipBLASLt
    (``torch._scaled_mm``; mat2 re-laid column-major as it requires — k is at
    most a few thousand rows, a cheap copy)."""
    one = torch.ones((), device=a8.device)
    b_cm = b8_rowmajor.t().contiguous().t()
    return torch._scaled_mm(a8, b_cm, scale_a=scale.reshape(()), scale_b=one,
                            out_dtype=torch.bfloat16)


def _mm8_ok(b: int, d: int, *cols: int) -> bool:
    """Can the fp8 gradient GEMMs run on hipBLASLt (measured 2.6× the bf16
    matmul)?  Every GEMM dimension must be 16-aligned; otherwise the e4m3
    slabs are dequantized and rocBLAS runs in bf16."""
    return (all(x % 16 == 0 for x in (b, d) + cols)
            and hasattr(torch, "_scaled_mm"))


def _scale_inplace_ok(x: torch.Tensor) -> bool:
    return (x.is_cuda and x.dtype == torch.bfloat16 and x.is_contiguous()
            and x.data_ptr() % 16 == 0 and extension_available())


def scale_bf16_(x: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """In-place ``x *= scale.to(bf16)`` for a contiguous bf16 GPU tensor and a
    0-d device scalar, by the vectorized HIP kernel (16-byte accesses; fp32
    product of the element and the bf16-rounded scale, rounded to
    nearest-even — bitwise what ``x * scale.to(torch.bfloat16)`` gives).
    Returns ``x``."""
    lib = _require_lib()
    if not (x.is_cuda and x.dtype == torch.bfloat16 and x.is_contiguous()):
        raise RuntimeError("scale_bf16_ needs a contiguous bf16 GPU tensor")
    s = scale.detach().reshape(()).to(device=x.device, dtype=torch.float32)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    _check(lib.scale_bf16_inplace(
        ctypes.c_void_p(stream), ctypes.c_void_p(x.data_ptr()),
        ctypes.c_void_p(s.data_ptr()), ctypes.c_longlong(x.numel())),
        "scale_bf16_inplace")
    return x


def _rows_16b(t: torch.Tensor) -> torch.Tensor:
    """``t`` itself when the wgrad kernel can read it in place (unit column
    stride, 16-byte-aligned rows), otherwise its contiguous copy."""
    if (t.stride(1) == 1 and t.stride(0) >= t.shape[1]
            and t.stride(0) % 8 == 0 and t.data_ptr() % 16 == 0):
        return t
    return t.contiguous()


def _wgrad_slices(k: int, m: int, n: int, device) -> int:
    """K-slice count for the split-K weight-gradient kernel (0: unsupported
    dims).  SIGLIP_WGRAD_SLICES overrides the plan, for sweeps."""
    n_cu = torch.cuda.get_device_properties(device).multi_processor_count
    s = _require_lib().linear_wgrad_plan(k, m, n, n_cu)
    env = os.environ.get("SIGLIP_WGRAD_SLICES")
    return int(env) if s and env else s


def linear_wgrad_supported(dy: torch.Tensor, x: torch.Tensor) -> bool:
    """Does the native split-K kernel take this ``dyᵀ @ x``?  GPU, bf16, 2-D,
    a shared non-empty batch, and M, N multiples of 8 (its 16-byte loads)."""
    return (dy.is_cuda and x.is_cuda and dy.dtype == torch.bfloat16
            and x.dtype == torch.bfloat16 and dy.dim() == 2 and x.dim() == 2
            and dy.shape[0] == x.shape[0] and dy.shape[0] > 0
            and dy.shape[1] > 0 and x.shape[1] > 0
            and dy.shape[1] % 8 == 0 and x.shape[1] % 8 == 0
            and extension_available())


def linear_wgrad(dy: torch.Tensor, x: torch.Tensor,
                 slices: Optional[int] = None) -> torch.Tensor:
    """Weight gradient of a bias-free linear layer: ``dW (M, N) = dyᵀ @ x``
    for ``dy`` (B, M) and ``x`` (B, N).

    bf16 GPU operands run the split-K HIP kernel: (output tiles) × (K slices)
    workgroups fill the chip where the library's output-tiled GEMM occupies
    24 of 256 CUs at 768×768; slices leave fp32 partials in a workspace from
    the torch allocator and a second kernel sums them in slice order — no
    atomics, bitwise reproducible.  ``dy`` / ``x`` may be row-strided views.
    Dims the kernel does not take fall back to the library matmul."""
    if not linear_wgrad_supported(dy, x):
        if dy.is_cuda and dy.dtype == torch.bfloat16:
            _require_lib()      # a missing extension is an error, not a path
        return dy.t() @ x
    lib = _require_lib()
    dy, x = _rows_16b(dy.detach()), _rows_16b(x.detach())
    k, m = dy.shape
    n = x.shape[1]
    if slices is None:
        slices = _wgrad_slices(k, m, n, dy.device)
    dw = torch.empty((m, n), device=dy.device, dtype=torch.bfloat16)
    ws = torch.empty((max(slices, 1), m, n), device=dy.device,
                     dtype=torch.float32)
    stream = torch.cuda.current_stream(dy.device).cuda_stream
    _check(lib.linear_wgrad_bf16(
        ctypes.c_void_p(stream), ctypes.c_void_p(dy.data_ptr()),
        ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(ws.data_ptr()),
        ctypes.c_void_p(dw.data_ptr()), k, m, n, dy.stride(0), x.stride(0),
        slices), "linear_wgrad_bf16")
    return dw


def native_wgrad_enabled() -> bool:
    """SIGLIP_NATIVE_WGRAD=0 sends the towers' weight gradient back to the
    library GEMM (A/B runs); default on."""
    return os.environ.get("SIGLIP_NATIVE_WGRAD", "1") != "0"


class _LinearNativeWgrad(torch.autograd.Function):
    """Bias-free ``x @ Wᵀ`` whose weight gradient comes from
    :func:`linear_wgrad`.  Forward and the input gradient (computed only when
    asked for) stay on the library."""

    @staticmethod
    def forward(ctx, x, weight):
        ctx.save_for_backward(x, weight)
        return x @ weight.t()

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dx = dy @ weight if ctx.needs_input_grad[0] else None
        dw = linear_wgrad(dy, x) if ctx.needs_input_grad[1] else None
        return dx, dw


def linear_nobias(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """``x @ weightᵀ``.  2-D bf16 GPU inputs with supported dims (and
    SIGLIP_NATIVE_WGRAD unset or 1) take :class:`_LinearNativeWgrad`;
    everything else is ``F.linear``."""
    if (native_wgrad_enabled() and x.dim() == 2 and weight.dim() == 2
            and x.is_cuda and weight.is_cuda
            and x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16
            and x.shape[0] > 0 and weight.shape[0] % 8 == 0
            and weight.shape[1] % 8 == 0 and extension_available()):
        return _LinearNativeWgrad.apply(x, weight)
    import torch.nn.functional as F
    return F.linear(x, weight)


class GBand(NamedTuple):
    """One column band of dL/dlogit for :func:`grad_gemms`: the ``(b, c)``
    slab (bf16, or e4m3 ×448), its ``(c, b)`` transpose (e4m3 only), the
    ``c`` text rows it covers and the quantization of those rows."""
    g: torch.Tensor
    gt: Optional[torch.Tensor]
    zt: torch.Tensor
    qc: Optional[QuantCache] = None


def grad_gemms(bands, zimg: torch.Tensor, n: int, scale: torch.Tensor,
               on_dztxt=None, gt_full: Optional[torch.Tensor] = None,
               bf16_scale: bool = False):
    """The two gradient GEMMs of every backward regime → ``(dzimg, dztxt)``:
    ``dztxt = scale·gᵀ@zimg`` FIRST, then ``on_dztxt(dztxt)`` (a distributed
    caller's async reduce-scatter overlaps what follows), then
    ``dzimg = scale·g@ztxt``.

    ``bands`` is one :class:`GBand` covering all ``n`` text rows, or an
    iterable of them in row order; an iterable may be lazy (each band is
    consumed before the next is requested) and accumulates dzimg in fp32.
    ``gt_full`` is the whole ``(n, b)`` e4m3 transpose when the image side
    has one scale for all bands (the fp8 ring): dztxt is then one GEMM.

    e4m3 slabs carry a fixed ×448; with the operands' per-tensor scales it
    is folded into ``_scaled_mm``'s scale argument, so no elementwise pass
    runs.  Unaligned shapes dequantize and use the bf16 matmul.

    ``bf16_scale``: multiply bf16 products that STAY bf16 by the scale
    rounded to bf16 (the saved-g paths: a fp32 0-d multiplier would promote
    the whole product to fp32 — two extra full-tensor passes — and the
    ~0.4% rounding is below the bf16 grad noise floor).  False (the
    recompute path) multiplies by the fp32 scale and then casts.  Products
    headed for the fp32 accumulator, and dequantized e4m3 slabs, always
    take the fp32 scale.
    """
    b, d = zimg.shape
    single = isinstance(bands, GBand)
    s8 = scale / 448.0

    def gemm(g, transpose, g8, other, other_q, s_q, c, keep_bf16):
        """scale · op(g) @ other for a slab of ``c`` logit columns; ``g8`` is
        op(g) as a row-major e4m3 tensor when the policy provides one."""
        if g8 is not None and _mm8_ok(b, d, n, c):
            return scaled_mm8(g8, other_q, s8 * s_q)
        s = scale
        if g8 is not None:
            g = g.to(torch.bfloat16) * (1.0 / 448.0)
        elif bf16_scale and keep_bf16:
            out = (g.T if transpose else g) @ other
            if _scale_inplace_ok(out):
                # The product is fresh, so scale it in place: one vectorized
                # pass, bit-identical to ``out * scale.to(bf16)``.
                return scale_bf16_(out, scale)
            return out * scale.to(g.dtype)
        return ((g.T if transpose else g) @ other) * s

    def dztxt_of(band):
        qc, c = band.qc, band.zt.shape[0]
        return gemm(band.g, True, band.gt, zimg, qc and qc.zi_q,
                    qc and qc.gemm_scales[0], c, True)

    def dzimg_of(band):
        qc, c = band.qc, band.zt.shape[0]
        g8 = band.g if band.g.dtype == torch.float8_e4m3fn else None
        return gemm(band.g, False, g8, band.zt, qc and qc.zt_q,
                    qc and qc.gemm_scales[1], c, single)

    if single:
        dztxt = dztxt_of(bands).to(zimg.dtype)
        if on_dztxt is not None:
            on_dztxt(dztxt)
        return dzimg_of(bands).to(zimg.dtype), dztxt

    dzimg_acc = torch.zeros((b, d), device=zimg.device, dtype=torch.float32)
    if gt_full is not None:
        bands = list(bands)
        qc = bands[0].qc
        dztxt = gemm(gt_full, False, gt_full, zimg, qc.zi_q,
                     qc.gemm_scales[0], n, True).to(zimg.dtype)
        if on_dztxt is not None:
            on_dztxt(dztxt)
    else:
        dztxt = torch.empty((n, d), device=zimg.device, dtype=zimg.dtype)
    j0 = 0
    for band in bands:
        j1 = j0 + band.zt.shape[0]
        if gt_full is None:
            dztxt[j0:j1] = dztxt_of(band)
        dzimg_acc += dzimg_of(band).float()
        j0 = j1
    if gt_full is None and on_dztxt is not None:
        on_dztxt(dztxt)
    return dzimg_acc.to(zimg.dtype), dztxt


def band_grad_gemms(zimg: torch.Tensor, ztxt: torch.Tensor, step: int, emit,
                    scale: torch.Tensor, *, diag_offset: Optional[int] = None,
                    g_dtype=torch.bfloat16, with_gt: bool = False,
                    qc: Optional[QuantCache] = None, on_dztxt=None,
                    bf16_scale: bool = False):
    """The column-banded recompute backward → ``(dzimg, dztxt)``: per band of
    ``step`` columns, ``emit(j0, j1, diag_j, g, gt)`` writes dL/dlogit of
    columns ``j0:j1`` into the ``(b, j1 − j0)`` slab ``g`` (and its transpose
    into ``gt``, given ``with_gt``; ``None`` otherwise), and
    :func:`grad_gemms` runs the band's two GEMMs (``scale``, ``on_dztxt``,
    ``bf16_scale`` are its).  ``diag_j`` is ``diag_offset`` shifted to the
    band, ``qc`` the per-tensor quantization whose text rows go with each
    band.  ``step >= n`` is one band: a single :class:`GBand`, no fp32
    accumulator."""
    b, n = zimg.shape[0], ztxt.shape[0]
    step = min(step, n)

    def slabs(c):
        return (torch.empty((b, c), device=zimg.device, dtype=g_dtype),
                torch.empty((c, b), device=zimg.device, dtype=g_dtype)
                if with_gt else None)

    def bands():
        # One reused slab (pair): grad_gemms consumes each band before it
        # asks for the next, so the stream orders the kernel of band k+1
        # after the GEMMs of band k.  This generator must stay lazy — a list
        # of its bands would all alias the one slab.  A ragged last band gets
        # a slab of its own width.
        bufs = slabs(step)
        for j0, j1, diag_j in col_bands(n, step, diag_offset):
            g, gt = bufs if j1 - j0 == step else slabs(j1 - j0)
            emit(j0, j1, diag_j, g, gt)
            yield GBand(g, gt, ztxt[j0:j1], qc and qc.text_rows(j0, j1))

    return grad_gemms(next(bands()) if step == n else bands(), zimg, n, scale,
                      on_dztxt=on_dztxt, bf16_scale=bf16_scale)


def scalar_grads(out3: torch.Tensor, go: torch.Tensor, t_eff: torch.Tensor,
                 t_prime: torch.Tensor, bias: torch.Tensor):
    """``(dt_prime, dbias)`` from a reduced ``[loss, Σg·dot, Σg]``:
    dt' = go·t_eff·Σg·dot (chain rule through t = e^{t'}; t_eff carries the
    per-tensor scales when the kernel's dot is of quantized rows),
    dbias = go·Σg."""
    return ((out3[1] * go * t_eff).to(t_prime.dtype).reshape(t_prime.shape),
            (out3[2] * go).to(bias.dtype).reshape(bias.shape))


def siglip_fwd_g(zimg: torch.Tensor, ztxt: torch.Tensor,
                 t_prime: torch.Tensor, bias: torch.Tensor,
                 diag_offset: Optional[int], quant: str = "bf16",
                 qcache=None, g_slab: Optional[torch.Tensor] = None,
                 gt_slab: Optional[torch.Tensor] = None, col0: int = 0,
                 out3: Optional[torch.Tensor] = None):
    """Fused forward that also emits the g slab and both scalar partials.

    Returns ``(out3, g_slab, gt_slab)`` where ``out3`` is the RAW (8, 32)
    per-XCD scalar buffer (atomically accumulated — pass the same buffer
    across chunk calls to sum them; reduce with :func:`reduce_out3` →
    ``[loss, Σ g·dot, Σ g]``), ``g_slab`` is the ``(b, n)`` dL/dlogit
    slab (bf16, or e4m3 ×448 for fp8/mixed along with its ``(n, b)``
    transpose ``gt_slab``).  When ``g_slab`` is supplied the chunk is written
    at column offset ``col0`` with the slab's width as row stride — the ring
    strategy assembles one ``(b, W·b)`` slab chunk by chunk.
    """
    _validate(zimg, ztxt, quant)
    b, n = zimg.shape[0], ztxt.shape[0]
    dev = zimg.device
    fp8g = quant in ("fp8", "mixed")
    if fp8g and b % 4 != 0:
        raise RuntimeError(f"{quant} fwd+g requires batch % 4 == 0")
    g_dtype = torch.float8_e4m3fn if fp8g else torch.bfloat16
    # A supplied slab takes this chunk at columns (gᵀ: rows) col0:col0+n; a
    # slab allocated here holds the chunk alone, whatever col0 says about
    # the other one.
    if g_slab is None:
        g_slab = g = torch.empty((b, n), device=dev, dtype=g_dtype)
    else:
        g = g_slab[:, col0:col0 + n]
    gt = None
    if fp8g and gt_slab is None:
        gt_slab = gt = torch.empty((n, b), device=dev, dtype=g_dtype)
    elif fp8g:
        gt = gt_slab[col0:col0 + n]
    if out3 is None:
        out3 = _out_buf(dev)
    zi_k, zt_k, tp_k, rowscales = _logit_operands(
        quant, zimg, ztxt, _prep_scalar(t_prime, dev), qcache)
    _launch_tile(2, quant, zi_k, zt_k, tp_k, _prep_scalar(bias, dev), out3,
                 g=g, gt=gt, diag_offset=diag_offset, rowscales=rowscales)
    return out3, g_slab, gt_slab if fp8g else None


def _pair_block(what: str, zimg: torch.Tensor, ztxt: torch.Tensor):
    """Validate the embeddings of a pair-grid op ``what``; returns the
    contiguous detached pair and ``(b, n, d, device)``."""
    if zimg.dim() != 2 or ztxt.dim() != 2 or zimg.shape[1] != ztxt.shape[1]:
        raise RuntimeError(
            f"expected (b, d) and (n, d) embeddings, got "
            f"{tuple(zimg.shape)} and {tuple(ztxt.shape)}")
    _validate(zimg, ztxt, "bf16")
    if ztxt.device != zimg.device:
        raise RuntimeError("zimg and ztxt must be on the same device")
    b, d = zimg.shape
    n = ztxt.shape[0]
    if b < 1 or n < 1:
        raise RuntimeError(f"{what} needs a non-empty block")
    return (zimg.detach().contiguous(), ztxt.detach().contiguous(), b, n, d,
            zimg.device)


def _diag_arg(diag_offset: Optional[int]) -> int:
    """``diag_offset`` as the kernels' int32 argument."""
    if diag_offset is None:
        return _DIAG_NONE
    diag = int(diag_offset)
    # No positive can lie inside an int32 block.
    return diag if -(2 ** 31) < diag < 2 ** 31 else _DIAG_NONE


def _g_view(g: Optional[torch.Tensor], b: int, n: int, device):
    """The dL/dlogit slab of a ``(b, n)`` block, allocated here or the
    caller's view after validation; returns ``(g, ldg)``."""
    if g is None:
        g = torch.empty((b, n), device=device, dtype=torch.bfloat16)
    elif (g.device != device or g.dtype != torch.bfloat16
          or g.shape != (b, n) or g.stride(1) != 1
          or (b > 1 and g.stride(0) < n)):
        raise RuntimeError(
            f"g must be a bf16 ({b}, {n}) view with unit column stride on "
            f"{device} (got {g.dtype} {tuple(g.shape)}, strides "
            f"{tuple(g.stride())} on {g.device})")
    return g, max(g.stride(0), n)


def _vec_ok(v, dtype, length: int, device) -> bool:
    """A contiguous ``dtype`` ``(length,)`` tensor on ``device``?"""
    return (isinstance(v, torch.Tensor) and v.device == device
            and v.dtype == dtype and v.shape == (length,)
            and v.is_contiguous())


def _rank_side(name: str, thr, cnt, length: int, device):
    """Validate one side (rows or columns) of :func:`pair_rank_counts`;
    returns ``(thr, cnt)`` with ``cnt`` allocated if needed, or
    ``(None, None)`` for a skipped side."""
    if thr is None:
        if cnt is not None:
            raise RuntimeError(f"{name}_cnt given without {name}_thr")
        return None, None
    if not _vec_ok(thr, torch.float32, length, device):
        raise RuntimeError(
            f"{name}_thr must be a contiguous fp32 ({length},) tensor on "
            f"{device} (got {thr.dtype} {tuple(thr.shape)} on {thr.device})")
    if cnt is None:
        cnt = torch.zeros(length, device=device, dtype=torch.int32)
    elif not _vec_ok(cnt, torch.int32, length, device):
        raise RuntimeError(
            f"{name}_cnt must be a contiguous int32 ({length},) tensor on "
            f"{device} (got {cnt.dtype} {tuple(cnt.shape)} on {cnt.device})")
    return thr, cnt


def pair_rank_counts(zimg: torch.Tensor, ztxt: torch.Tensor,
                     row_thr: Optional[torch.Tensor] = None,
                     col_thr: Optional[torch.Tensor] = None,
                     diag_offset: Optional[int] = None,
                     row_cnt: Optional[torch.Tensor] = None,
                     col_cnt: Optional[torch.Tensor] = None):
    """Threshold counts over the ``(b, n)`` score grid ``s = zimg @ ztxtᵀ``
    without materializing it → ``(row_cnt | None, col_cnt | None)``:

    ``row_cnt[i] += #{j ≠ i + diag_offset : s_ij > row_thr[i]}`` and
    ``col_cnt[j] += #{i ≠ j − diag_offset : s_ij > col_thr[j]}`` (strict
    ``>``; ``diag_offset=None``: nothing is excluded).  Thresholds are fp32
    ``(b,)`` / ``(n,)``; a side without a threshold is skipped and returned
    as ``None``.  Counts are int32 and ADDED into ``row_cnt`` / ``col_cnt``
    when given (the caller zeroes them), so column chunks (``ztxt[j0:j1]``
    with ``diag_offset − j0``) and repeated calls accumulate; otherwise they
    start from zeros allocated here.  Integer atomics only: the result is
    bitwise reproducible.  No autograd."""
    zi, zt, b, n, d, dev = _pair_block("pair_rank_counts", zimg, ztxt)
    lib = _require_lib()
    row_thr, row_cnt = _rank_side("row", row_thr, row_cnt, b, dev)
    col_thr, col_cnt = _rank_side("col", col_thr, col_cnt, n, dev)
    if row_thr is None and col_thr is None:
        return None, None
    stream = torch.cuda.current_stream(dev).cuda_stream
    _check(lib.pair_rank_counts_bf16(
        ctypes.c_void_p(stream), _ptr(zi), _ptr(zt), _ptr(row_thr),
        _ptr(col_thr), _ptr(row_cnt), _ptr(col_cnt), b, n, d,
        _diag_arg(diag_offset)),
        "pair_rank_counts_bf16")
    return row_cnt, col_cnt


def pair_topk_max_k() -> int:
    """Largest ``k`` :func:`pair_topk` serves."""
    return _require_lib().pair_topk_max_k()


def pair_topk(zimg: torch.Tensor, ztxt: torch.Tensor, k: int,
              diag_offset: Optional[int] = None,
              n_splits: Optional[int] = None):
    """The ``k`` best scoring columns of every row of the ``(b, n)`` score
    grid ``s = zimg @ ztxtᵀ`` without materializing it →
    ``(scores (b, k) fp32, columns (b, k) int32)``.

    The candidates of row ``i`` are the columns ``j ≠ i + diag_offset``
    (``diag_offset=None``: all of them), ordered by higher score first and,
    among equal scores, lower column first; slots past the last candidate
    hold ``(−inf, −1)``.  ``1 ≤ k ≤ pair_topk_max_k()``.

    A workgroup keeps running lists for 128 rows over one of ``n_splits``
    contiguous spans of column tiles and a second kernel merges the spans'
    lists (workspace from the torch allocator: ``n_splits · b · capacity``
    pairs).  ``n_splits`` defaults to the smallest value that gives two
    workgroups per CU and is clamped to ``[1, ceil(n / tile)]``; the order
    is total, so the result does not depend on it and is bitwise
    reproducible.  No atomics, no autograd."""
    zi, zt, b, n, d, dev = _pair_block("pair_topk", zimg, ztxt)
    lib = _require_lib()
    k = int(k)
    if not 1 <= k <= lib.pair_topk_max_k():
        raise RuntimeError(
            f"pair_topk serves 1 <= k <= {lib.pair_topk_max_k()} (got {k}); "
            "pass impl='torch' for more")
    tile = lib.pair_topk_tile_dim()
    tiles_m, tiles_n = -(-b // tile), -(-n // tile)
    if n_splits is None:
        n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
        n_splits = -(-2 * n_cu // tiles_m)
    n_splits = max(1, min(int(n_splits), tiles_n))
    cap = lib.pair_topk_capacity(k)
    ws_s = torch.empty((n_splits, b, cap), device=dev, dtype=torch.float32)
    ws_c = torch.empty((n_splits, b, cap), device=dev, dtype=torch.int32)
    out_s = torch.empty((b, k), device=dev, dtype=torch.float32)
    out_c = torch.empty((b, k), device=dev, dtype=torch.int32)
    stream = torch.cuda.current_stream(dev).cuda_stream
    _check(lib.pair_topk_bf16(
        ctypes.c_void_p(stream), _ptr(zi), _ptr(zt), _ptr(ws_s), _ptr(ws_c),
        _ptr(out_s), _ptr(out_c), b, n, d, _diag_arg(diag_offset), k,
        n_splits),
        "pair_topk_bf16")
    return out_s, out_c


def _softmax_block(what: str, zimg: torch.Tensor, ztxt: torch.Tensor,
                   t_prime: torch.Tensor):
    """Validate the embeddings of a softmax op; returns the contiguous
    detached pair, ``t'`` as a device fp32 scalar and the tile counts."""
    zi, zt, b, n, _, dev = _pair_block(what, zimg, ztxt)
    tile = _require_lib().softmax_tile_dim()
    return zi, zt, _prep_scalar(t_prime, dev), -(-b // tile), -(-n // tile)


def _softmax_side(name: str, lse, w, length: int, device):
    """Validate one side (rows or columns) of :func:`softmax_g`: both vectors
    or neither."""
    if (lse is None) != (w is None):
        raise RuntimeError(f"{name}_lse and {name}_w must be given together")
    for what, v in ((f"{name}_lse", lse), (f"{name}_w", w)):
        if v is not None and not _vec_ok(v, torch.float32, length, device):
            raise RuntimeError(
                f"{what} must be a contiguous fp32 ({length},) tensor on "
                f"{device} (got {v.dtype} {tuple(v.shape)} on {v.device})")
    return lse, w


def pair_lse(zimg: torch.Tensor, ztxt: torch.Tensor, t_prime: torch.Tensor,
             rows: bool = True, cols: bool = True):
    """Log-sum-exp of every row and every column of the ``(b, n)`` logit grid
    ``z = exp(t')·zimg @ ztxtᵀ`` without materializing it →
    ``(row_lse (b,) | None, col_lse (n,) | None)``, fresh fp32 tensors; a side
    that is switched off is skipped and returned as ``None``.

    One MFMA pass leaves per-tile ``(max, Σ exp(z − max))`` partials in
    workspaces from the torch allocator (``O((b + n) · tiles)`` floats), a
    second kernel folds them in tile order: no float atomics, bitwise
    reproducible.  ``t_prime`` is read on the device (no host sync).  Column
    chunks (``ztxt[j0:j1]``) and ranks compose in the caller:
    ``torch.logaddexp`` of the row results, ``torch.logsumexp`` over ranks'
    column results.  No autograd."""
    zi, zt, tp, tiles_m, tiles_n = _softmax_block("pair_lse", zimg, ztxt,
                                                  t_prime)
    if not rows and not cols:
        return None, None
    lib = _require_lib()
    b, d = zi.shape
    n = zt.shape[0]
    dev = zi.device

    def side(on, tiles, length):
        if not on:
            return None, None
        return (torch.empty((tiles, length, 2), device=dev,
                            dtype=torch.float32),
                torch.empty(length, device=dev, dtype=torch.float32))

    row_ws, row_lse = side(rows, tiles_n, b)
    col_ws, col_lse = side(cols, tiles_m, n)
    stream = torch.cuda.current_stream(dev).cuda_stream
    _check(lib.softmax_lse_bf16(
        ctypes.c_void_p(stream), _ptr(zi), _ptr(zt), _ptr(tp), _ptr(row_ws),
        _ptr(col_ws), _ptr(row_lse), _ptr(col_lse), b, n, d),
        "softmax_lse_bf16")
    return row_lse, col_lse


def softmax_g(zimg: torch.Tensor, ztxt: torch.Tensor, t_prime: torch.Tensor,
              row_lse: Optional[torch.Tensor], row_w: Optional[torch.Tensor],
              col_lse: Optional[torch.Tensor], col_w: Optional[torch.Tensor],
              diag_offset: Optional[int], g: Optional[torch.Tensor] = None):
    """dL/dlogit of the softmax contrastive loss over the ``(b, n)`` block →
    ``(g, gs_partials)``:

    ``g_ij = row_w_i·exp(z_ij − row_lse_i) + col_w_j·exp(z_ij − col_lse_j)
    − [j == i + diag_offset]·(row_w_i + col_w_j)``, bf16, and one fp32
    ``Σ g_ij·s_ij`` (``s = z / t``) per 128×128 tile, each reduced in a fixed
    order (``dt' = t·gs_partials.sum()``).

    The LSE and weight vectors are fp32 ``(b,)`` / ``(n,)``; a side given as
    ``None, None`` adds no term.  ``diag_offset=None``: no positives.  ``g``
    may be the caller's ``(b, n)`` view with unit column stride — a column
    band of a wider slab: the view carries the offset and its row stride,
    so slicing, not pointer arithmetic, bounds the write; only its elements
    are touched.  No autograd."""
    zi, zt, tp, tiles_m, tiles_n = _softmax_block("softmax_g", zimg, ztxt,
                                                  t_prime)
    lib = _require_lib()
    b, d = zi.shape
    n = zt.shape[0]
    dev = zi.device
    row_lse, row_w = _softmax_side("row", row_lse, row_w, b, dev)
    col_lse, col_w = _softmax_side("col", col_lse, col_w, n, dev)
    g, ldg = _g_view(g, b, n, dev)
    gs = torch.empty(tiles_m * tiles_n, device=dev, dtype=torch.float32)
    stream = torch.cuda.current_stream(dev).cuda_stream
    _check(lib.softmax_g_bf16(
        ctypes.c_void_p(stream), _ptr(zi), _ptr(zt), _ptr(tp), _ptr(row_lse),
        _ptr(row_w), _ptr(col_lse), _ptr(col_w), _ptr(g), _ptr(gs), b, n, d,
        ctypes.c_longlong(ldg), _diag_arg(diag_offset)), "softmax_g_bf16")
    return g, gs


_DUPLICATES = {"positive": 0, "ignore": 1}


def _check_id_labels(duplicates, img_ids, txt_ids, b: int, n: int, dev):
    """What every sample-ID op checks of its labels: a known ``duplicates``
    mode and contiguous int64 ``(b,)`` / ``(n,)`` ids on ``dev``."""
    if duplicates not in _DUPLICATES:
        raise ValueError(f"unknown duplicates {duplicates!r}")
    for what, ids, length in (("img_ids", img_ids, b), ("txt_ids", txt_ids, n)):
        if not _vec_ok(ids, torch.int64, length, dev):
            raise RuntimeError(
                f"{what} must be a contiguous int64 ({length},) tensor on "
                f"{dev} (got {getattr(ids, 'dtype', type(ids))} "
                f"{tuple(getattr(ids, 'shape', ()))} on "
                f"{getattr(ids, 'device', None)})")


def sigmoid_ids(zimg: torch.Tensor, ztxt: torch.Tensor, t_prime: torch.Tensor,
                bias: torch.Tensor, img_ids: torch.Tensor,
                txt_ids: torch.Tensor, duplicates: str = "positive",
                diag_offset: Optional[int] = None,
                g: Optional[torch.Tensor] = None, want_g: bool = True):
    """Sigmoid contrastive loss with sample-ID labels over the ``(b, n)``
    block → ``(partials (tiles, 3) fp32, g | None)``.

    With ``z_ij = exp(t')·<zimg_i, ztxt_j> + bias``: a pair with a negative
    id on either side is masked; ``duplicates="positive"`` makes a pair
    positive where the ids are equal; ``"ignore"`` makes ``j == i +
    diag_offset`` the positive (``None``: none) and masks every other pair
    with equal ids; the rest are negatives.  Per 128×128 tile (row-major tile
    order) ``partials`` holds ``Σ softplus(−l·z)``, ``Σ g·s`` and ``Σ g``
    over the pairs that are not masked, with ``g = −l·σ(−l·z)`` and
    ``s = (z − bias) / t``; each is reduced in a fixed order, so the result
    is bitwise reproducible and the same with and without ``g``.

    Ids are contiguous int64 ``(b,)`` / ``(n,)`` on the embeddings' device
    and are compared as 64-bit values.  ``want_g=False`` runs the loss-only
    kernel and returns ``g`` as ``None``.  Otherwise ``g`` (bf16, 0 where
    masked) is allocated here or is the caller's ``(b, n)`` view with unit
    column stride — a column band of a wider slab: the view carries the
    offset and its row stride, so slicing, not pointer arithmetic, bounds the
    write; only its elements are touched.  ``t_prime`` and ``bias`` are read
    on the device (no host sync).  No autograd."""
    zi, zt, b, n, d, dev = _pair_block("sigmoid_ids", zimg, ztxt)
    _check_id_labels(duplicates, img_ids, txt_ids, b, n, dev)
    ldg = n
    if want_g:
        g, ldg = _g_view(g, b, n, dev)
    elif g is not None:
        raise RuntimeError("g given with want_g=False")
    lib = _require_lib()
    tile = lib.sigmoid_ids_tile_dim()
    tp, bp = _prep_scalar(t_prime, dev), _prep_scalar(bias, dev)
    partials = torch.empty((-(-b // tile) * -(-n // tile), 3), device=dev,
                           dtype=torch.float32)
    stream = torch.cuda.current_stream(dev).cuda_stream
    _check(lib.sigmoid_ids_bf16(
        ctypes.c_void_p(stream), _ptr(zi), _ptr(zt), _ptr(tp), _ptr(bp),
        _ptr(img_ids), _ptr(txt_ids), _ptr(g), _ptr(partials), b, n, d,
        ctypes.c_longlong(ldg), _diag_arg(diag_offset),
        _DUPLICATES[duplicates]),
        "sigmoid_ids_bf16")
    return partials, g


class PairLseIds(NamedTuple):
    """What :func:`pair_lse_ids` returns; a skipped side is three ``None``."""
    row_lse: Optional[torch.Tensor]
    row_pos: Optional[torch.Tensor]
    row_cnt: Optional[torch.Tensor]
    col_lse: Optional[torch.Tensor]
    col_pos: Optional[torch.Tensor]
    col_cnt: Optional[torch.Tensor]


def pair_lse_ids(zimg: torch.Tensor, ztxt: torch.Tensor,
                 t_prime: torch.Tensor, img_ids: torch.Tensor,
                 txt_ids: torch.Tensor, duplicates: str = "positive",
                 diag_offset: Optional[int] = None, rows: bool = True,
                 cols: bool = True) -> PairLseIds:
    """Masked log-sum-exp, positive-logit sum and positive count of every row
    and every column of the ``(b, n)`` logit grid ``z = exp(t')·zimg @ ztxtᵀ``
    with sample-ID labels, without materializing the grid →
    :class:`PairLseIds` of fresh tensors; a side that is switched off is
    skipped and returned as ``None``.

    Pair classes are those of :func:`sigmoid_ids`: a pair with a negative id
    on either side is masked; ``duplicates="positive"`` makes a pair positive
    where the ids are equal; ``"ignore"`` makes ``j == i + diag_offset`` the
    positive (``None``: none) and masks every other pair with equal ids.  A
    masked pair is never a positive.  Then ``lse`` (fp32) runs over the pairs
    that are not masked (``−inf`` where there is none), ``pos`` (fp32) is the
    sum of ``z`` over the positives and ``cnt`` (int32, exact) their number.

    One MFMA pass leaves per-tile partials in workspaces from the torch
    allocator (16 bytes per row and column tile), a second kernel folds them
    in tile order: no atomics, bitwise reproducible.  ``t_prime`` is read on
    the device (no host sync).  Ids are contiguous int64 ``(b,)`` / ``(n,)``
    on the embeddings' device and are compared as 64-bit values.  Column
    chunks (``ztxt[j0:j1]``, ``txt_ids[j0:j1]``, ``diag_offset − j0``)
    compose in the caller: ``torch.logaddexp`` of the row LSEs, sums of the
    row ``pos`` and ``cnt``.  No autograd."""
    zi, zt, b, n, d, dev = _pair_block("pair_lse_ids", zimg, ztxt)
    _check_id_labels(duplicates, img_ids, txt_ids, b, n, dev)
    if not rows and not cols:
        return PairLseIds(None, None, None, None, None, None)
    lib = _require_lib()
    tile = lib.softmax_ids_tile_dim()
    tp = _prep_scalar(t_prime, dev)

    def side(on, tiles, length):
        if not on:
            return None, None, None, None
        # 16-byte records (max, Σ exp, Σ positive logits, count).
        return (torch.empty((tiles, length, 4), device=dev,
                            dtype=torch.int32),
                torch.empty(length, device=dev, dtype=torch.float32),
                torch.empty(length, device=dev, dtype=torch.float32),
                torch.empty(length, device=dev, dtype=torch.int32))

    row_ws, row_lse, row_pos, row_cnt = side(rows, -(-n // tile), b)
    col_ws, col_lse, col_pos, col_cnt = side(cols, -(-b // tile), n)
    stream = torch.cuda.current_stream(dev).cuda_stream
    _check(lib.softmax_ids_lse_bf16(
        ctypes.c_void_p(stream), _ptr(zi), _ptr(zt), _ptr(tp), _ptr(img_ids),
        _ptr(txt_ids), _ptr(row_ws), _ptr(col_ws), _ptr(row_lse),
        _ptr(row_pos), _ptr(row_cnt), _ptr(col_lse), _ptr(col_pos),
        _ptr(col_cnt), b, n, d, _diag_arg(diag_offset),
        _DUPLICATES[duplicates]), "softmax_ids_lse_bf16")
    return PairLseIds(row_lse, row_pos, row_cnt, col_lse, col_pos, col_cnt)


def _softmax_ids_side(name: str, lse, w, pw, length: int, device):
    """Validate one side of :func:`softmax_g_ids`: all three vectors or
    none."""
    if (lse is None) != (pw is None):
        raise RuntimeError(
            f"{name}_lse, {name}_w and {name}_pw must be given together")
    _softmax_side(name, lse, w, length, device)
    if pw is not None and not _vec_ok(pw, torch.float32, length, device):
        raise RuntimeError(
            f"{name}_pw must be a contiguous fp32 ({length},) tensor on "
            f"{device} (got {pw.dtype} {tuple(pw.shape)} on {pw.device})")
    return lse, w, pw


def softmax_g_ids(zimg: torch.Tensor, ztxt: torch.Tensor,
                  t_prime: torch.Tensor, img_ids: torch.Tensor,
                  txt_ids: torch.Tensor, duplicates: str,
                  diag_offset: Optional[int],
                  row_lse: Optional[torch.Tensor],
                  row_w: Optional[torch.Tensor],
                  row_pw: Optional[torch.Tensor],
                  col_lse: Optional[torch.Tensor],
                  col_w: Optional[torch.Tensor],
                  col_pw: Optional[torch.Tensor],
                  g: Optional[torch.Tensor] = None):
    """dL/dlogit of the softmax contrastive loss with sample-ID labels over
    the ``(b, n)`` block → ``(g, gs_partials)``:

    ``g_ij = row_w_i·exp(z_ij − row_lse_i) + col_w_j·exp(z_ij − col_lse_j)
    − [positive]·(row_pw_i + col_pw_j)``, exactly 0 where the pair is masked
    (classes as in :func:`pair_lse_ids`), bf16, and one fp32 ``Σ g_ij·s_ij``
    (``s = z / t``) per 128×128 tile, each reduced in a fixed order
    (``dt' = t·gs_partials.sum()``).

    The LSE and weight vectors are fp32 ``(b,)`` / ``(n,)``; a side given as
    three ``None`` adds no term.  ``g`` may be the caller's ``(b, n)`` view
    with unit column stride — a column band of a wider slab: the view carries
    the offset and its row stride, so slicing, not pointer arithmetic, bounds
    the write; only its elements are touched.  No autograd."""
    zi, zt, b, n, d, dev = _pair_block("softmax_g_ids", zimg, ztxt)
    _check_id_labels(duplicates, img_ids, txt_ids, b, n, dev)
    row_lse, row_w, row_pw = _softmax_ids_side("row", row_lse, row_w, row_pw,
                                               b, dev)
    col_lse, col_w, col_pw = _softmax_ids_side("col", col_lse, col_w, col_pw,
                                               n, dev)
    g, ldg = _g_view(g, b, n, dev)
    lib = _require_lib()
    tile = lib.softmax_ids_tile_dim()
    tp = _prep_scalar(t_prime, dev)
    gs = torch.empty(-(-b // tile) * -(-n // tile), device=dev,
                     dtype=torch.float32)
    stream = torch.cuda.current_stream(dev).cuda_stream
    _check(lib.softmax_ids_g_bf16(
        ctypes.c_void_p(stream), _ptr(zi), _ptr(zt), _ptr(tp), _ptr(img_ids),
        _ptr(txt_ids), _ptr(row_lse), _ptr(row_w), _ptr(row_pw),
        _ptr(col_lse), _ptr(col_w), _ptr(col_pw), _ptr(g), _ptr(gs), b, n, d,
        ctypes.c_longlong(ldg), _diag_arg(diag_offset),
        _DUPLICATES[duplicates]), "softmax_ids_g_bf16")
    return g, gs


class _FusedL2Normalize(torch.autograd.Function):
    """Row-wise L2 normalize via the single-pass HIP kernels (bf16, fp32
    math; torch ``F.normalize(dim=-1)`` semantics) — replaces the ~10-kernel
    autograd chain on the towers' hot path."""

    @staticmethod
    def forward(ctx, x, eps):
        lib = _require_lib()
        x = x.contiguous()
        b, d = x.shape
        y = torch.empty_like(x)
        rn = torch.empty(b, device=x.device, dtype=torch.float32)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        _check(lib.l2norm_fwd_bf16(
            ctypes.c_void_p(stream), ctypes.c_void_p(x.data_ptr()),
            ctypes.c_void_p(y.data_ptr()), ctypes.c_void_p(rn.data_ptr()),
            b, d, ctypes.c_float(eps)), "l2norm_fwd")
        ctx.save_for_backward(y, rn)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _require_lib()
        y, rn = ctx.saved_tensors
        dy = dy.contiguous()
        b, d = y.shape
        dx = torch.empty_like(y)
        stream = torch.cuda.current_stream(y.device).cuda_stream
        _check(lib.l2norm_bwd_bf16(
            ctypes.c_void_p(stream), ctypes.c_void_p(dy.data_ptr()),
            ctypes.c_void_p(y.data_ptr()), ctypes.c_void_p(rn.data_ptr()),
            ctypes.c_void_p(dx.data_ptr()), b, d), "l2norm_bwd")
        return dx, None


def l2_normalize(x: torch.Tensor, eps: float = 1e-12) -> torch.Tensor:
    """L2-normalize rows.  GPU bf16 2-D inputs take the fused kernel pair;
    everything else falls back to ``F.normalize`` (identical semantics)."""
    if (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 2
            and x.shape[1] % 2 == 0 and extension_available()):
        return _FusedL2Normalize.apply(x, eps)
    import torch.nn.functional as F
    return F.normalize(x, dim=-1, eps=eps)


def siglip_bwd_from_g(zimg: torch.Tensor, ztxt: torch.Tensor,
                      t_prime: torch.Tensor, bias: torch.Tensor,
                      grad_output: torch.Tensor, out3: torch.Tensor,
                      g: torch.Tensor, gt: Optional[torch.Tensor],
                      quant: str = "bf16", qcache=None, on_dztxt=None):
    """Backward from the fwd+g saved slab: two gradient GEMMs plus the scalar
    grads — no logits recompute.  ``out3`` is the REDUCED 3-vector
    (:func:`reduce_out3`).  Same return contract as :func:`siglip_bwd`.

    ``on_dztxt(dztxt)`` fires as soon as the text gradient exists so a
    distributed caller overlaps its reduce-scatter with the dzimg GEMM.
    """
    b, d = zimg.shape
    n = ztxt.shape[0]
    t_true = _prep_scalar(t_prime, zimg.device).exp()
    go = _go_scalar(grad_output, zimg.device)
    qc = qcache if quant in ("fp8", "mixed") else None
    t_eff = t_true
    if qc is not None and qc.rowwise:
        # The slabs already fold the per-row ratios, the GEMM scale carries
        # only the tensor-max factor, and dt' needs no scale correction (the
        # MFMA accumulated the true dot) — but there is no dequantize route.
        if not _mm8_ok(b, d, n):
            raise RuntimeError("row-wise fp8 needs 16-aligned GEMM shapes")
    elif quant == "fp8":
        t_eff = t_true * qc.si * qc.st
    # bf16_scale=True: see grad_gemms — the saved-g path scales the bf16
    # products in their own dtype.
    dzimg, dztxt = grad_gemms(GBand(g, gt, ztxt, qc), zimg, n, go * t_true,
                              on_dztxt=on_dztxt, bf16_scale=True)
    return (dzimg, dztxt) + scalar_grads(out3, go, t_eff, t_prime, bias)


def siglip_bwd_from_g_chunks(zimg: torch.Tensor, chunks, t_prime: torch.Tensor,
                             bias: torch.Tensor, grad_output: torch.Tensor,
                             out3s, g_chunks, gt: torch.Tensor, qcaches,
                             on_dztxt=None):
    """Backward from per-chunk saved g (the fp8 ring): text ``chunks`` in row
    order, each with its own e4m3 slab, REDUCED ``out3`` and per-tensor
    :class:`QuantCache` (text scales differ per chunk, the image side is
    shared), plus the one ``(n, b)`` transpose slab ``gt`` — dztxt is a single
    GEMM.  Same return contract as :func:`siglip_bwd_from_g`."""
    t_true = _prep_scalar(t_prime, zimg.device).exp()
    go = _go_scalar(grad_output, zimg.device)
    dzimg, dztxt = grad_gemms(
        [GBand(g, None, zt, qc)
         for g, zt, qc in zip(g_chunks, chunks, qcaches)],
        zimg, gt.shape[0], go * t_true, on_dztxt=on_dztxt, gt_full=gt)
    dt_prime = dbias = 0
    for out3, qc in zip(out3s, qcaches):
        dtp, dbs = scalar_grads(out3, go, t_true * qc.si * qc.st, t_prime,
                                bias)
        dt_prime, dbias = dt_prime + dtp, dbias + dbs
    return dzimg, dztxt, dt_prime, dbias


def siglip_bwd_banded(zimg: torch.Tensor, ztxt: torch.Tensor,
                      t_prime: torch.Tensor, bias: torch.Tensor,
                      grad_output: torch.Tensor, out3: torch.Tensor,
                      slabs, on_dztxt=None):
    """Backward from column-banded saved g (bf16 ``(b, c_k)`` slabs covering
    the text rows in order): per-band GEMMs, still no recompute.  Same
    return contract as :func:`siglip_bwd_from_g`."""
    t_true = _prep_scalar(t_prime, zimg.device).exp()
    go = _go_scalar(grad_output, zimg.device)
    bands, j0 = [], 0
    for g in slabs:
        bands.append(GBand(g, None, ztxt[j0:j0 + g.shape[1]]))
        j0 += g.shape[1]
    dzimg, dztxt = grad_gemms(bands, zimg, ztxt.shape[0], go * t_true,
                              on_dztxt=on_dztxt, bf16_scale=True)
    return (dzimg, dztxt) + scalar_grads(out3, go, t_true, t_prime, bias)
