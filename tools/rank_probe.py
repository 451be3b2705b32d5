"""Time the fused rank-count kernel against one MFMA pass with a scalar
epilogue and against the torch composite it replaces, in one process.

    python tools/rank_probe.py [--batch 32768] [--dim 768] [--iters 30]

Three timings at the same (B, B, d) bf16 shape, each the median of ``--iters``
warm calls timed one by one between device events:

- ``rank``:      ``ops.pair_rank_counts`` with both sides counted, thresholds
                 at the positive scores, ``diag_offset = 0`` (what
                 ``retrieval_ranks`` launches);
- ``fwd``:       ``ops.siglip_fwd`` — the cost of one MFMA pass over the pair
                 grid with a scalar epilogue;
- ``composite``: the torch code a user writes without the kernel — bf16
                 ``zimg[r0:r1] @ ztxt.T`` in 4096-row chunks, a compare
                 against both threshold vectors and two sums (no positive
                 mask: in the composite's favour).

``--only rank`` times the kernel alone (for a kernel-trace run).  Prints one
JSON line.
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_sigmoid_loss_amd import ops, positive_scores  # noqa: E402


def median_ms(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    return statistics.median(times), min(times), max(times)


def composite(zi, zt, row_thr, col_thr, chunk=4096):
    b, n = zi.shape[0], zt.shape[0]
    rc = torch.empty(b, device=zi.device, dtype=torch.int32)
    cc = torch.zeros(n, device=zi.device, dtype=torch.int32)
    for r0 in range(0, b, chunk):
        r1 = min(b, r0 + chunk)
        s = zi[r0:r1] @ zt.T
        rc[r0:r1] = (s > row_thr[r0:r1, None]).sum(1, dtype=torch.int32)
        cc += (s > col_thr[None, :]).sum(0, dtype=torch.int32)
    return rc, cc


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=32768)
    p.add_argument("--dim", type=int, default=768)
    p.add_argument("--iters", type=int, default=30)
    p.add_argument("--only", choices=["all", "rank"], default="all")
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rank_probe needs a GPU")
    if args.iters < 20:
        raise SystemExit("--iters must be at least 20")

    b, d = args.batch, args.dim
    g = torch.Generator(device="cuda").manual_seed(0)
    zi = torch.nn.functional.normalize(
        torch.randn(b, d, device="cuda", generator=g), dim=-1).bfloat16()
    zt = torch.nn.functional.normalize(
        torch.randn(b, d, device="cuda", generator=g), dim=-1).bfloat16()
    thr = positive_scores(zi, zt, 0)
    rc = torch.zeros(b, device="cuda", dtype=torch.int32)
    cc = torch.zeros(b, device="cuda", dtype=torch.int32)

    def rank():
        ops.pair_rank_counts(zi, zt, thr, thr, 0, row_cnt=rc, col_cnt=cc)

    flop = 2.0 * b * b * d
    out = {"probe": "rank_counts", "batch": b, "dim": d, "iters": args.iters,
           "device": torch.cuda.get_device_name(0)}
    ms, lo, hi = median_ms(rank, args.iters)
    out.update(rank_ms=round(ms, 4), rank_min_ms=round(lo, 4),
               rank_max_ms=round(hi, 4), rank_tflops=round(flop / ms * 1e-9, 1))
    if args.only == "all":
        tp = torch.tensor(10.0, device="cuda").log()
        bias = torch.tensor(-10.0, device="cuda")
        ms_f, lo, hi = median_ms(
            lambda: ops.siglip_fwd(zi, zt, tp, bias, 0), args.iters)
        out.update(fwd_ms=round(ms_f, 4), fwd_min_ms=round(lo, 4),
                   fwd_max_ms=round(hi, 4))
        ms_c, lo, hi = median_ms(lambda: composite(zi, zt, thr, thr),
                                 args.iters)
        out.update(composite_ms=round(ms_c, 4), composite_min_ms=round(lo, 4),
                   composite_max_ms=round(hi, 4),
                   rank_over_fwd=round(ms / ms_f, 3),
                   composite_over_rank=round(ms_c / ms, 3))
        # How often the composite's bf16-rounded logits give the same count.
        k_rc, k_cc = ops.pair_rank_counts(zi, zt, thr, thr, None)
        c_rc, c_cc = composite(zi, zt, thr, thr)
        out.update(composite_rows_equal=round(
            float((k_rc == c_rc).double().mean()), 4))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
