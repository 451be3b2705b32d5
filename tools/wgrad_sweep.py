"""Sweep the split-K weight-gradient kernel's slice count against the library
GEMM at one (batch, M, N) shape.

    python tools/wgrad_sweep.py [--batch 32768] [--m 768] [--n 768]

Each timing is the mean of ``--iters`` back-to-back calls between device
events, walking ``--sets`` distinct operand pairs so the 256 MB Infinity
Cache does not hold a call's inputs from the call before (as in a training
step, where other kernels run in between).  The native figure covers both
launches: the split-K kernel and the slice reduction.
"""

import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_sigmoid_loss_amd import ops  # noqa: E402


def timed(fn, pairs, iters):
    for a, x in pairs:
        fn(a, x)
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(iters):
        fn(*pairs[i % len(pairs)])
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=32768)
    p.add_argument("--m", type=int, default=768)
    p.add_argument("--n", type=int, default=768)
    p.add_argument("--iters", type=int, default=40)
    p.add_argument("--sets", type=int, default=4)
    p.add_argument("--slices", type=int, nargs="*",
                   default=[1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 21, 28])
    args = p.parse_args()

    pairs = [(torch.randn(args.batch, args.m, device="cuda").bfloat16(),
              torch.randn(args.batch, args.n, device="cuda").bfloat16())
             for _ in range(args.sets)]
    flop = 2.0 * args.batch * args.m * args.n
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = -(-args.m // 128) * -(-args.n // 128)
    plan = ops._wgrad_slices(args.batch, args.m, args.n, pairs[0][0].device)
    print(f"# shape (batch, M, N) = ({args.batch}, {args.m}, {args.n}); "
          f"{n_cu} CUs; {tiles} tiles of 128x128; plan: {plan} slices")

    ms = timed(lambda a, x: a.T @ x, pairs, args.iters)
    print(f"library a.T @ x            {ms:8.4f} ms  {flop / ms * 1e-9:7.1f} TF/s")
    ref = pairs[0][0].float().T @ pairs[0][1].float()
    for s in args.slices:
        ms = timed(lambda a, x: ops.linear_wgrad(a, x, slices=s), pairs,
                   args.iters)
        err = (ops.linear_wgrad(*pairs[0], slices=s).float() - ref).abs().max()
        print(f"native slices={s:3d} wgs={tiles * s:4d} {ms:8.4f} ms  "
              f"{flop / ms * 1e-9:7.1f} TF/s  max-abs-err {err.item():.4g}")


if __name__ == "__main__":
    main()
