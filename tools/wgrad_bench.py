"""Weight gradients through mmseq_gemm_wgrad (the product's entry: split-K TN GEMM + fixed-order
reduction) at every wgrad shape of the benchmarked step: the joint encoder's (R = 328 320 rows)
and the ViT's (R = 251 520), each with and without the fused bias gradient (column sums of dY).
Prints one JSON line per shape: time (ms) and TFLOP/s of both, and the bias's cost in percent.
usage: python tools/wgrad_bench.py [--iters N] [--shapes joint|vit|all] [--only OUTxIN]
(--only: one shape, for a counter pass that must tell the dispatches of two shapes apart)
A/B: MMSEQ_BENCH_LIB=<another build of the library>; alternate the two in separate runs."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multimodal_sequencing_amd import _native as N  # noqa: E402
if os.environ.get("MMSEQ_BENCH_LIB"):  # A/B runs: another build of the library
    N.LIB_PATH = os.environ["MMSEQ_BENCH_LIB"]

ROWS = {"joint": 328320, "vit": 251520}
SHAPES = ((2304, 768), (768, 768), (3072, 768), (768, 3072))  # out x in: QKV, O, FC1, FC2


def t(fn, iters):
    # as many warm-up calls as timed ones: after three, the first shape of a run still read
    # ~8 % low (its with-bias line, timed second, came out faster than its no-bias line)
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--shapes", choices=("joint", "vit", "all"), default="all")
    ap.add_argument("--only", default=None, help="one shape, e.g. 2304x768")
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in args.only.split("x"))] if args.only else SHAPES
    lib = os.environ.get("MMSEQ_BENCH_LIB", "tree")
    for net in (("joint", "vit") if args.shapes == "all" else (args.shapes,)):
        R = ROWS[net]
        # one pair of operands per row count, sliced per shape (column slices keep the row stride
        # out of the picture: every shape gets its own contiguous copy)
        big_dy = torch.randn(R, 3072, device="cuda").bfloat16()
        big_x = torch.randn(R, 3072, device="cuda").bfloat16()
        for out, inp in shapes:
            dy = big_dy[:, :out].contiguous()
            x = big_x[:, :inp].contiguous()
            gW = torch.zeros(out, inp, device="cuda")
            gb = torch.zeros(out, device="cuda")
            fl = 2.0 * R * out * inp
            t0 = t(lambda: N.gemm_wgrad(dy, x, gW), args.iters)
            t1 = t(lambda: N.gemm_wgrad(dy, x, gW, gb), args.iters)
            print(json.dumps({"lib": lib, "net": net, "R": R, "out": out, "in": inp,
                              "no_bias_ms": round(t0 * 1e3, 4), "no_bias_tf": round(fl / t0 / 1e12, 1),
                              "bias_ms": round(t1 * 1e3, 4), "bias_tf": round(fl / t1 / 1e12, 1),
                              "bias_cost_pct": round((t1 / t0 - 1) * 100, 2)}), flush=True)
            del dy, x


if __name__ == "__main__":
    main()
