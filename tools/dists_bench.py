"""Time mlic_image_dists_u8 (csrc/dists.hip) on one 1920 x 1088 pair and on a batch of 8 pairs with device
events, as tools/lpips_bench.py does for LPIPS: warm-up, then the median of N calls; then the same calls with the
library's stage timing on (mlic_dists_profile: event pairs around the stem, the twelve dense convs with their
operand packs, and the set-0, tap, stats and reduce launches).  Prints one JSON line; --md PATH also writes the
table as markdown.

Roofs as in lpips_bench:
    dense convs: algorithmic FLOP (2 * Cout * Cin * 9 * h * w per image and layer, on the CEIL grids) over their
                 time, of the 833 TF/s split-fp16 MFMA peak
    stem:        2 * 3 * H * W floats read, 2 * 64 * H * W floats written per pair, of 8 TB/s
    taps:        per tap the planes of both images read once (2 * C * h * w * 4 bytes) and, taps 1-4, the L2-pooled
                 planes written (2 * C * ceil(h/2) * ceil(w/2) * 4), of 8 TB/s; the strip halo rows, the partials
                 and set 0 (the image itself, 1 % of tap 1) are not charged
Weights are metrics.dists_synthetic_weights(7); the images are a synthetic image and a noisy copy."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from mlic_amd import _lib, metrics, synthetic  # noqa: E402

PEAK_TFLOPS, PEAK_GBPS = 833.0, 8000.0


def algorithmic(H, W):
    """Per pair: dense-conv FLOP, stem bytes, tap bytes."""
    hs, ws = [H], [W]
    for _ in range(4):
        hs.append((hs[-1] + 1) // 2)
        ws.append((ws[-1] + 1) // 2)
    flop, k = 0, 0
    for l in range(1, 13):
        while l > metrics.LPIPS_TAP_LAST[k]:
            k += 1
        flop += 2 * 2 * metrics.LPIPS_COUT[l] * metrics.LPIPS_CIN[l] * 9 * hs[k] * ws[k]
    stem = 2 * (3 + 64) * H * W * 4
    taps = 0
    for k, c in enumerate(metrics.LPIPS_TAP_C):
        taps += 2 * c * hs[k] * ws[k] * 4
        if k < 4:
            taps += 2 * c * hs[k + 1] * ws[k + 1] * 4
    return flop, stem, taps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1088)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--precision", type=int, default=2)
    ap.add_argument("--md", default=None, help="also write the table as markdown to this path")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dists_bench needs a HIP device")
    dev = torch.device("cuda:0")
    H, W = args.height, args.width
    sd = metrics.dists_synthetic_weights(7)
    names = list(sd)
    h = metrics.dists_create_handle(names, [sd[k].to(dev) for k in names], dev)
    _lib.call("mlic_dists_set_precision", h, args.precision)
    flop, stem_b, tap_b = algorithmic(H, W)
    rec = {"H": H, "W": W, "precision": args.precision, "iters": args.iters, "warmup": args.warmup,
           "per_pair": {"dense_conv_gflop": flop / 1e9, "stem_mb": stem_b / 1e6, "tap_mb": tap_b / 1e6}, "rows": {}}
    base = synthetic.synth_image(H, W, 5).to(dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for B in [int(v) for v in args.batches.split(",")]:
        a = base.expand(B, 3, H, W).contiguous()
        b = (a + torch.randn(a.shape, device=dev) * (4 / 255.0)).contiguous()
        need = C.c_size_t()
        _lib.call("mlic_dists_scratch_bytes", B, H, W, C.byref(need))
        scratch = torch.empty(need.value, dtype=torch.uint8, device=dev)
        out = torch.empty(B, dtype=torch.float64, device=dev)
        sa, sb = (C.c_int64 * 3)(*a.stride()[:3]), (C.c_int64 * 3)(*b.stride()[:3])

        def call():
            _lib.call("mlic_image_dists_u8", h, st, C.c_void_p(a.data_ptr()), sa, C.c_void_p(b.data_ptr()), sb, B, H, W,
                      C.c_void_p(scratch.data_ptr()), need.value, C.c_void_p(out.data_ptr()), None)

        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        stages = (C.c_double * 3)()
        _lib.call("mlic_dists_profile", h, 1, None)
        for _ in range(args.iters):
            call()
        _lib.call("mlic_dists_profile", h, 0, stages)
        stem_ms, conv_ms, tap_ms = (v / args.iters for v in stages)
        row = {"scratch_mb": need.value / 1e6, "ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms),
               "ms_per_pair": statistics.median(ms) / B, "stem_ms": stem_ms, "conv_ms": conv_ms, "tap_ms": tap_ms,
               "conv_tflops": B * flop / conv_ms / 1e9, "stem_gbps": B * stem_b / stem_ms / 1e6,
               "tap_gbps": B * tap_b / tap_ms / 1e6, "dists_first": out[0].item()}
        row["conv_fraction_of_peak"] = row["conv_tflops"] / PEAK_TFLOPS
        row["stem_fraction_of_hbm"] = row["stem_gbps"] / PEAK_GBPS
        row["tap_fraction_of_hbm"] = row["tap_gbps"] / PEAK_GBPS
        rec["rows"][str(B)] = row
        del scratch
    n = C.c_int64()
    _lib.call("mlic_dists_range_fallbacks", h, C.byref(n), 0)
    rec["range_fallbacks"] = n.value
    _lib.call("mlic_dists_destroy", h)
    print(json.dumps(rec))
    if args.md:
        lines = [f"| {H} x {W}, precision {args.precision} | ms / call (median of {args.iters}) | ms / pair | stem ms | "
                 "dense convs ms | taps ms | convs TF/s (of 833) | stem GB/s (of 8000) | taps GB/s (of 8000) |",
                 "|---|---|---|---|---|---|---|---|---|"]
        for B, r in rec["rows"].items():
            lines.append(f"| B = {B} | {r['ms_median']:.2f} | {r['ms_per_pair']:.2f} | {r['stem_ms']:.2f} | "
                         f"{r['conv_ms']:.2f} | {r['tap_ms']:.2f} | {r['conv_tflops']:.0f} "
                         f"({100 * r['conv_fraction_of_peak']:.1f} %) | {r['stem_gbps']:.0f} "
                         f"({100 * r['stem_fraction_of_hbm']:.1f} %) | {r['tap_gbps']:.0f} "
                         f"({100 * r['tap_fraction_of_hbm']:.1f} %) |")
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
