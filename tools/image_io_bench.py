"""Time the uint8 ingest / egress kernels (csrc/image_io.hip) on one batch (default 32 x 1080 x 1920 interleaved
RGB, padded 1080 -> 1088) with device events: warm-up, then the median of N calls, and in the same run the torch
sequences they replace:
    ingest: img.float().div(255) + permute + pad64            egress: to_u8 of the crop + permute().contiguous()
and the rate loop's prefilter (codec.blur3_pad, --blur-batch images of the same size, default 8) next to what the
reference runs on the device for it:
    blur: F.pad(conv2d(x[:, :, :H, :W], gaussian, padding=1, groups=3)) -- crop, depthwise conv, pad to 64 again
Prints one JSON line; --md PATH also writes the table as markdown.

Algorithmic bytes, counted from the shapes (what has to move, once):
    ingest: B*H*W*3 uint8 read, B*3*Hp*Wp fp32 written          egress: B*3*H*W fp32 read, B*H*W*3 uint8 written
    egress with sq_err: the reference image's B*H*W*3 bytes read as well
    blur: B*3*Hp*Wp fp32 read and B*3*Hp*Wp fp32 written
The torch sequences are charged the same bytes, so their GB/s is the same useful work over their time.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from mlic_amd import bitstream, codec  # noqa: E402


def algorithmic_bytes(B, H, W):
    Hp, Wp = (H + 63) // 64 * 64, (W + 63) // 64 * 64
    return {"ingest": B * H * W * 3 + B * 3 * Hp * Wp * 4, "egress": B * 3 * H * W * 4 + B * H * W * 3,
            "egress_ref": B * 3 * H * W * 4 + 2 * B * H * W * 3}


def blur_bytes(B, H, W):
    Hp, Wp = (H + 63) // 64 * 64, (W + 63) // 64 * 64
    return 2 * 4 * B * 3 * Hp * Wp


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--blur-batch", type=int, default=8, help="images of the prefilter rows")
    ap.add_argument("--md", default=None, help="also write the table as markdown to this path")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("image_io_bench needs a HIP device")
    dev = torch.device("cuda:0")
    B, H, W = args.batch, args.height, args.width
    nbytes = algorithmic_bytes(B, H, W)
    nbytes["blur"] = blur_bytes(args.blur_batch, H, W)
    g = torch.Generator(device="cpu").manual_seed(7)
    img = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g).to(dev)
    x_hat = codec.ingest_u8(img, "hwc")
    x_hat = (x_hat + 0.02 * torch.randn(x_hat.shape, device=dev)).contiguous()  # a padded x_hat, some of it outside [0,1]
    out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev)
    xb = codec.ingest_u8(img[:1].expand(args.blur_batch, H, W, 3).contiguous(), "hwc")
    gauss = torch.tensor(codec.BLUR3_WEIGHTS, dtype=torch.float32, device=dev).view(1, 1, 3, 3).repeat(3, 1, 1, 1)

    def blur_torch():
        return bitstream.pad64(torch.nn.functional.conv2d(xb[:, :, :H, :W], gauss, padding=1, groups=3))

    runs = {
        "ingest kernel": ("ingest", lambda: codec.ingest_u8(img, "hwc")),
        "ingest torch": ("ingest", lambda: bitstream.pad64(img.float().div(255).permute(0, 3, 1, 2)).contiguous()),
        "egress kernel": ("egress", lambda: codec.egress_u8(x_hat, H, W, "hwc", out=out)),
        "egress kernel + sq_err": ("egress_ref", lambda: codec.egress_u8(x_hat, H, W, "hwc", ref=img, out=out)),
        "egress torch": ("egress", lambda: bitstream.to_u8(x_hat[:, :, :H, :W]).permute(0, 2, 3, 1).contiguous()),
        f"blur kernel (B = {args.blur_batch})": ("blur", lambda: codec.blur3_pad(xb, H, W)),
        f"blur torch crop + conv2d + pad (B = {args.blur_batch})": ("blur", blur_torch),
    }
    rec = {"batch": B, "H": H, "W": W, "iters": args.iters, "warmup": args.warmup, "algorithmic_bytes": nbytes,
           "rows": {}}
    for name, (kind, fn) in runs.items():
        r = timed(fn, args.warmup, args.iters)
        r["GBps"] = nbytes[kind] / r["ms_median"] / 1e6
        r["fraction_of_8TBps"] = r["GBps"] / 8000.0
        rec["rows"][name] = r
    # the same results: egress exactly; ingest up to torch's device division (a product with 1 / 255)
    a, b = codec.ingest_u8(img, "hwc"), bitstream.pad64(img.float().div(255).permute(0, 3, 1, 2)).contiguous()
    rec["ingest_elements_differing_from_device_torch"] = int((a != b).sum())
    rec["ingest_max_abs_diff_from_device_torch"] = float((a - b).abs().max())
    rec["ingest_equals_cpu_torch_on_image_0"] = bool(torch.equal(
        a[:1].cpu(), bitstream.pad64(img[:1].cpu().float().div(255).permute(0, 3, 1, 2))))
    rec["egress_equals_torch"] = bool(torch.equal(
        codec.egress_u8(x_hat, H, W, "hwc"), bitstream.to_u8(x_hat[:, :, :H, :W]).permute(0, 2, 3, 1)))
    kb, tb = (rec["rows"][k]["ms_median"] for k in list(runs)[-2:])
    rec["blur_speedup_vs_torch"] = tb / kb
    rec["blur_max_abs_diff_from_device_torch"] = float((codec.blur3_pad(xb, H, W) - blur_torch()).abs().max())
    rec["ingest_speedup_vs_torch"] = rec["rows"]["ingest torch"]["ms_median"] / rec["rows"]["ingest kernel"]["ms_median"]
    rec["egress_speedup_vs_torch"] = rec["rows"]["egress torch"]["ms_median"] / rec["rows"]["egress kernel"]["ms_median"]
    print(json.dumps(rec))
    if args.md:
        lines = [f"| {B} x {H} x {W} x 3 uint8 (padded to {(H + 63) // 64 * 64} x {(W + 63) // 64 * 64}) "
                 f"| ms (median of {args.iters}) | min | max | algorithmic MB | GB/s | of 8 TB/s |",
                 "|---|---|---|---|---|---|---|"]
        for name, (kind, _) in runs.items():
            r = rec["rows"][name]
            lines.append(f"| {name} | {r['ms_median']:.3f} | {r['ms_min']:.3f} | {r['ms_max']:.3f} | "
                         f"{nbytes[kind] / 1e6:.1f} | {r['GBps']:.0f} | {100 * r['fraction_of_8TBps']:.1f} % |")
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
