"""Time the scaled-coding edge kernels (csrc/resample.hip) on the GPU.

    python tools/resample_bench.py [--batch 32] [--runs 20] [--out FILE.json]

Per case: the median of `--runs` device-event timings after warm-up, for
  - the fused kernel (codec.ingest_u8_scaled / egress_u8_scaled),
  - the device composition it replaces: .float().div(255) + F.interpolate(bicubic, antialias=True) + clamp + pad64,
    and the reverse chain clamp + interpolate + clamp * 255 + floor + to(uint8) + permute,
  - the plain ingest_u8 / egress_u8 kernels on the image at the kernel's fp32 side (what unscaled coding pays),
and the kernel's own algorithmic bytes (every input and output element once) over 8 TB/s, the HBM peak.
Cases: 32 x 1080 x 1920 <-> 540 x 960 (code at half size, decode to display size) and the thumbnail's inverse,
135 x 240 -> 1080 x 1920 on the egress side with 1080 x 1920 -> 135 x 240 (the thumbnail decode itself).
One JSON line per case on stdout; --out also writes them to a file.  Needs a HIP device: there is no CPU fallback."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM = 8.0e12  # bytes / s


def median_ms(fn, runs, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def pad64(n):
    return (n + 63) // 64 * 64


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--filter", default="bicubic", choices=["lanczos3", "bicubic", "triangle"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench needs a HIP device")
    from mlic_amd import bitstream, codec
    dev = torch.device("cuda:0")
    B, flt = args.batch, args.filter
    g = torch.Generator(device="cpu").manual_seed(0)
    rows = []

    def report(name, src, dst, fused, chain, plain, nbytes):
        ms, lo, hi = median_ms(fused, args.runs)
        cms, _, _ = median_ms(chain, args.runs)
        pms, _, _ = median_ms(plain, args.runs)
        row = {"case": name, "filter": flt, "batch": B, "from": src, "to": dst, "fused_ms": round(ms, 4),
               "fused_min_ms": round(lo, 4), "fused_max_ms": round(hi, 4), "torch_chain_ms": round(cms, 4),
               "plain_kernel_ms": round(pms, 4), "algorithmic_bytes": nbytes,
               "floor_ms_at_8TBs": round(nbytes / HBM * 1e3, 4), "achieved_GBs": round(nbytes / ms / 1e6, 1)}
        rows.append(row)
        print(json.dumps(row), flush=True)

    for (Hi, Wi), (h, w) in (((1080, 1920), (540, 960)), ((1080, 1920), (135, 240))):
        img = torch.randint(0, 256, (B, Hi, Wi, 3), dtype=torch.uint8, generator=g).to(dev)
        small = torch.randint(0, 256, (B, h, w, 3), dtype=torch.uint8, generator=g).to(dev)
        Hp, Wp = pad64(h), pad64(w)

        def chain_in():
            v = img.permute(0, 3, 1, 2).float().div(255)
            v = F.interpolate(v, size=(h, w), mode="bicubic", antialias=True, align_corners=False).clamp(0, 1)
            return bitstream.pad64(v).contiguous()

        report("ingest", (Hi, Wi), (h, w), lambda: codec.ingest_u8_scaled(img, (h, w), flt), chain_in,
               lambda: codec.ingest_u8(small), B * 3 * (Hi * Wi + 4 * Hp * Wp))
        x = torch.rand(B, 3, Hp, Wp, generator=g).to(dev)
        big = torch.rand(B, 3, pad64(Hi), pad64(Wi), generator=g).to(dev)

        def chain_out():
            v = x[:, :, :h, :w].clamp(0, 1)
            v = F.interpolate(v, size=(Hi, Wi), mode="bicubic", antialias=True, align_corners=False)
            return (v.clamp(0, 1) * 255).floor().to(torch.uint8).permute(0, 2, 3, 1).contiguous()

        report("egress", (h, w), (Hi, Wi), lambda: codec.egress_u8_scaled(x, h, w, (Hi, Wi), flt), chain_out,
               lambda: codec.egress_u8(big, Hi, Wi), B * 3 * (4 * h * w + Hi * Wi))
        report("egress+ref", (h, w), (Hi, Wi), lambda: codec.egress_u8_scaled(x, h, w, (Hi, Wi), flt, ref=img), chain_out,
               lambda: codec.egress_u8(big, Hi, Wi, ref=img), B * 3 * (4 * h * w + 2 * Hi * Wi))
        if (h, w) == (135, 240):  # the thumbnail decode: full-size x_hat down to the preview

            def chain_thumb():
                v = F.interpolate(big[:, :, :Hi, :Wi].clamp(0, 1), size=(h, w), mode="bicubic", antialias=True,
                                  align_corners=False)
                return (v.clamp(0, 1) * 255).floor().to(torch.uint8).permute(0, 2, 3, 1).contiguous()

            report("egress-thumbnail", (Hi, Wi), (h, w), lambda: codec.egress_u8_scaled(big, Hi, Wi, (h, w), flt),
                   chain_thumb, lambda: codec.egress_u8(big, Hi, Wi), B * 3 * (4 * Hi * Wi + h * w))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
