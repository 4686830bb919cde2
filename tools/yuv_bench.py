"""Time the Y'CbCr ingest / egress kernels (csrc/image_yuv.hip) for I420 and NV12 frames on one batch (default
32 x 1080 x 1920, 4:2:0, BT.709 limited range, left-sited chroma; padded 1080 -> 1088) with device events, and in
the same process, alternating call by call, the RGB kernels mlic_image_ingest_u8 / mlic_image_egress_u8 on
interleaved RGB of the same size.  Every kernel is called once per round, round after round, so drift of the
device's clocks falls on all of them alike; the table holds the median, minimum and maximum over the rounds.
Prints one JSON line; --md PATH also writes the table as markdown.

Algorithmic bytes, counted from the shapes (what has to move, once):
    ingest yuv: B*(H*W + 2*ch*cw) uint8 read, B*3*Hp*Wp fp32 written     ingest u8: B*H*W*3 read, the same written
    egress yuv: B*3*H*W fp32 read, B*(H*W + 2*ch*cw) uint8 written       egress u8: the same read, B*H*W*3 written
    with sq_err: the reference frame's bytes read as well
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from mlic_amd import _lib, codec  # noqa: E402


def _p(t):
    return C.c_void_p(t.data_ptr())


def _planes(ts):
    out = []
    for t in ts:
        out += [_p(t), (C.c_int64 * 3)(*t.stride())]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--md", default=None, help="also write the table as markdown to this path")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("yuv_bench needs a HIP device")
    dev = torch.device("cuda:0")
    B, H, W = args.batch, args.height, args.width
    Hp, Wp = (H + 63) // 64 * 64, (W + 63) // 64 * 64
    fmt = codec.YuvFormat(sub=(2, 2), matrix="bt709", full_range=False, site_x="left")
    ch, cw = fmt.chroma_size(H, W)
    frame = codec.yuv_frame_bytes(H, W, "i420")
    g = torch.Generator(device="cpu").manual_seed(7)
    src = {k: torch.randint(0, 256, (B, frame), dtype=torch.uint8, generator=g).to(dev) for k in ("i420", "nv12")}
    dst = {k: torch.empty(B, frame, dtype=torch.uint8, device=dev) for k in ("i420", "nv12")}
    rgb = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g).to(dev)
    rgb_out = torch.empty_like(rgb)
    x = torch.empty(B, 3, Hp, Wp, dtype=torch.float32, device=dev)
    x_hat = codec.ingest_u8(rgb, "hwc")
    x_hat = (x_hat + 0.02 * torch.randn(x_hat.shape, device=dev)).contiguous()  # some of it outside [0, 1]
    sq3 = torch.zeros(B, 3, dtype=torch.int64, device=dev)
    sq1 = torch.zeros(B, dtype=torch.int64, device=dev)
    desc = fmt.desc()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    s3 = (C.c_int64 * 3)(*x_hat.stride()[:3])
    s4 = (C.c_int64 * 4)(*rgb.stride())
    yuv_bytes, rgb_bytes, f32 = B * frame, B * H * W * 3, B * 3 * 4

    def ingest_yuv(k):
        a = _planes(codec.split_yuv(src[k], H, W, k))
        return lambda: _lib.call("mlic_image_ingest_yuv8", stream, *a, C.byref(desc), B, H, W, _p(x), Hp, Wp)

    def egress_yuv(k, ref):
        a = _planes(codec.split_yuv(dst[k], H, W, k))
        r = _planes(codec.split_yuv(src[k], H, W, k)) + [_p(sq3)] if ref else [None] * 7
        return lambda: _lib.call("mlic_image_egress_yuv8", stream, _p(x_hat), s3, B, H, W, C.byref(desc), *a, *r)

    def egress_u8(ref):
        r = [_p(rgb), s4, _p(sq1)] if ref else [None, None, None]
        return lambda: _lib.call("mlic_image_egress_u8", stream, _p(x_hat), s3, B, H, W, _p(rgb_out), s4, *r)

    runs = {
        "ingest yuv8 I420": (yuv_bytes + f32 * Hp * Wp, ingest_yuv("i420")),
        "ingest yuv8 NV12": (yuv_bytes + f32 * Hp * Wp, ingest_yuv("nv12")),
        "ingest u8 RGB (HWC)": (rgb_bytes + f32 * Hp * Wp,
                                lambda: _lib.call("mlic_image_ingest_u8", stream, _p(rgb), s4, B, H, W, _p(x), Hp, Wp)),
        "egress yuv8 I420": (f32 * H * W + yuv_bytes, egress_yuv("i420", False)),
        "egress yuv8 NV12": (f32 * H * W + yuv_bytes, egress_yuv("nv12", False)),
        "egress u8 RGB (HWC)": (f32 * H * W + rgb_bytes, egress_u8(False)),
        "egress yuv8 I420 + sq_err": (f32 * H * W + 2 * yuv_bytes, egress_yuv("i420", True)),
        "egress yuv8 NV12 + sq_err": (f32 * H * W + 2 * yuv_bytes, egress_yuv("nv12", True)),
        "egress u8 RGB (HWC) + sq_err": (f32 * H * W + 2 * rgb_bytes, egress_u8(True)),
    }
    ms = {name: [] for name in runs}
    for it in range(args.warmup + args.iters):
        for name, (_, fn) in runs.items():  # one call of each per round
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= args.warmup:
                ms[name].append(e0.elapsed_time(e1))
    rec = {"batch": B, "H": H, "W": W, "format": repr(fmt), "iters": args.iters, "warmup": args.warmup, "rows": {}}
    for name, (nbytes, _) in runs.items():
        med = statistics.median(ms[name])
        rec["rows"][name] = {"ms_median": med, "ms_min": min(ms[name]), "ms_max": max(ms[name]),
                             "algorithmic_bytes": nbytes, "GBps": nbytes / med / 1e6,
                             "fraction_of_8TBps": nbytes / med / 1e6 / 8000.0,
                             "spread": (max(ms[name]) - min(ms[name])) / med}
    # the bytes the two layouts give are the same planes
    a, b = (tuple(p.clone() for p in codec.split_yuv(dst[k], H, W, k)) for k in ("i420", "nv12"))
    rec["i420_equals_nv12"] = all(torch.equal(p, q) for p, q in zip(a, b))
    print(json.dumps(rec))
    if args.md:
        lines = [f"| {B} x {H} x {W} (padded to {Hp} x {Wp}), 4:2:0 | ms (median of {args.iters}) | min | max | "
                 f"algorithmic MB | GB/s | of 8 TB/s |", "|---|---|---|---|---|---|---|"]
        for name, r in rec["rows"].items():
            lines.append(f"| {name} | {r['ms_median']:.3f} | {r['ms_min']:.3f} | {r['ms_max']:.3f} | "
                         f"{r['algorithmic_bytes'] / 1e6:.1f} | {r['GBps']:.0f} | {100 * r['fraction_of_8TBps']:.1f} % |")
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
