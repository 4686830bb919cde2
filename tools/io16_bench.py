"""Time the four high-bit-depth I/O kernels (csrc/image_io16.hip) on one batch (default 32 x 1080 x 1920; Y'CbCr
4:2:0, BT.2020 limited range, left-sited chroma; padded 1080 -> 1088) with device events, and in the same process,
alternating call by call, their 8-bit counterparts of the same kind on the same shapes: RGB interleaved (HWC) at
depth 16 against uint8 RGB, and P010 (NV12 layout, depth 10, MSB-aligned) and I010 (I420 layout, depth 10,
LSB-aligned) against NV12 and I420 (BT.709, which the 8-bit kernels take).  Every kernel is called once per round,
round after round, so drift of the device's clocks falls on all of them alike; the table holds the median, minimum
and maximum over the rounds.  Prints one JSON line; --md PATH also writes the table as markdown.

Algorithmic bytes, counted from the shapes (what has to move, once), with s = 1 or 2 bytes a sample:
    ingest: s * samples read, B*3*Hp*Wp fp32 written        egress: B*3*H*W fp32 read, s * samples written
    with sq_err: the reference's s * samples read as well   (samples: B*H*W*3 RGB, B*(H*W + 2*ch*cw) Y'CbCr)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
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
        raise SystemExit("io16_bench needs a HIP device")
    dev = torch.device("cuda:0")
    B, H, W = args.batch, args.height, args.width
    Hp, Wp = (H + 63) // 64 * 64, (W + 63) // 64 * 64
    fmt8 = codec.YuvFormat(sub=(2, 2), matrix="bt709", full_range=False, site_x="left")
    p010 = codec.YuvFormat(sub=(2, 2), matrix="bt2020", full_range=False, site_x="left", depth=10, msb=True)
    i010 = codec.YuvFormat(sub=(2, 2), matrix="bt2020", full_range=False, site_x="left", depth=10)
    frame = codec.yuv_frame_samples(H, W, "i420")
    r = np.random.default_rng(7)

    def words(shape, depth, msb):  # uint16 on the device (moved, never computed with there)
        w = r.integers(0, 1 << depth, shape, dtype=np.uint16)
        return torch.from_numpy(w << (16 - depth) if msb else w).to(dev)

    src8 = {k: torch.from_numpy(r.integers(0, 256, (B, frame), dtype=np.uint8)).to(dev) for k in ("i420", "nv12")}
    dst8 = {k: torch.empty(B, frame, dtype=torch.uint8, device=dev) for k in ("i420", "nv12")}
    src16 = {"i420": words((B, frame), 10, False), "nv12": words((B, frame), 10, True)}
    dst16 = {k: torch.empty(B, frame, dtype=torch.int16, device=dev).view(torch.uint16) for k in ("i420", "nv12")}
    fmt16 = {"i420": i010, "nv12": p010}
    rgb8 = torch.from_numpy(r.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).to(dev)
    rgb8_out = torch.empty_like(rgb8)
    rgb16 = words((B, H, W, 3), 16, False)
    rgb16_out = torch.empty(B, H, W, 3, dtype=torch.int16, device=dev).view(torch.uint16)
    x = torch.empty(B, 3, Hp, Wp, dtype=torch.float32, device=dev)
    x_hat = codec.ingest_u8(rgb8, "hwc")
    x_hat = (x_hat + 0.02 * torch.randn(x_hat.shape, device=dev)).contiguous()  # some of it outside [0, 1]
    sq3 = torch.zeros(B, 3, dtype=torch.int64, device=dev)
    sq1 = torch.zeros(B, dtype=torch.int64, device=dev)
    d8 = fmt8.desc()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    s3 = (C.c_int64 * 3)(*x_hat.stride()[:3])
    s4 = (C.c_int64 * 4)(*rgb8.stride())
    yuv_n, rgb_n, f32 = B * frame, B * H * W * 3, B * 3 * 4

    def ingest_yuv8(k):
        a = _planes(codec.split_yuv(src8[k], H, W, k))
        return lambda: _lib.call("mlic_image_ingest_yuv8", stream, *a, C.byref(d8), B, H, W, _p(x), Hp, Wp)

    def ingest_yuv16(k):
        a = _planes(codec.split_yuv(src16[k], H, W, k, depth=10))
        f = fmt16[k]
        d = f.desc()
        return lambda: _lib.call("mlic_image_ingest_yuv16", stream, *a, C.byref(d), 10, int(f.msb), B, H, W, _p(x), Hp, Wp)

    def egress_yuv8(k, ref):
        a = _planes(codec.split_yuv(dst8[k], H, W, k))
        rr = _planes(codec.split_yuv(src8[k], H, W, k)) + [_p(sq3)] if ref else [None] * 7
        return lambda: _lib.call("mlic_image_egress_yuv8", stream, _p(x_hat), s3, B, H, W, C.byref(d8), *a, *rr)

    def egress_yuv16(k, ref):
        a = _planes(codec.split_yuv(dst16[k], H, W, k, depth=10))
        rr = _planes(codec.split_yuv(src16[k], H, W, k, depth=10)) + [_p(sq3)] if ref else [None] * 7
        f = fmt16[k]
        d = f.desc()
        return lambda: _lib.call("mlic_image_egress_yuv16", stream, _p(x_hat), s3, B, H, W, C.byref(d), 10, int(f.msb), *a,
                                 *rr)

    def egress_u8(ref):
        rr = [_p(rgb8), s4, _p(sq1)] if ref else [None, None, None]
        return lambda: _lib.call("mlic_image_egress_u8", stream, _p(x_hat), s3, B, H, W, _p(rgb8_out), s4, *rr)

    def egress_u16(ref):
        rr = [_p(rgb16), s4, _p(sq1)] if ref else [None, None, None]
        return lambda: _lib.call("mlic_image_egress_u16", stream, _p(x_hat), s3, B, H, W, 16, 0, _p(rgb16_out), s4, *rr)

    runs = {
        "ingest u16 RGB (HWC, d 16)": (2 * rgb_n + f32 * Hp * Wp,
                                       lambda: _lib.call("mlic_image_ingest_u16", stream, _p(rgb16), s4, 16, 0, B, H, W,
                                                         _p(x), Hp, Wp)),
        "ingest u8 RGB (HWC)": (rgb_n + f32 * Hp * Wp,
                                lambda: _lib.call("mlic_image_ingest_u8", stream, _p(rgb8), s4, B, H, W, _p(x), Hp, Wp)),
        "ingest yuv16 I010": (2 * yuv_n + f32 * Hp * Wp, ingest_yuv16("i420")),
        "ingest yuv8 I420": (yuv_n + f32 * Hp * Wp, ingest_yuv8("i420")),
        "ingest yuv16 P010": (2 * yuv_n + f32 * Hp * Wp, ingest_yuv16("nv12")),
        "ingest yuv8 NV12": (yuv_n + f32 * Hp * Wp, ingest_yuv8("nv12")),
        "egress u16 RGB (HWC, d 16)": (f32 * H * W + 2 * rgb_n, egress_u16(False)),
        "egress u8 RGB (HWC)": (f32 * H * W + rgb_n, egress_u8(False)),
        "egress yuv16 I010": (f32 * H * W + 2 * yuv_n, egress_yuv16("i420", False)),
        "egress yuv8 I420": (f32 * H * W + yuv_n, egress_yuv8("i420", False)),
        "egress yuv16 P010": (f32 * H * W + 2 * yuv_n, egress_yuv16("nv12", False)),
        "egress yuv8 NV12": (f32 * H * W + yuv_n, egress_yuv8("nv12", False)),
        "egress u16 RGB + sq_err": (f32 * H * W + 4 * rgb_n, egress_u16(True)),
        "egress u8 RGB + sq_err": (f32 * H * W + 2 * rgb_n, egress_u8(True)),
        "egress yuv16 I010 + sq_err": (f32 * H * W + 4 * yuv_n, egress_yuv16("i420", True)),
        "egress yuv8 I420 + sq_err": (f32 * H * W + 2 * yuv_n, egress_yuv8("i420", True)),
        "egress yuv16 P010 + sq_err": (f32 * H * W + 4 * yuv_n, egress_yuv16("nv12", True)),
        "egress yuv8 NV12 + sq_err": (f32 * H * W + 2 * yuv_n, egress_yuv8("nv12", True)),
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
    rec = {"batch": B, "H": H, "W": W, "iters": args.iters, "warmup": args.warmup, "rows": {}}
    for name, (nbytes, _) in runs.items():
        med = statistics.median(ms[name])
        rec["rows"][name] = {"ms_median": med, "ms_min": min(ms[name]), "ms_max": max(ms[name]),
                             "algorithmic_bytes": nbytes, "GBps": nbytes / med / 1e6,
                             "fraction_of_8TBps": nbytes / med / 1e6 / 8000.0,
                             "spread": (max(ms[name]) - min(ms[name])) / med}
    # the two layouts' launches wrote the same samples (P010's are the I010 ones shifted up)
    a = tuple(p.cpu().to(torch.int32) for p in codec.split_yuv(dst16["i420"], H, W, "i420", depth=10))
    b = tuple(p.cpu().to(torch.int32) for p in codec.split_yuv(dst16["nv12"], H, W, "nv12", depth=10))
    rec["i010_shifted_equals_p010"] = all(torch.equal(p << 6, q) for p, q in zip(a, b))
    print(json.dumps(rec))
    if args.md:
        lines = [f"| {B} x {H} x {W} (padded to {Hp} x {Wp}) | ms (median of {args.iters}) | min | max | "
                 f"algorithmic MB | GB/s | of 8 TB/s |", "|---|---|---|---|---|---|---|"]
        for name, row in rec["rows"].items():
            lines.append(f"| {name} | {row['ms_median']:.3f} | {row['ms_min']:.3f} | {row['ms_max']:.3f} | "
                         f"{row['algorithmic_bytes'] / 1e6:.1f} | {row['GBps']:.0f} | {100 * row['fraction_of_8TBps']:.1f} % |")
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
