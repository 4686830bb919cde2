"""Time mlic_image_ms_ssim_u8 on one batch (default 32 x 3 x 1080 x 1920) with device events: warm-up, then
the median of N calls; prints one JSON line with the time, the algorithmic bytes (counted below from the
shapes) and the achieved GB/s.  --cpu also times the float32 torch path of metrics.ms_ssim_u8 on the same
batch (torch's current thread count).

Algorithmic bytes, each level's planes read once and only pooled planes and partial sums written:
  level l reads 2 planes of h_l x w_l fp32 (8 B per pixel-channel), levels 0-3 write 2 pooled planes of
  h_{l+1} x w_{l+1} fp32; the partial sums and the combine kernel are a few KB and are counted too.
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from mlic_amd import _lib, metrics  # noqa: E402


def algorithmic_bytes(B, Cn, H, W, tile=64):
    planes, total, per_level = B * Cn, 0, []
    h, w = H, W
    for level in range(5):
        ho, wo = (h + 1) // 2, (w + 1) // 2
        tiles = -(-(h + h % 2) // tile) * -(-(w + w % 2) // tile)
        rd = 2 * planes * h * w * 4
        wr = (2 * planes * ho * wo * 4 if level < 4 else 0) + planes * tiles * 16
        per_level.append({"level": level, "h": h, "w": w, "read": rd, "written": wr})
        total += rd + wr
        total += planes * tiles * 16  # the combine kernel reads the partial sums back
        h, w = ho, wo
    total += planes * 5 * 8 + B * 8
    return total, per_level


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu", action="store_true")
    args = ap.parse_args()
    B, Cn, H, W = args.batch, 3, args.height, args.width
    nbytes, per_level = algorithmic_bytes(B, Cn, H, W)
    if not torch.cuda.is_available():
        raise SystemExit("ms_ssim_bench needs a HIP device")
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(7)
    # a padded x_hat scored in place: the operands are 1080-row views of 1088-row tensors
    a = torch.rand(B, Cn, H + 8, W, generator=g).to(dev)[:, :, :H]
    b = (a + 0.03 * torch.randn(a.shape, generator=g).to(dev)).clamp(0, 1)
    need = C.c_size_t()
    _lib.call("mlic_ms_ssim_scratch_bytes", B, Cn, H, W, C.byref(need))
    scratch = torch.empty(need.value, dtype=torch.uint8, device=dev)
    out = torch.empty(B, dtype=torch.float64, device=dev)
    sa, sb = (C.c_int64 * 3)(*a.stride()[:3]), (C.c_int64 * 3)(*b.stride()[:3])
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        _lib.call("mlic_image_ms_ssim_u8", st, C.c_void_p(a.data_ptr()), sa, C.c_void_p(b.data_ptr()), sb, B, Cn, H,
                  W, C.c_void_p(scratch.data_ptr()), need.value, C.c_void_p(out.data_ptr()), None)

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
    med = statistics.median(ms)
    rec = {"batch": B, "channels": Cn, "H": H, "W": W, "iters": args.iters, "ms_median": med, "ms_min": min(ms),
           "ms_max": max(ms), "algorithmic_bytes": nbytes,
           "bytes_per_pixel_channel": nbytes / (B * Cn * H * W), "GBps": nbytes / med / 1e6,
           "fraction_of_8TBps": nbytes / med / 1e6 / 8000.0, "scratch_bytes": need.value,
           "value_mean": out.mean().item(), "per_level": per_level}
    if args.cpu:
        ac, bc = a.cpu(), b.cpu()
        t0 = time.time()
        vc = metrics.ms_ssim_u8(ac, bc)
        rec["cpu_float32_s"] = time.time() - t0
        rec["cpu_threads"] = torch.get_num_threads()
        rec["cpu_vs_kernel_max_abs_diff"] = (vc - out.cpu()).abs().max().item()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
