"""Time the rate-map kernels (csrc/ratemap.hip) on the GPU, each next to the existing kernel that reads the same bytes.

    python tools/ratemap_bench.py [--batch 32] [--runs 20] [--out FILE.json] [--model MLICPP_L]

Per case: the median of `--runs` device-event timings after warm-up, and the case's algorithmic bytes (every input
and output element of every launch once) over 8 TB/s, the HBM peak.
  - rate_maps (two launches, all four outputs) at the 1080p latent grids, batch x (320, 68, 120) + (192, 17, 30),
    against mlic_neglog2_sum over the same two tensors (which allocates its scratch and waits for the stream inside
    the call, so its event time holds that too: take the kernels' own times from a kernel trace of this program)
  - sq_err_blocks (block 16) against sq_err_roi with an all-ones mask, batch x 1080 x 1920
  - heat_u8 (cell 16, alone and blended over an under-image) against egress_u8, batch x 1080 x 1920
  - net.rate_map against net.forward on one 512 x 768 image: what code_image(rate_map=True) adds is one forward and
    the two map launches
One JSON line per case on stdout; --out also writes them to a file.  Needs a HIP device: there is no CPU fallback."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--model", default="MLICPP_L")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("ratemap_bench needs a HIP device")
    from mlic_amd import _lib, codec, get_model, synthetic
    dev = torch.device("cuda:0")
    B = args.batch
    g = torch.Generator(device="cpu").manual_seed(0)
    rows = []

    def report(name, fn, nbytes, **extra):
        ms, lo, hi = median_ms(fn, args.runs)
        row = {"case": name, "batch": B, "ms": round(ms, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4),
               "algorithmic_bytes": nbytes, "floor_ms_at_8TBs": round(nbytes / HBM * 1e3, 4),
               "achieved_GBs": round(nbytes / ms / 1e6, 1), **extra}
        rows.append(row)
        print(json.dumps(row), flush=True)

    # ---- rate_maps against neglog2_sum
    M, S, N, h, w = 320, 10, 192, 68, 120
    y = torch.rand(B, M, h, w, generator=g).clamp_(1e-9, 1.0).to(dev)
    z = torch.rand(B, N, h // 4, w // 4, generator=g).clamp_(1e-9, 1.0).to(dev)
    n_in = 4 * (y.numel() + z.numel())
    n_maps = 8 * (B * S * h * w + B * (h // 4) * (w // 4))
    n_fin = 8 * (B * h * w + B * (S + 1))
    # terms: the likelihoods in, the two maps out; finish: the maps in twice (cells, plane sums), cell_bits and slice_bits out
    report("rate_maps", lambda: codec.rate_maps(y, z, S), n_in + n_maps + 2 * n_maps + n_fin, terms_launch_bytes=n_in + n_maps,
           finish_launch_bytes=2 * n_maps + n_fin)
    out = torch.empty(2 * B, dtype=torch.float64, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def neglog2():
        _lib.call("mlic_neglog2_sum", st, C.c_void_p(y.data_ptr()), B, y[0].numel(), C.c_void_p(out.data_ptr()))
        _lib.call("mlic_neglog2_sum", st, C.c_void_p(z.data_ptr()), B, z[0].numel(), C.c_void_p(out.data_ptr() + 8 * B))

    report("neglog2_sum(y)+neglog2_sum(z)", neglog2, n_in, note="event time includes the call's hipMalloc, stream wait and hipFree")
    del y, z

    # ---- sq_err_blocks against sq_err_roi, heat_u8 against egress_u8
    H, W = 1080, 1920
    a = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g).to(dev)
    b = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g).to(dev)
    ones = torch.ones(B, H, W, dtype=torch.uint8, device=dev)
    npx = B * H * W
    report("sq_err_blocks(16)", lambda: codec.sq_err_blocks(a, b, 16), 6 * npx + 4 * B * (-(-H // 16)) * (-(-W // 16)))
    report("sq_err_blocks(64)", lambda: codec.sq_err_blocks(a, b, 64), 6 * npx + 4 * B * (-(-H // 64)) * (-(-W // 64)))
    report("sq_err_roi(all-ones mask)", lambda: codec.sq_err_roi(a, b, ones), 7 * npx)
    plane = (torch.rand(B, -(-H // 16), -(-W // 16), generator=g).double() * 40).to(dev)
    report("heat_u8", lambda: codec.heat_u8(plane, H, W, 16, 0.0, 40.0), 3 * npx + 8 * plane.numel())
    report("heat_u8(under, alpha 128)", lambda: codec.heat_u8(plane, H, W, 16, 0.0, 40.0, under=a, alpha=128),
           6 * npx + 8 * plane.numel())
    x = torch.rand(B, 3, 1088, 1920, generator=g).to(dev)
    report("egress_u8", lambda: codec.egress_u8(x, H, W), (12 + 3) * npx)
    del a, b, ones, x, plane

    # ---- what code_image(rate_map=True) adds: one forward and the two map launches
    net = get_model(args.model)
    net.load_state_dict(synthetic.synth_state_dict(args.model, rate=2))
    net = net.to(dev).eval()
    net.update()
    kw = {"s": 2} if hasattr(net, "levels") else {}
    img = synthetic.synth_image(512, 768, 3).to(dev)
    fms, _, _ = median_ms(lambda: net(img, **kw), args.runs)
    rms, _, _ = median_ms(lambda: net.rate_map(img, **kw), args.runs)
    row = {"case": "net.rate_map vs net.forward", "model": args.model, "image": [512, 768], "forward_ms": round(fms, 4),
           "rate_map_ms": round(rms, 4)}
    rows.append(row)
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
