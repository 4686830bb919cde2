"""Measurements for tiled coding (DESIGN.md section 5 "Tiled coding"); prints one JSON line per part.

    python tools/tiled_bench.py blend  [--size 4096 --tile 1024]     the blend launch against egress_u8
    python tools/tiled_bench.py memory [--size 4096 --tile 1024]     peak device memory and wall time, three arms
    python tools/tiled_bench.py cost   [--height 1080 --width 1920 --tile 512]   bpp and PSNR, untiled / V = 0 / V = 32

blend: one launch of mlic_image_tile_blend_u8 over the whole size x size image (T = tile, V = 0 and --overlap, with
and without the squared-error reference) against mlic_image_egress_u8 on one contiguous plane set of the same pixel
count, device events, a warm-up and then rounds that alternate the arms; medians.  The table and the tiles are
built once, so a timed call is the launch alone.  Algorithmic bytes: 12 per pixel read (V = 0; (1 + V / S)^2 times
that with overlap), 3 written, 3 more read with a reference.

memory: each arm in a fresh child process, so that its peak is its own: (a) encode_images + decode_images of the
whole image, (b) encode_tiled + decode_tiled with tile_batch 4, (c) decode_tiled of a 512 x 512 region of (b)'s
file.  Peak = the largest (total - free) device memory sampled after each call (the executor's arena only grows
inside a process) minus what the process held before the first call.

cost: the cost of tiling in bytes and PSNR on the synthetic weights (which say little about seams on trained
checkpoints): the same image untiled, tiled with V = 0 and with V = 32."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mlic_amd import _lib, codec, get_model, synthetic  # noqa: E402


def _net(name):
    net = get_model(name)
    net.load_state_dict(synthetic.synth_state_dict(name, 0))
    net = net.to(torch.device("cuda:0")).eval()
    net.update()
    return net


def _u8_image(H, W, seed=3):
    x = synthetic.synth_image((H + 63) // 64 * 64, (W + 63) // 64 * 64, seed)[0, :, :H, :W]
    return torch.round(x * 255).to(torch.uint8).permute(1, 2, 0).contiguous()


def _event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def blend(args):
    dev = torch.device("cuda:0")
    N, T = args.size, args.tile
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device="cpu").manual_seed(7)
    ref = torch.randint(0, 256, (N, N, 3), dtype=torch.uint8, generator=g).to(dev)
    out = torch.empty(N, N, 3, dtype=torch.uint8, device=dev)
    plane = (torch.rand(1, 3, N, N, device=dev) * 1.1 - 0.05).contiguous()
    sq = torch.zeros(1, dtype=torch.int64, device=dev)
    d3, d4 = (C.c_int64 * 3)(3 * N, 3, 1), (C.c_int64 * 4)(3 * N * N, 3 * N, 3, 1)
    s3 = (C.c_int64 * 3)(3 * N * N, N * N, N)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    arms, keep, nbytes = {}, [], {}

    def egress(with_ref):
        return lambda: _lib.call("mlic_image_egress_u8", stream, p(plane), s3, 1, N, N, p(out), d4,
                                 p(ref) if with_ref else None, d4 if with_ref else None, p(sq) if with_ref else None)

    for with_ref in (False, True):
        name = "egress_u8" + (" + sq_err" if with_ref else "")
        arms[name] = egress(with_ref)
        nbytes[name] = N * N * (12 + 3 + (3 if with_ref else 0))
    for V in (0, args.overlap):
        grid = codec.tile_grid(N, N, T, V)
        tiles = [(torch.rand(3, codec._pad64(h), codec._pad64(w), device=dev) * 1.1 - 0.05) for _, _, h, w in grid["rects"]]
        ptrs = [t.data_ptr() for t in tiles]
        table = torch.tensor(ptrs, dtype=torch.int64).to(dev)
        host = (C.c_void_p * len(ptrs))(*ptrs)
        keep += [tiles, table, host]
        read = sum(12 * h * w for _, _, h, w in grid["rects"])
        for with_ref in (False, True):
            name = f"blend V = {V}" + (" + sq_err" if with_ref else "")
            arms[name] = (lambda table=table, host=host, V=V, with_ref=with_ref: _lib.call(
                "mlic_image_tile_blend_u8", stream, p(table), host, N, N, T, V, 0, 0, N, N, p(out), d3,
                p(ref) if with_ref else None, d3 if with_ref else None, p(sq) if with_ref else None))
            nbytes[name] = read + N * N * (3 + (3 if with_ref else 0))
    for fn in arms.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(args.iters):  # alternate the arms inside every round
        for k, fn in arms.items():
            ms[k].append(_event_ms(fn))
    rec = {"part": "blend", "size": N, "tile": T, "overlap": args.overlap, "iters": args.iters, "warmup": args.warmup, "rows": {}}
    for k, v in ms.items():
        med = statistics.median(v)
        rec["rows"][k] = {"ms_median": med, "ms_min": min(v), "ms_max": max(v), "algorithmic_MB": nbytes[k] / 1e6,
                          "GBps": nbytes[k] / med / 1e6}
    for V in (0, args.overlap):
        for tail in ("", " + sq_err"):
            rec[f"ratio blend V = {V}{tail} / egress_u8{tail}"] = (rec["rows"][f"blend V = {V}{tail}"]["ms_median"] /
                                                                   rec["rows"]["egress_u8" + tail]["ms_median"])
    # V = 0: the same pixels as egress_u8 of each tile pasted in place
    grid = codec.tile_grid(N, N, T, 0)
    tiles = keep[0]
    arms["blend V = 0"]()
    ok = True
    for t, (ty, tx, th, tw) in zip(tiles, grid["rects"]):
        ok = ok and bool(torch.equal(out[ty:ty + th, tx:tx + tw], codec.egress_u8(t.unsqueeze(0), th, tw, "hwc")[0]))
    rec["blend_v0_equals_egress_per_tile"] = ok
    print(json.dumps(rec))


def _used():
    free, total = torch.cuda.mem_get_info()
    return total - free


def memory_arm(args):
    dev = torch.device("cuda:0")
    net = _net(args.model)
    img = torch.from_numpy(np.load(args.image)).to(dev)
    N = img.size(0)
    torch.cuda.synchronize()
    base, peak = _used(), 0
    rec = {"part": "memory", "arm": args.arm, "size": N, "tile": args.tile, "model": args.model}

    def call(fn):
        nonlocal peak
        torch.cuda.synchronize()
        t0 = time.time()
        r = fn()
        torch.cuda.synchronize()
        dt = time.time() - t0
        peak = max(peak, _used() - base)
        return r, dt

    for rnd in range(2):  # the first round sizes the arena and loads code objects; the second is the time
        if args.arm == "untiled":
            files, rec["encode_s"] = call(lambda: codec.encode_images(net, img))
            (px, info), rec["decode_s"] = call(lambda: codec.decode_images(net, files, ref=img.unsqueeze(0)))
            rec.update(bytes=len(files[0]), psnr=info[0]["psnr"])
        elif args.arm == "tiled":
            data, rec["encode_s"] = call(lambda: codec.encode_tiled(net, img, tile=args.tile, overlap=32, tile_batch=4))
            (px, info), rec["decode_s"] = call(lambda: codec.decode_tiled(net, data, ref=img, tile_batch=4))
            rec.update(bytes=len(data), psnr=info["psnr"])
            with open(args.file, "wb") as f:
                f.write(data)
        else:
            with open(args.file, "rb") as f:
                data = f.read()
            t = codec.parse_container_tiled(data)
            side = args.region_side
            y0 = x0 = (t.ny // 2) * (t.T - t.V) + t.V + 50  # inside one tile's interior at the default size and tile
            (px, info), rec["decode_s"] = call(lambda: codec.decode_tiled(net, data, region=(y0, x0, side, side), tile_batch=4))
            rec.update(region=[y0, x0, side, side], tiles_decoded=info["tiles_decoded"])
    rec["peak_device_MB"] = peak / 1e6
    rec["held_before_first_call_MB"] = base / 1e6
    print(json.dumps(rec))


def memory(args):
    N = args.size
    with tempfile.TemporaryDirectory() as tmp:
        image, file = os.path.join(tmp, "image.npy"), os.path.join(tmp, "tiled.bit")
        np.save(image, _u8_image(N, N).numpy())
        for arm in ("tiled", "region", "untiled"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "memory-arm", "--arm", arm, "--image", image,
                                "--file", file, "--tile", str(args.tile), "--model", args.model, "--region-side",
                                str(args.region_side)], timeout=args.arm_timeout)
            if r.returncode != 0:
                raise SystemExit(f"memory arm {arm} failed with status {r.returncode}")


def cost(args):
    net = _net(args.model)
    H, W, T = args.height, args.width, args.tile
    img = _u8_image(H, W)
    rec = {"part": "cost", "H": H, "W": W, "tile": T, "model": args.model, "rows": {}}
    files = codec.encode_images(net, img)
    _, info = codec.decode_images(net, files, ref=img.unsqueeze(0))
    rec["rows"]["untiled"] = {"bytes": len(files[0]), "bpp": info[0]["bpp"], "psnr": info[0]["psnr"]}
    for V in (0, 32):
        data, einfo = codec.encode_tiled(net, img, tile=T, overlap=V, return_info=True)
        _, dinfo = codec.decode_tiled(net, data, ref=img)
        rec["rows"][f"tiled V = {V}"] = {"bytes": len(data), "bpp": dinfo["bpp"], "psnr": dinfo["psnr"],
                                         "grid": list(einfo["grid"]), "index_bytes": 26 + 8 * (len(einfo["tile_bytes"]) + 1)}
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("part", choices=["blend", "memory", "memory-arm", "cost"])
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--tile", type=int, default=None)
    ap.add_argument("--overlap", type=int, default=32, help="blend: the overlap timed next to V = 0")
    ap.add_argument("--model", default="MLICPP_L")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--arm", choices=["untiled", "tiled", "region"])
    ap.add_argument("--image")
    ap.add_argument("--file")
    ap.add_argument("--arm-timeout", type=int, default=240)
    ap.add_argument("--region-side", type=int, default=512)
    args = ap.parse_args()
    if args.tile is None:
        args.tile = 512 if args.part == "cost" else 1024
    if not torch.cuda.is_available():
        raise SystemExit("tiled_bench needs a HIP device")
    {"blend": blend, "memory": memory, "memory-arm": memory_arm, "cost": cost}[args.part](args)


if __name__ == "__main__":
    main()
