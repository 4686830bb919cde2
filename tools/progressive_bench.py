"""Time progressive decoding on the GPU (DESIGN.md section 5 "Progressive coding").

    python tools/progressive_bench.py [--what decode|prefix|sizes|kernels] [--batch 8] [--runs 7] [--out FILE.json]

MLICPP_L with the realistic-rate synthetic weights on `--batch` images of 1088 x 1920.  Every time is a host clock
around a call that ends in a stream synchronise (net.decompress brackets itself so), the median of `--runs` after
two warm-up calls, with the minimum and maximum beside it.
  decode   net.decompress of the plain strings.  Uses nothing this feature added, so the same file times a library
           and package from before it ($MLIC_HIP_LIB and the import path choose them): run the two alternately.
  prefix   plain decode, layered decode at K = S, and the prefix decode at K = 0, 1, 2, 5, S for both fills, each
           with the host's wait and rANS-decode milliseconds of the call (mlic_host_stats, summed over threads).
  sizes    bytes per image of plain and layered files at two rates, and for one image layer_bytes * 8 beside
           rate_map's slice_bits.
  kernels  phase_fill and phase_dequant (int16 zero symbols), 50 launches each at batch x (32, 68, 120), for a kernel
           trace of this program; prints their algorithmic bytes (the means read once, y_hat written once: phase 0
           writes all of it, phase 1 half; phase_dequant also reads 2 bytes per symbol).
One JSON line per case on stdout; --out also writes them to a file.  Needs a HIP device: there is no CPU fallback."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, W = 1088, 1920


def timed(fn, runs, warmup=2):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"ms": round(ts[len(ts) // 2], 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["decode", "prefix", "sizes", "kernels"], default="prefix")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("progressive_bench needs a HIP device")
    from mlic_amd import _lib, get_model, synthetic
    dev = torch.device("cuda:0")
    B = args.batch
    rows = []

    def emit(row):
        row = {"what": args.what, "tag": args.tag, "batch": B, **row}
        rows.append(row)
        print(json.dumps(row), flush=True)

    def model(rate):
        net = get_model("MLICPP_L")
        net.load_state_dict(synthetic.synth_state_dict("MLICPP_L", rate=rate))
        net = net.to(dev).eval()
        net.update()
        return net

    def host_ms(net, fn):
        e, d, w = C.c_double(), C.c_double(), C.c_double()
        _lib.call("mlic_host_stats", net._handle, C.byref(e), C.byref(d), C.byref(w), 1)
        fn()
        _lib.call("mlic_host_stats", net._handle, C.byref(e), C.byref(d), C.byref(w), 1)
        return {"host_dec_ms": round(d.value, 3), "host_wait_ms": round(w.value, 3)}

    if args.what == "kernels":
        Cn, h, w = 32, H // 16, W // 16
        n = Cn * h * w
        params = torch.randn(B, 2 * n, device=dev)
        yh = torch.zeros(B, n, device=dev)
        sym16 = torch.zeros(B * n // 2, dtype=torch.int16, device=dev)
        table = torch.linspace(0.11, 64.0, 64, device=dev)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for phase in (0, 1):
            d = _lib.QuantDesc(params=params.data_ptr(), params_bs=2 * n, yh=yh.data_ptr(), yh_bs=n, nlim=32767, ntable=64,
                               table=table.data_ptr(), phase=phase, vbr=0, B=B, C=Cn, H=h, W=w,
                               sym16=sym16.data_ptr())
            for _ in range(50):
                _lib.call("mlic_phase_fill_run", st, C.byref(d))
            for _ in range(50):
                _lib.call("mlic_phase_dequant_run", st, C.byref(d))
            wrote = 4 * B * n if phase == 0 else 2 * B * n
            emit({"phase": phase, "elements": B * n, "phase_fill_bytes": 2 * B * n + wrote,
                  "phase_dequant_bytes": 2 * B * n + wrote + B * n})
    else:
        x = torch.cat([synthetic.synth_image(H, W, 20 + i) for i in range(B)]).to(dev)
        net = model(2)
        layered = hasattr(net, "decompress_layers")
        c = net.compress(x, **({"layered": True} if layered and args.what != "decode" else {}))
        S = net.slice_num
        if args.what == "decode":
            emit({"case": "decompress(plain strings)", **timed(lambda: net.decompress(c["strings"], c["shape"]), args.runs)})
        elif args.what == "prefix":
            zs = c["strings"][1]
            plain = lambda: net.decompress(c["strings"], c["shape"])  # noqa: E731
            emit({"case": "decompress(plain strings)", **timed(plain, args.runs), **host_ms(net, plain)})
            lay = lambda: net.decompress_layers(c["layers"], zs, c["shape"])  # noqa: E731
            emit({"case": f"decompress_layers, K = {S}", **timed(lay, args.runs), **host_ms(net, lay)})
            for fill in ("mean", "zero"):
                for K in (0, 1, 2, 5, S):
                    f = lambda: net.decompress(c["strings"], c["shape"], slices=K, fill=fill)  # noqa: E731
                    emit({"case": f"decompress(slices={K}, fill={fill})", "slices": K, "fill": fill,
                          **timed(f, args.runs), **host_ms(net, f)})
        else:
            from mlic_amd import codec
            for rate in (2, 5):
                n2 = net if rate == 2 else model(rate)
                c2 = c if rate == 2 else n2.compress(x, layered=True)
                plain = [len(codec.write_container(H, W, c2["shape"], c2["strings"][0][b], c2["strings"][1][b]))
                         for b in range(B)]
                lay = [len(codec.write_container_layered(H, W, c2["shape"], c2["strings"][1][b], c2["layers"][b]))
                       for b in range(B)]
                emit({"case": "file bytes per image", "rate_set": rate, "plain": plain, "layered": lay,
                      "overhead": [a - b for a, b in zip(lay, plain)],
                      "y_strings": [len(s) for s in c2["strings"][0]],
                      "sum_of_layers": [sum(len(l) for l in c2["layers"][b]) for b in range(B)]})
            sb = net.rate_map(x[:1])["slice_bits"][0].cpu().tolist()
            emit({"case": "coded bits against estimate, image 0", "layer_bits": [8 * len(l) for l in c["layers"][0]],
                  "slice_bits": [round(v, 1) for v in sb[:-1]]})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
