"""Time the residual layer's two kernels (csrc/residual.hip) on one batch (default 32 x 1080 x 1920, dense HWC) with
device events, and in the same process, alternating call by call, the existing kernels that move bytes of the same
kind: mlic_image_egress_u8 (with and without a reference) and mlic_image_sq_err_blocks_u8.  Every kernel is called
once per round, round after round, so drift of the device's clocks falls on all of them alike; the table holds the
median, minimum and maximum over the rounds.  Two contents: "noise" (base and x independent random bytes: every
histogram bin is hit, runs are short) and "smooth" (a synthetic picture and a copy of it with a few grey levels of
noise: most samples share a context and a bin, the case that contends in the LDS histogram).

--rate MODEL: on synthetic images and weights, per tau in 0, 1, 2, 4, the residual string's bits per sample, the
zeroth-order entropy of the symbols without contexts, and their cross-entropy under the file's 24 tables (escaped
symbols counted at the escape's cost plus their bypass nibbles).  Prints one JSON line; --md PATH also writes the
tables as markdown.

--segments: the segmented residual strings (csrc/residual_coder.hip).  (a) mlic_residual_encode_segments and
mlic_residual_decode_segments on the batch's symbols (both contents, L in 1024, 4096, 16384): the time of the whole
entry between two device events (table upload, the launches -- count, scan, write for the encoder -- and the status
read-back), the bytes in and out, the waves launched, and the bytes of the segments against one serial string.
(b) With --segments-model MODEL: wall time per image of encode_images and decode_images for "MLR1", "MLR2" with the
host coder and "MLR2" with the device coder, on the same images in the same process (--e2e-batch images of the bench
size), and the files' sizes.

--yuv: the two passes over the planes of Y'CbCr frames (csrc/residual_yuv.hip) on a batch of 4:2:0 frames: 8-bit planar
(I420) and semi-planar (NV12), 10-bit planar (LSB words) and semi-planar (P010, MSB words); tau 0 and 1; "noise" and
"smooth" contents; front with x, the statistics launch, front without x, apply without and with a reference.  In the
same rounds, call by call, the RGB kernels that move bytes of the same kind: residual_front_u8 / residual_apply_u8 for
bytes and the _u16 pair (depth 10) for words.  A 4:2:0 frame has half the samples of an RGB image, so the rows to
compare are GB/s, not ms.  Above depth 8 the shift of a content is the shift rule's for its worst frame.  With
--yuv-model MODEL also the wall time per frame of encode_residual_yuv / decode_yuv against plain encode_yuv /
decode_yuv, and the files' sizes split into base, segments and low-bit plane.  Nothing else of the tool runs then.

Algorithmic bytes of the plane kernels, Ns = B (H W + 2 hc wc) samples of w bytes, P = 8 B shift (H G_0 + 2 hc G_1):
    front with x: 2 w Ns read, Ns (ctx) + 2 Ns (sym) + P written      statistics: 2 w Ns read
    front without x: w Ns read, Ns written      apply: w Ns + 2 Ns + P read, w Ns written; with ref: w Ns more read

Algorithmic bytes, counted from the shapes (what has to move, once), N = B*H*W*3 samples:
    front with x: 2 N read, N (ctx) + 2 N (sym) written              front without x: N read, N written
    apply: N + 2 N read, N written; with ref: N more read
    egress_u8: 4 N read, N written; with ref: N more read            sq_err_blocks: 2 N read
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mlic_amd import _lib, codec  # noqa: E402


def _p(t):
    return C.c_void_p(t.data_ptr())


def _rate(model: str, H: int, W: int, rate: int, level):
    from mlic_amd import get_model, synthetic
    dev = torch.device("cuda:0")
    net = get_model(model)
    net.load_state_dict(synthetic.synth_state_dict(model, rate=rate))
    net = net.to(dev).eval()
    net.update()
    x = torch.cat([synthetic.synth_image(H, W, 70 + i) for i in range(2)])
    imgs = (x * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().to(dev)
    plain = codec.encode_images(net, imgs, level=level)
    base, info = codec.decode_images(net, plain, ref=imgs)
    rows = {}
    for tau in (0, 1, 2, 4):
        files, einfo = codec.encode_images(net, imgs, level=level, max_error=tau, return_info=True)
        _, dinfo = codec.decode_images(net, files, ref=imgs)
        f = codec.residual_front(base, imgs, tau, "hwc")
        n = 3 * H * W
        h0 = hc = bits = 0.0
        for b in range(2):
            sym = f["sym"][b].cpu().numpy().reshape(-1).astype(np.int64)
            ctx = f["ctx"][b].cpu().numpy().reshape(-1).astype(np.int64)
            cnt = np.bincount(sym + 255, minlength=511).astype(np.float64)
            pr = cnt[cnt > 0] / n
            h0 += float(-(pr * np.log2(pr)).sum())
            t = codec.residual_tables(f["hist"][b])
            cost = 0.0
            for k in range(codec.RES_CTX):
                if t["m"][k] == codec.RES_ABSENT:
                    continue
                m = int(t["m"][k])
                s = sym[ctx == k]
                fr = t["freq"][k].astype(np.float64)
                inside = np.abs(s) <= m
                cost += float(-np.log2(fr[s[inside] + m] / 65536.0).sum())
                esc = np.abs(s[~inside])
                # the escape symbol, then the bypass coder: a 4-bit count of nibbles and the value's nibbles
                v = np.where(s[~inside] < 0, 2 * (esc - m) - 1, 2 * (esc - m - 1))
                nib = np.ceil(np.log2(v + 1.0) / 4.0)  # 0 for v = 0
                cost += float(esc.size * -math.log2(fr[2 * m + 1] / 65536.0) + (4.0 * (nib + 1)).sum())
            hc += cost / n
            bits += 8.0 * einfo[b]["residual_bytes"] / n
        rows[str(tau)] = {"residual_bits_per_sample": bits / 2, "entropy0_bits_per_sample": h0 / 2,
                          "cross_entropy_tables_bits_per_sample": hc / 2,
                          "header_and_tables_bytes": [codec.peek(fl, n_levels=getattr(net, "levels", None))["header_bytes"]
                                                      for fl in files],
                          "base_bytes": [e["base_bytes"] for e in einfo], "residual_bytes": [e["residual_bytes"] for e in einfo],
                          "max_abs_err": [d["max_abs_err"] for d in dinfo]}
    return {"model": model, "synthetic_rate": rate, "level": level, "H": H, "W": W, "images": 2,
            "base_psnr": [d["psnr"] for d in info], "base_bpp": [d["bpp"] for d in info], "rows": rows}


def _segments_kernels(contents, B, H, W, tau, iters, warmup, lengths):
    """(a): per content and segment length, the two entries between device events."""
    rows = {}
    N = 3 * H * W
    for name, (base, x) in contents.items():
        f = codec.residual_front(base, x, tau, "hwc")
        hist = f["hist"].cpu().numpy()
        tabs = [codec.residual_tables(hist[b]) for b in range(B)]
        serial = None
        for L in lengths:
            n_seg = -(-N // L)
            cap = min(max(codec._seg_cap_of_hist(hist[b], tabs[b], n_seg) for b in range(B)),
                      codec.residual_segment_cap(H, W, L))
            buf = torch.empty(B * cap, dtype=torch.uint8, device=base.device)
            enc, dec, coded = [], [], None
            for it in range(warmup + iters):
                e0, e1, d0, d1 = (torch.cuda.Event(enable_timing=True) for _ in range(4))
                e0.record()
                coded = codec.residual_encode_segments(f["sym"], f["ctx"], tabs, L, "device", cap=cap, out=buf)
                e1.record()
                e1.synchronize()
                data, segb = [c[0] for c in coded], [c[1] for c in coded]
                d0.record()
                q = codec.residual_decode_segments(data, segb, f["ctx"], tabs, L, "device")
                d1.record()
                d1.synchronize()
                if it >= warmup:
                    enc.append(e0.elapsed_time(e1))
                    dec.append(d0.elapsed_time(d1))
            assert torch.equal(q, f["sym"])
            print(f"segments: {name}, L {L} done", file=sys.stderr, flush=True)
            nbytes = sum(len(c[0]) for c in coded)
            if serial is None:  # one serial string per image, for the size comparison (image 0 only: it is slow)
                from mlic_amd import entropy
                serial = len(entropy.rans_encode(f["sym"][0].reshape(-1).cpu().numpy().astype(np.int32),
                                                 f["ctx"][0].reshape(-1).cpu().numpy().astype(np.int32),
                                                 *codec._coder_tables(tabs[0])))
            rows[f"{name}, L {L}"] = {
                "segments_per_image": n_seg, "waves": B * -(-n_seg // 64), "capacity_bytes_per_image": cap,
                "encode_ms_median": statistics.median(enc), "encode_ms_min": min(enc),
                "decode_ms_median": statistics.median(dec), "decode_ms_min": min(dec),
                "encode_bytes_in": 2 * 3 * B * N, "decode_bytes_in": B * N + nbytes, "decode_bytes_out": 2 * B * N,
                "segment_bytes": nbytes, "index_bytes": 4 * n_seg * B,
                "image0_segmented_bytes": len(coded[0][0]) + 4 * n_seg, "image0_serial_bytes": serial,
                "image0_overhead_bytes_per_segment": (len(coded[0][0]) + 4 * n_seg - serial) / n_seg}
    return rows


def _segments_e2e(model, B, H, W, rate, level, tau, lengths, reps):
    """(b): wall time per image of encode_images / decode_images per file kind, and the files' sizes."""
    import time
    from mlic_amd import get_model, synthetic
    dev = torch.device("cuda:0")
    net = get_model(model)
    net.load_state_dict(synthetic.synth_state_dict(model, rate=rate))
    net = net.to(dev).eval()
    net.update()
    x = torch.cat([synthetic.synth_image(H, W, 70 + i) for i in range(B)])
    imgs = (x * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().to(dev)
    kinds = {"MLR1 (host, serial)": {}}
    for L in lengths:
        kinds[f"MLR2 host, L {L}"] = {"residual_segment": L, "residual_coder": "host"}
        kinds[f"MLR2 device, L {L}"] = {"residual_segment": L, "residual_coder": "device"}
    plain = codec.encode_images(net, imgs, level=level)
    codec.decode_images(net, plain)
    torch.cuda.synchronize()
    rows = {}
    for it in range(reps + 1):  # the first round warms up
        for name, kw in kinds.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            files = codec.encode_images(net, imgs, level=level, max_error=tau, **kw)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            out, _ = codec.decode_images(net, files, residual_coder=kw.get("residual_coder", "device"))
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            assert int((out.to(torch.int16) - imgs.to(torch.int16)).abs().max()) <= tau
            r = rows.setdefault(name, {"encode_ms_per_image": [], "decode_ms_per_image": [],
                                       "file_bytes": [len(f) for f in files]})
            print(f"segments e2e: round {it}, {name} done", file=sys.stderr, flush=True)
            if it:
                r["encode_ms_per_image"].append(1e3 * (t1 - t0) / B)
                r["decode_ms_per_image"].append(1e3 * (t2 - t1) / B)
    # the same calls without the second layer: what the residual layer adds
    base = {"encode_ms_per_image": [], "decode_ms_per_image": [], "file_bytes": [len(f) for f in plain]}
    for it in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        codec.encode_images(net, imgs, level=level)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        codec.decode_images(net, plain)
        torch.cuda.synchronize()
        base["encode_ms_per_image"].append(1e3 * (t1 - t0) / B)
        base["decode_ms_per_image"].append(1e3 * (time.perf_counter() - t1) / B)
    rows["plain file (no residual layer)"] = base
    for r in rows.values():
        r["encode_ms_per_image"] = statistics.median(r["encode_ms_per_image"])
        r["decode_ms_per_image"] = statistics.median(r["decode_ms_per_image"])
    return {"model": model, "synthetic_rate": rate, "level": level, "images": B, "H": H, "W": W, "tau": tau,
            "reps": reps, "rows": rows}


def _yuv_contents(B, H, W, depth, msb, dev, g):
    """{"noise" | "smooth": (base, x)}: two (y, cb, cr) tuples of dense 4:2:0 sample planes as words of `depth`."""
    hc, wc = (H + 1) // 2, (W + 1) // 2
    maxv = (1 << depth) - 1
    up = 16 - depth if msb else 0
    # words travel to the device as int16 and are viewed as uint16 there

    def words(t):
        t = (t.to(torch.int32) << up)
        t = t.to(torch.uint8) if depth == 8 else t.to(torch.uint16).view(torch.int16)
        return t.to(dev) if depth == 8 else t.to(dev).view(torch.uint16)

    out = {"noise": tuple(tuple(words(torch.randint(0, maxv + 1, (B, h, w), generator=g)) for h, w in
                                ((H, W), (hc, wc), (hc, wc))) for _ in range(2))}
    sb, sx = [], []
    for p, (h, w) in enumerate(((H, W), (hc, wc), (hc, wc))):
        yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        pic = (0.5 + 0.39 * torch.sin(yy / (97.0 if p == 0 else 48.5)) * torch.cos(xx / (131.0 if p == 0 else 65.5))) * maxv
        pic = pic.round().to(torch.int32).view(1, h, w).expand(B, h, w)
        amp = 3 << (depth - 8)
        sb.append(words(pic))
        sx.append(words((pic + torch.randint(-amp, amp + 1, (B, h, w), generator=g)).clamp(0, maxv)))
    out["smooth"] = (tuple(sb), tuple(sx))
    return out


def _semi_planar(planes):
    """(y, cb, cr) dense -> (y, cb, cr) with cb and cr views of one interleaved buffer (column stride 2)."""
    y, cb, cr = planes
    if cb.dtype == torch.uint16:
        uv = torch.stack((cb.view(torch.int16), cr.view(torch.int16)), -1).contiguous().view(torch.uint16)
    else:
        uv = torch.stack((cb, cr), -1).contiguous()
    return y, uv[..., 0], uv[..., 1]


def _yuv_e2e(model, B, H, W, rate, level, reps):
    import time
    from mlic_amd import get_model, synthetic
    dev = torch.device("cuda:0")
    net = get_model(model)
    net.load_state_dict(synthetic.synth_state_dict(model, rate=rate))
    net = net.to(dev).eval()
    net.update()
    x = torch.cat([synthetic.synth_image(H, W, 70 + i) for i in range(B)])
    rows = {}
    for name, layout, fmt in (("4:2:0 8-bit (I420)", "i420", codec.YuvFormat((2, 2), "bt709", False, "left", 8)),
                              ("4:2:0 10-bit (P010)", "nv12", codec.YuvFormat((2, 2), "bt709", False, "left", 10, True))):
        y, cb, cr = codec.egress_yuv(x.float(), H, W, fmt)  # the CPU restatement: the frames to code
        buf = np.zeros((B, codec.yuv_frame_samples(H, W, layout)), np.uint8 if fmt.depth == 8 else np.uint16)
        for dst, src in zip(codec.split_yuv(buf, H, W, layout, fmt.depth), (y, cb, cr)):
            dst[...] = src.numpy()
        dbuf = torch.from_numpy(buf).to(dev)
        planes = codec.split_yuv(dbuf, H, W, layout, fmt.depth)
        plain = codec.encode_yuv(net, *planes, fmt, level=level)
        codec.decode_yuv(net, plain, fmt)
        for tau in (None, 0, 1):
            enc, dec, files, info = [], [], None, None
            for it in range(reps + 1):  # the first round warms up
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if tau is None:
                    files = codec.encode_yuv(net, *planes, fmt, level=level)
                else:
                    files, info = codec.encode_residual_yuv(net, *planes, fmt, max_error=tau, level=level, return_info=True)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                out, _ = codec.decode_yuv(net, files, fmt)
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                if it:
                    enc.append(1e3 * (t1 - t0) / B)
                    dec.append(1e3 * (t2 - t1) / B)
            if tau == 0:
                assert all(torch.equal(o.cpu().view(torch.int16) if fmt.depth > 8 else o.cpu(),
                                       p.cpu().view(torch.int16) if fmt.depth > 8 else p.cpu()) for o, p in zip(out, planes))
            print(f"yuv e2e: {name}, tau {tau} done", file=sys.stderr, flush=True)
            r = {"encode_ms_per_frame": statistics.median(enc), "decode_ms_per_frame": statistics.median(dec),
                 "file_bytes": sum(len(f) for f in files) / B}
            if info is not None:
                r.update(base_bytes=sum(d["base_bytes"] for d in info) / B, segment_bytes=sum(d["residual_bytes"] for d in info) / B,
                         low_bytes=sum(d["low_bytes"] for d in info) / B, shift=[d["shift"] for d in info])
            rows[f"{name}, " + ("plain encode_yuv / decode_yuv" if tau is None else f"residual, tau {tau}")] = r
    return {"model": model, "synthetic_rate": rate, "level": level, "frames": B, "H": H, "W": W, "reps": reps, "rows": rows}


def _yuv(args):
    """--yuv: see the module's docstring."""
    dev = torch.device("cuda:0")
    B, H, W = args.batch, args.height, args.width
    g = torch.Generator(device="cpu").manual_seed(11)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    fmt8 = codec.YuvFormat((2, 2), "bt709", False, "left", 8)
    fmt10 = codec.YuvFormat((2, 2), "bt709", False, "left", 10)
    fmt10m = codec.YuvFormat((2, 2), "bt709", False, "left", 10, True)
    geom = codec.residual_yuv_geom(H, W, (2, 2))
    Ns = B * geom["N"]
    ctx = torch.empty(B, geom["N"], dtype=torch.uint8, device=dev)
    sym = torch.empty(B, geom["N"], dtype=torch.int16, device=dev)
    count = torch.empty(B, 24, dtype=torch.int32, device=dev)
    hist = torch.empty(B, 24, 128, dtype=torch.int32, device=dev)
    digest = torch.empty(B, dtype=torch.int64, device=dev)
    merr, mq, status = (torch.empty(B, dtype=torch.int32, device=dev) for _ in range(3))
    sq, sq3 = torch.empty(B, dtype=torch.int64, device=dev), torch.empty(B, 3, dtype=torch.int64, device=dev)
    plane = torch.empty(B, geom["groups"] * 3, dtype=torch.int64, device=dev)
    runs = {}
    for label, fmt, semi in (("8-bit planar", fmt8, False), ("8-bit NV12", fmt8, True), ("10-bit planar", fmt10, False),
                             ("10-bit P010", fmt10m, True)):
        w = 1 if fmt.depth == 8 else 2
        contents = _yuv_contents(B, H, W, fmt.depth, fmt.msb, dev, g)
        outp = tuple(torch.empty_like(t.view(torch.int16) if w == 2 else t) for t in contents["noise"][0])
        outp = tuple(t.view(torch.uint16) for t in outp) if w == 2 else outp
        if semi:
            contents = {k: (_semi_planar(b), _semi_planar(x)) for k, (b, x) in contents.items()}
            outp = _semi_planar(outp)
        d = fmt.desc()
        deep = () if w == 1 else (fmt.depth, int(fmt.msb))
        sfx = "yuv8" if w == 1 else "yuv16"
        for tau in (0, 1):
            for cname, (b, x) in contents.items():
                shift = 0
                if w == 2:
                    st = codec.residual_stats_yuv(b, x, fmt, tau)
                    shift = max(codec.residual_shift(fmt.depth, geom["N"], int(m), int(s_)) for m, s_ in
                                zip(st["max_abs_q"].cpu().tolist(), st["sum_abs_q"].cpu().tolist()))
                P = 8 * B * geom["groups"] * shift
                lo = _p(plane) if shift else None
                ba, xa, oa = codec._plane_args(*b), codec._plane_args(*x), codec._plane_args(*outp)
                key = f"{label}, tau {tau}, {cname}"

                def front(ba=ba, xa=xa, tau=tau, shift=shift, lo=lo, d=d, deep=deep, sfx=sfx):
                    _lib.call(f"mlic_image_residual_front_{sfx}", stream, *ba, *xa, C.byref(d), *deep, B, H, W, tau, shift,
                              _p(ctx), _p(count), _p(digest), _p(sym), lo, _p(hist), _p(merr), _p(mq), _p(sq))

                def stats(ba=ba, xa=xa, tau=tau, d=d, deep=deep, sfx=sfx):
                    _lib.call(f"mlic_image_residual_stats_{sfx}", stream, *ba, *xa, C.byref(d), *deep, B, H, W, tau, _p(mq), _p(sq))

                def ctx_only(ba=ba, tau=tau, d=d, deep=deep, sfx=sfx):
                    _lib.call(f"mlic_image_residual_front_{sfx}", stream, *ba, *([None] * 6), C.byref(d), *deep, B, H, W, tau, 0,
                              _p(ctx), _p(count), _p(digest), None, None, None, None, None, None)

                def apply(ba=ba, tau=tau, shift=shift, lo=lo, ref=None, d=d, deep=deep, sfx=sfx, oa=oa):
                    r = [None] * 6 + [None, None] if ref is None else list(ref) + [_p(sq3), _p(merr)]
                    _lib.call(f"mlic_image_residual_apply_{sfx}", stream, *ba, _p(sym), lo, C.byref(d), *deep, B, H, W, tau, shift,
                              *oa, *r, _p(status))

                # the apply rows read the symbols of this row's front pass: the front call runs just before them
                runs[f"front_planes, x | {key} (shift {shift})"] = (2 * w * Ns + 3 * Ns + P, front)
                if tau == 0:
                    runs[f"front_planes, statistics | {key}"] = (2 * w * Ns, stats)
                    runs[f"front_planes, no x | {key}"] = (w * Ns + Ns, ctx_only)
                runs[f"apply_planes | {key} (shift {shift})"] = (2 * w * Ns + 2 * Ns + P, apply)
                runs[f"apply_planes + ref | {key} (shift {shift})"] = \
                    (3 * w * Ns + 2 * Ns + P, lambda apply=apply, xa=xa: apply(ref=xa))
        runs[f"-- keep {label}"] = (0, (contents, outp))  # the buffers live as long as the rows
    # the yardsticks: the RGB kernels on an image batch of the same height and width
    N3 = B * H * W * 3
    y8b = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g).to(dev)
    y8x = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g).to(dev)
    y8o = torch.empty_like(y8b)
    y16b = torch.randint(0, 1024, (B, H, W, 3), dtype=torch.int16, generator=g).to(dev).view(torch.uint16)
    y16x = torch.randint(0, 1024, (B, H, W, 3), dtype=torch.int16, generator=g).to(dev).view(torch.uint16)
    y16o = torch.empty_like(y16b.view(torch.int16)).view(torch.uint16)
    ctx3 = torch.empty(B, 3, H, W, dtype=torch.uint8, device=dev)
    sym3 = torch.empty(B, 3, H, W, dtype=torch.int16, device=dev)
    plane3 = torch.empty(B, codec.residual_plane_words(H, W, 3), dtype=torch.int64, device=dev)
    s4 = (C.c_int64 * 4)(*y8b.stride())
    runs["yardstick: residual_front_u8, x, noise (HWC)"] = (5 * N3, lambda: _lib.call(
        "mlic_image_residual_front_u8", stream, _p(y8b), s4, _p(y8x), s4, B, H, W, 1, _p(ctx3), _p(count), _p(digest), _p(sym3),
        _p(hist), _p(merr)))
    runs["yardstick: residual_apply_u8 (HWC)"] = (4 * N3, lambda: _lib.call(
        "mlic_image_residual_apply_u8", stream, _p(y8b), s4, _p(sym3), B, H, W, 1, _p(y8o), s4, None, None, None, None))
    runs["yardstick: residual_front_u16, x, noise (HWC, depth 10, shift 3)"] = (7 * N3 + 8 * plane3.numel(), lambda: _lib.call(
        "mlic_image_residual_front_u16", stream, _p(y16b), s4, _p(y16x), s4, B, H, W, 10, 1, 3, _p(ctx3), _p(count), _p(digest),
        _p(sym3), _p(plane3), _p(hist), _p(merr), _p(mq), _p(sq)))
    runs["yardstick: residual_apply_u16 (HWC, depth 10, shift 3)"] = (6 * N3 + 8 * plane3.numel(), lambda: _lib.call(
        "mlic_image_residual_apply_u16", stream, _p(y16b), s4, _p(sym3), _p(plane3), B, H, W, 10, 1, 3, _p(y16o), s4, None, None,
        None, None, _p(status)))
    timed = {k: v for k, v in runs.items() if not k.startswith("-- keep")}
    ms = {name: [] for name in timed}
    for it in range(args.warmup + args.iters):
        for name, (_, fn) in timed.items():  # one call of each per round
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= args.warmup:
                ms[name].append(e0.elapsed_time(e1))
    rec = {"yuv": True, "batch": B, "H": H, "W": W, "iters": args.iters, "warmup": args.warmup, "rows": {}}
    for name, (nbytes, _) in timed.items():
        med = statistics.median(ms[name])
        rec["rows"][name] = {"ms_median": med, "ms_min": min(ms[name]), "ms_max": max(ms[name]), "algorithmic_bytes": nbytes,
                             "GBps": nbytes / med / 1e6, "fraction_of_8TBps": nbytes / med / 1e6 / 8000.0}
    if args.yuv_model:
        rec["e2e"] = _yuv_e2e(args.yuv_model, args.e2e_batch, H, W, args.synthetic_rate, args.level, args.e2e_reps)
    print(json.dumps(rec))
    if args.md:
        lines = [f"| {B} x {H} x {W} 4:2:0 frames (yardsticks: RGB images) | ms (median of {args.iters}, device events, whole "
                 f"entry) | min | max | algorithmic MB | GB/s | of 8 TB/s |", "|---|---|---|---|---|---|---|"]
        for name, r in rec["rows"].items():
            lines.append(f"| {name} | {r['ms_median']:.3f} | {r['ms_min']:.3f} | {r['ms_max']:.3f} | "
                         f"{r['algorithmic_bytes'] / 1e6:.1f} | {r['GBps']:.0f} | {100 * r['fraction_of_8TBps']:.1f} % |")
        if args.yuv_model:
            q = rec["e2e"]
            lines += ["", f"| {q['model']} (synthetic rate {q['synthetic_rate']}), {q['frames']} x {q['H']} x {q['W']}, wall ms "
                      f"per frame (median of {q['reps']}) | encode | decode | file B | base B | segments B | low bits B | shift |",
                      "|---|---|---|---|---|---|---|---|"]
            for name, r in q["rows"].items():
                lines.append(f"| {name} | {r['encode_ms_per_frame']:.2f} | {r['decode_ms_per_frame']:.2f} | {r['file_bytes']:.0f} | "
                             + (f"{r['base_bytes']:.0f} | {r['segment_bytes']:.0f} | {r['low_bytes']:.0f} | {r['shift']} |"
                                if "base_bytes" in r else "| | | |"))
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tau", type=int, default=1)
    ap.add_argument("--rate", default=None, metavar="MODEL", help="also the rate table, with this model's synthetic weights")
    ap.add_argument("--rate-size", type=int, nargs=2, default=(512, 768), metavar=("H", "W"))
    ap.add_argument("--synthetic-rate", type=int, default=1)
    ap.add_argument("--level", type=int, default=None)
    ap.add_argument("--md", default=None, help="also write the tables as markdown to this path")
    ap.add_argument("--segments", action="store_true", help="also the segmented coder's entries (csrc/residual_coder.hip)")
    ap.add_argument("--segment-lengths", type=int, nargs="+", default=(1024, 4096, 16384))
    ap.add_argument("--segments-model", default=None, metavar="MODEL", help="with --segments: the end-to-end wall times")
    ap.add_argument("--e2e-batch", type=int, default=8)
    ap.add_argument("--e2e-reps", type=int, default=3)
    ap.add_argument("--yuv", action="store_true", help="the plane kernels of Y'CbCr frames (csrc/residual_yuv.hip) alone")
    ap.add_argument("--yuv-model", default=None, metavar="MODEL", help="with --yuv: the end-to-end wall times and sizes")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("residual_bench needs a HIP device")
    if args.yuv:
        return _yuv(args)
    dev = torch.device("cuda:0")
    B, H, W, tau = args.batch, args.height, args.width, args.tau
    Hp, Wp = (H + 63) // 64 * 64, (W + 63) // 64 * 64
    g = torch.Generator(device="cpu").manual_seed(11)
    noise_b = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g).to(dev)
    noise_x = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g).to(dev)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    pic = (128 + 100 * torch.sin(yy / 97.0) * torch.cos(xx / 131.0)).round().clamp(0, 255).to(torch.uint8)
    smooth_b = pic.view(1, H, W, 1).expand(B, H, W, 3).contiguous()
    smooth_x = (smooth_b.to(torch.int16) + torch.randint(-3, 4, (B, H, W, 3), generator=g).to(dev).to(torch.int16)) \
        .clamp(0, 255).to(torch.uint8)
    out = torch.empty_like(noise_b)
    ctx = torch.empty(B, 3, H, W, dtype=torch.uint8, device=dev)
    sym = torch.empty(B, 3, H, W, dtype=torch.int16, device=dev)
    count = torch.empty(B, 24, dtype=torch.int32, device=dev)
    hist = torch.empty(B, 24, 128, dtype=torch.int32, device=dev)
    digest = torch.empty(B, dtype=torch.int64, device=dev)
    merr = torch.empty(B, dtype=torch.int32, device=dev)
    sq = torch.empty(B, dtype=torch.int64, device=dev)
    x_hat = codec.ingest_u8(noise_b, "hwc")
    blocks = torch.empty(B, (H + 15) // 16, (W + 15) // 16, dtype=torch.int64, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    s4 = (C.c_int64 * 4)(*noise_b.stride())
    s3 = (C.c_int64 * 3)(*x_hat.stride()[:3])
    N = B * H * W * 3

    def front(b, x):
        if x is None:
            return lambda: _lib.call("mlic_image_residual_front_u8", stream, _p(b), s4, None, None, B, H, W, tau, _p(ctx),
                                     _p(count), _p(digest), None, None, None)
        return lambda: _lib.call("mlic_image_residual_front_u8", stream, _p(b), s4, _p(x), s4, B, H, W, tau, _p(ctx),
                                 _p(count), _p(digest), _p(sym), _p(hist), _p(merr))

    def apply(ref):
        r = [_p(noise_x), s4, _p(sq), _p(merr)] if ref else [None, None, None, None]
        return lambda: _lib.call("mlic_image_residual_apply_u8", stream, _p(noise_b), s4, _p(sym), B, H, W, tau, _p(out), s4, *r)

    def egress(ref):
        r = [_p(noise_x), s4, _p(sq)] if ref else [None, None, None]
        return lambda: _lib.call("mlic_image_egress_u8", stream, _p(x_hat), s3, B, H, W, _p(out), s4, *r)

    runs = {
        "residual_front, x, noise": (5 * N, front(noise_b, noise_x)),
        "residual_front, x, smooth": (5 * N, front(smooth_b, smooth_x)),
        "residual_front, no x, noise": (2 * N, front(noise_b, None)),
        "residual_front, no x, smooth": (2 * N, front(smooth_b, None)),
        "residual_apply": (4 * N, apply(False)),
        "residual_apply + ref": (5 * N, apply(True)),
        "egress_u8 (HWC)": (5 * N, egress(False)),
        "egress_u8 (HWC) + sq_err": (6 * N, egress(True)),
        "sq_err_blocks_u8, block 16": (2 * N, lambda: _lib.call("mlic_image_sq_err_blocks_u8", stream, _p(noise_b), s4,
                                                                _p(noise_x), s4, B, H, W, 16, _p(blocks))),
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
    rec = {"batch": B, "H": H, "W": W, "tau": tau, "iters": args.iters, "warmup": args.warmup, "rows": {}}
    for name, (nbytes, _) in runs.items():
        med = statistics.median(ms[name])
        rec["rows"][name] = {"ms_median": med, "ms_min": min(ms[name]), "ms_max": max(ms[name]),
                             "algorithmic_bytes": nbytes, "GBps": nbytes / med / 1e6,
                             "fraction_of_8TBps": nbytes / med / 1e6 / 8000.0}
    if args.rate:
        rec["rate"] = _rate(args.rate, args.rate_size[0], args.rate_size[1], args.synthetic_rate, args.level)
    if args.segments:
        rec["segments"] = _segments_kernels({"noise": (noise_b, noise_x), "smooth": (smooth_b, smooth_x)}, B, H, W, tau,
                                            max(3, args.iters // 4), 1, args.segment_lengths)
        if args.segments_model:
            rec["segments_e2e"] = _segments_e2e(args.segments_model, args.e2e_batch, H, W, args.synthetic_rate, args.level,
                                                tau, args.segment_lengths, args.e2e_reps)
    print(json.dumps(rec))
    if args.md:
        lines = [f"| {B} x {H} x {W}, HWC, tau {tau} | ms (median of {args.iters}) | min | max | algorithmic MB | GB/s | "
                 f"of 8 TB/s |", "|---|---|---|---|---|---|---|"]
        for name, r in rec["rows"].items():
            lines.append(f"| {name} | {r['ms_median']:.3f} | {r['ms_min']:.3f} | {r['ms_max']:.3f} | "
                         f"{r['algorithmic_bytes'] / 1e6:.1f} | {r['GBps']:.0f} | {100 * r['fraction_of_8TBps']:.1f} % |")
        if args.rate:
            q = rec["rate"]
            lines += ["", f"| {q['model']} (synthetic weights, rate {q['synthetic_rate']}), 2 x {q['H']} x {q['W']} | residual "
                      f"bits / sample | entropy, no contexts | cross-entropy, 24 tables | header + tables B | max abs err |",
                      "|---|---|---|---|---|---|"]
            for t, r in q["rows"].items():
                lines.append(f"| tau {t} | {r['residual_bits_per_sample']:.4f} | {r['entropy0_bits_per_sample']:.4f} | "
                             f"{r['cross_entropy_tables_bits_per_sample']:.4f} | {r['header_and_tables_bytes']} | "
                             f"{r['max_abs_err']} |")
        if args.segments:
            lines += ["", f"| segments, {B} x {H} x {W}, tau {tau} | segments / image | waves | encode ms (median) | min | "
                      f"decode ms (median) | min | segment MB | image 0: segmented B | serial B | overhead B / segment |",
                      "|---|---|---|---|---|---|---|---|---|---|---|"]
            for name, r in rec["segments"].items():
                lines.append(f"| {name} | {r['segments_per_image']} | {r['waves']} | {r['encode_ms_median']:.3f} | "
                             f"{r['encode_ms_min']:.3f} | {r['decode_ms_median']:.3f} | {r['decode_ms_min']:.3f} | "
                             f"{r['segment_bytes'] / 1e6:.1f} | {r['image0_segmented_bytes']} | {r['image0_serial_bytes']} | "
                             f"{r['image0_overhead_bytes_per_segment']:.2f} |")
        if args.segments and args.segments_model:
            q = rec["segments_e2e"]
            lines += ["", f"| {q['model']} (synthetic rate {q['synthetic_rate']}), {q['images']} x {q['H']} x {q['W']}, tau "
                      f"{q['tau']}, wall ms per image (median of {q['reps']}) | encode_images | decode_images | file bytes "
                      f"(mean) |", "|---|---|---|---|"]
            for name, r in q["rows"].items():
                lines.append(f"| {name} | {r['encode_ms_per_image']:.2f} | {r['decode_ms_per_image']:.2f} | "
                             f"{sum(r['file_bytes']) / len(r['file_bytes']):.0f} |")
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
