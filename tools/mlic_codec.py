"""Image file -> bitstream file -> image file with the uint8 codec path (mlic_amd/codec.py).

    python tools/mlic_codec.py encode IMAGE OUT.bit --model MLICPP_L --checkpoint ckpt.pth.tar
    python tools/mlic_codec.py decode IN.bit IMAGE  --model MLICPP_L --checkpoint ckpt.pth.tar
    ... --synthetic SEED instead of --checkpoint: the seeded synthetic weights (mlic_amd/synthetic.py)
    ... --level N: the level of a *_VBR model (encode; a decode reads it from the file)
    ... --max-bpp X [--max-passes N]: encode under a budget of X bits per pixel (the whole file): while the file
        is above it, the 3x3 Gaussian prefilter and another encode, at most N times (default 8)
    ... --level auto (with --max-bpp): the highest level of a *_VBR model whose unfiltered file fits
    ... --roi MASK --roi-levels LO HI (encode, a *_VBR model): ROI coding.  MASK is an image of the picture's size,
        read as images are, first channel, nonzero = inside the region of interest: 64 x 64 blocks outside it are
        coded at level LO, blocks inside at up to HI.  The file carries the level map; decode needs no flag
    ... --tile T [--overlap V] (encode): tiled coding.  The image is cut into T x T tiles (T a multiple of 64, at
        least 128) that overlap by V pixels (0, 16, 32 or 64; default 32), each tile is coded by itself, and the
        file is the tiled container with an index.  Device memory is that of --tile-batch tiles (default 8)
        whatever the image's size.  Goes with --level N; not with --max-bpp, --level auto or --roi
    ... --region Y0 X0 H W (decode, a tiled file): decode that window only; the tiles outside it are not touched.
        A tiled file is recognised by its magic; decode needs no --tile
    ... --scale N/D | --coded-size WxH [--filter lanczos3|bicubic|triangle] (encode): scaled coding.  The image is
        resampled to the coded size (per axis max(1, floor(L * N/D + 1/2)), ratio 1/8 to 8) in the ingest launch,
        coded at that size, and the scaled file records the display size and the filter; --level and --max-bpp act
        on the coded image, bpp is the whole file over the display pixels.  A scaled file is recognised by its
        magic and decodes to its display size
    ... --out-size WxH [--filter F] (decode): the output size of any plain, VBR or scaled file (a thumbnail
        without the full-size image; a plain file is resampled with lanczos3 unless --filter says otherwise).
        Scaled coding is not together with --roi, --tile, --region, frame files or a depth above 8
    ... a source (encode) or destination (decode) named .y4m or .yuv is an 8-bit Y'CbCr frame, coded without an RGB
        round trip (codec.encode_yuv / decode_yuv).  .y4m: C420jpeg (centre-sited chroma), C420mpeg2 / C420 (left),
        C422, C444; any other colour space or bit depth is refused by its tag.  Raw .yuv: --yuv i420|nv12|nv21|yv12|
        i422|i444 (default i420) and --size WxH.  --frame N picks the frame (default 0; one frame is coded).
        --matrix 601|709|2020 (default 709), --range full|limited (default limited) and --chroma-site left|centre (default:
        the y4m tag's, else left) say what the bytes mean; none of it is written into the bitstream, so a decode
        takes the same flags.  decode ... --ref SRC prints the PSNR per plane and the 6:1:1 mean against SRC.
        Not together with --roi, --tile or --region
    python tools/mlic_codec.py info IN.bit --model MLICPP_L_VBR     what the file says (and its level map, or
        for a tiled file its grid and per-tile sizes)
    python tools/mlic_codec.py ratemap IMAGE -o HEAT.png --model M --checkpoint C [--level L | --roi MASK --roi-levels
        LO HI] [--what bits|slice K|z|error] [--cmap hot|gray] [--alpha A] [--hi X] [--csv FILE]
        where the bits go (codec.rate_map: one forward of the model, no file is written): a heat map of the image's
        size.  --what bits (default): bits per 16 x 16 cell, z's share included; slice K: slice K's bits per cell;
        z: the hyper latent's bits per 64 x 64 cell; error: the squared error of the reconstruction per 16 x 16
        block.  --hi X: the value drawn at full scale (default: the plane's maximum; 0 is the other end).  --alpha A
        (0..256, default 256): blend the map over the image, 256 = the map alone.  --csv FILE: the per-slice bit
        totals and the plane, as text.  An 8-bit RGB image; not together with any other coding option

    ... --layered (encode): progressive coding.  The y symbols are coded as one rANS string per channel slice and
        the file is the layered file, which still decodes when it is cut after any layer.  Goes with --level N; not
        with --max-bpp, --level auto, --roi, --tile, --scale / --coded-size or frame files
    ... --slices K [--fill mean|zero] (decode): entropy-decode the first K channel slices only, of a plain, VBR or
        layered file.  mean (default): the other slices take their predicted mean (and the latent residual
        prediction); zero: they are cleared and the slice loop stops after slice K - 1 (the cheap preview).  A
        layered file, whole or truncated, is recognised by its magic; without --slices every layer it holds is
        decoded.  Not with --out-size, --region or frame files
    ... --max-error T / --lossless (encode): residual coding.  The image is coded as without it and a second layer
        brings every sample of the decode within T of the original (--lossless = 0: the decode is the original);
        the file is the residual file around the unchanged base file.  Goes with --level N; not with --max-bpp,
        --level auto, --roi, --tile, --scale, --coded-size, --layered or Y'CbCr frames.
    ... --residual-segment L (encode, with --max-error / --lossless): the segmented residual file ("MLR2"): the
        residual string in independent segments of L samples (256..65536), coded and decoded on the GPU.
        --residual-coder host|device (encode with --residual-segment, decode): which coder runs; the bytes and the
        picture are the same either way.  decode, strip and info recognise the file by its magic.
        An image deeper than 8 bits (a 16-bit PPM) gets the deep residual file ("MLR3"): always segmented
        (--residual-segment defaults to the codec's 4096), the low bits of every residual stored raw;
        --residual-shift S fixes how many (0..depth - 7; default: the codec's shift rule).  decode writes the 16-bit
        PPM at the file's depth.
    ... --frame-max-error T / --frame-lossless (encode of a .y4m or .yuv frame): residual coding of the planes
        themselves (the "MLR4" file): every sample of Y', Cb and Cr of the decode is within T of the source's, at the
        frame's own subsampling and depth; always segmented, with --residual-segment, --residual-shift (frames deeper
        than 8 bits) and --residual-coder as above.  decode of such a file to .y4m / .yuv takes matrix, range, siting,
        subsampling and depth from the file.  Not with --max-bpp, --level auto, --roi, --tile, --scale or --layered.
    ... --base-only (decode): the base picture of a residual file alone, without the second layer.
    python tools/mlic_codec.py strip IN.bit -o OUT.bit             the base file inside a residual file
    python tools/mlic_codec.py truncate IN.bit -k K -o OUT.bit     the first bytes of a layered file up to the end
        of layer K - 1 (K = 0: the header and z alone); needs no model

    ... samples deeper than 8 bits (codec.encode_images(depth=) / YuvFormat(depth=); the bitstream does not know
        its depth).  A binary PPM of maxval 2^d - 1, d from 9 to 16 (16-bit big-endian samples), is encoded at depth d;
        decode IN.bit OUT.ppm --depth D writes one.  .y4m: C420pN / C422pN / C444pN for N in 9, 10, 12, 14, 16
        (little-endian, LSB-aligned samples; 4:2:0 left-sited), decode --depth N writes that tag.  Raw .yuv: --depth D
        says the file holds 16-bit little-endian words of D-bit samples, LSB-aligned or, with --msb, MSB-aligned
        (P010 is --yuv nv12 --depth 10 --msb).  --matrix 2020 (BT.2020 non-constant-luminance) needs a depth above
        8.  decode --ref prints the PSNRs at the peak 2^D - 1.  Not together with --tile / --region

Binary PPM (P6, maxval 255 or 2^d - 1) is read and written here; any other format goes through PIL (8-bit) when it
imports.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


# ---------------------------------------------------------------------------------------------- PPM
def _ppm_tokens(data: bytes, count: int):
    """The first `count` whitespace-separated header tokens ('#' comments skipped) and the offset of the byte
    after the single whitespace that ends the last one."""
    toks, pos, n = [], 0, len(data)
    while len(toks) < count:
        while pos < n and data[pos:pos + 1].isspace():
            pos += 1
        if pos < n and data[pos:pos + 1] == b"#":
            while pos < n and data[pos:pos + 1] not in (b"\n", b"\r"):
                pos += 1
            continue
        start = pos
        while pos < n and not data[pos:pos + 1].isspace():
            pos += 1
        if start == pos:
            raise ValueError("PPM: truncated header")
        toks.append(data[start:pos])
    if pos >= n or not data[pos:pos + 1].isspace():
        raise ValueError("PPM: no whitespace after the header")
    return toks, pos + 1


def read_ppm_deep(data: bytes):
    """Binary PPM (P6) bytes -> (image [H, W, 3], depth): uint8 and 8 for maxval 255; for a maxval from 256 to
    65535, which must be 2^depth - 1, uint16 in native byte order (the file's samples are 16-bit big-endian, per
    Netpbm) and that depth."""
    toks, off = _ppm_tokens(data, 4)
    if toks[0] != b"P6":
        raise ValueError("PPM: not a binary P6 file")
    try:
        W, H, maxval = (int(t) for t in toks[1:])
    except ValueError:
        raise ValueError("PPM: header fields are not numbers") from None
    if W < 1 or H < 1:
        raise ValueError(f"PPM: {W} x {H}, maxval {maxval}: a non-empty image expected")
    depth = maxval.bit_length()
    if not 8 <= depth <= 16 or maxval != (1 << depth) - 1:
        raise ValueError(f"PPM: maxval {maxval} is not 2^d - 1 for a depth d in [8, 16]")
    if depth == 8:
        if len(data) - off < H * W * 3:
            raise ValueError("PPM: pixel data truncated")
        return np.frombuffer(data, np.uint8, H * W * 3, off).reshape(H, W, 3).copy(), 8
    if len(data) - off < H * W * 6:
        raise ValueError("PPM: pixel data truncated")
    return np.frombuffer(data, ">u2", H * W * 3, off).reshape(H, W, 3).astype(np.uint16), depth


def read_ppm(data: bytes) -> np.ndarray:
    """Binary PPM (P6, maxval 255) bytes -> uint8 [H, W, 3].  A deeper file is read by read_ppm_deep."""
    img, depth = read_ppm_deep(data)
    if depth != 8:
        raise ValueError(f"PPM: maxval {(1 << depth) - 1}: an 8-bit image expected (read_ppm_deep reads deeper ones)")
    return img


def write_ppm(img: np.ndarray, depth: int = 8) -> bytes:
    """uint8 [H, W, 3] -> binary PPM bytes; or, with depth in 9..16, uint16 [H, W, 3] samples (at most 2^depth - 1)
    -> a PPM of maxval 2^depth - 1 with 16-bit big-endian samples."""
    img = np.ascontiguousarray(img)
    if depth == 8:
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
            raise ValueError(f"PPM: uint8 [H, W, 3] expected, got {img.dtype} {img.shape}")
        return b"P6\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes()
    if not isinstance(depth, int) or not 9 <= depth <= 16:
        raise ValueError(f"PPM: depth must be in [8, 16], got {depth!r}")
    if img.dtype != np.uint16 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f"PPM: uint16 [H, W, 3] expected at depth {depth}, got {img.dtype} {img.shape}")
    maxval = (1 << depth) - 1
    if img.size and int(img.max()) > maxval:
        raise ValueError(f"PPM: a sample above maxval {maxval}")
    return b"P6\n%d %d\n%d\n" % (img.shape[1], img.shape[0], maxval) + img.astype(">u2").tobytes()


def _is_ppm(path: str) -> bool:
    return os.path.splitext(path)[1].lower() in (".ppm", ".pnm")


def load_image(path: str, deep: bool = False):
    """-> uint8 [H, W, 3]; deep=True: (image, depth), uint16 for a PPM of more than 8 bits."""
    if _is_ppm(path):
        with open(path, "rb") as f:
            return read_ppm_deep(f.read()) if deep else read_ppm(f.read())
    try:
        from PIL import Image
    except ImportError:
        raise SystemExit(f"{path}: only binary PPM is read without PIL") from None
    img = np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)
    return (img, 8) if deep else img


def save_image(path: str, img: np.ndarray, depth: int = 8):
    if _is_ppm(path):
        with open(path, "wb") as f:
            f.write(write_ppm(img, depth))
        return
    if depth != 8:
        raise SystemExit(f"{path}: an image of depth {depth} is written as binary PPM only")
    try:
        from PIL import Image
    except ImportError:
        raise SystemExit(f"{path}: only binary PPM is written without PIL") from None
    Image.fromarray(img, "RGB").save(path)


# ---------------------------------------------------------------------------------------------- Y4M
# colour space tag -> (raw layout, (sub_x, sub_y), horizontal chroma siting)
Y4M_TAGS = {"420jpeg": ("i420", (2, 2), "centre"), "420mpeg2": ("i420", (2, 2), "left"), "420": ("i420", (2, 2), "left"),
            "422": ("i422", (2, 1), "left"), "444": ("i444", (1, 1), "left")}


Y4M_DEPTHS = (9, 10, 12, 14, 16)
_Y4M_REFUSAL = ("is not supported (8-bit C420jpeg, C420mpeg2, C420, C422, C444, and C420pN, C422pN, C444pN for N in "
                "9, 10, 12, 14, 16)")


def y4m_tag(tag: str):
    """A colour space tag without its 'C' -> (raw layout, (sub_x, sub_y), siting, depth); ValueError by name for a tag
    that is not supported.  C420pN is left-sited, as plain C420 is."""
    if tag in Y4M_TAGS:
        return Y4M_TAGS[tag] + (8,)
    base, p, n = tag.partition("p")
    if p and base in ("420", "422", "444") and n.isdigit() and int(n) in Y4M_DEPTHS and n == str(int(n)):
        return Y4M_TAGS[base] + (int(n),)
    raise ValueError(f"Y4M: colour space C{tag} {_Y4M_REFUSAL}")


def read_y4m(data: bytes, frame: int = 0, max_depth: int = 8):
    """YUV4MPEG2 bytes -> (y, cb, cr, tag, params): frame `frame` as arrays [H, W] and two chroma planes (the ceil
    rule), the colour space tag without its 'C' ("420jpeg" when the header has none) and the header's other
    parameters as a list of strings.  4:2:0 / 4:2:2 / 4:4:4 only: any other tag is refused by name.  A tag of more
    than max_depth bits is refused too (8 by default: the planes are then uint8); with max_depth=16 a C420p10 file
    gives uint16 planes (the file's samples are little-endian and LSB-aligned)."""
    end = data.find(b"\n")
    if not data.startswith(b"YUV4MPEG2 ") or end < 0:
        raise ValueError("Y4M: not a YUV4MPEG2 file")
    W = H = None
    tag, params = "420jpeg", []
    for tok in data[10:end].decode("ascii", "replace").split():
        if tok[0] == "W" or tok[0] == "H":
            try:
                v = int(tok[1:])
            except ValueError:
                raise ValueError(f"Y4M: bad header field {tok!r}") from None
            W, H = (v, H) if tok[0] == "W" else (W, v)
        elif tok[0] == "C":
            tag = tok[1:]
        else:
            params.append(tok)
    _, (sx, sy), _, depth = y4m_tag(tag)
    if depth > max_depth:
        raise ValueError(f"Y4M: colour space C{tag} is {depth} bits deep, above max_depth {max_depth}")
    if W is None or H is None or W < 1 or H < 1:
        raise ValueError("Y4M: the header needs positive W and H")
    if frame < 0:
        raise ValueError(f"Y4M: frame {frame}")
    ch, cw = (H + sy - 1) // sy, (W + sx - 1) // sx
    ns = H * W + 2 * ch * cw              # samples
    n = ns * (1 if depth == 8 else 2)     # bytes
    pos = end + 1
    for k in range(frame + 1):
        e = data.find(b"\n", pos)
        if not data.startswith(b"FRAME", pos) or e < 0:
            raise ValueError(f"Y4M: no frame {k} (the file ends or the FRAME marker is missing)")
        pos = e + 1
        if len(data) - pos < n:
            raise ValueError(f"Y4M: frame {k} is truncated ({len(data) - pos} of {n} bytes)")
        if k < frame:
            pos += n
    a = np.frombuffer(data, np.uint8, n, pos).copy() if depth == 8 else \
        np.frombuffer(data, "<u2", ns, pos).astype(np.uint16)
    return (a[:H * W].reshape(H, W), a[H * W:H * W + ch * cw].reshape(ch, cw), a[H * W + ch * cw:].reshape(ch, cw), tag,
            params)


def write_y4m(y: np.ndarray, cb: np.ndarray, cr: np.ndarray, tag: str, params=("F25:1", "Ip", "A1:1")) -> bytes:
    """One frame -> YUV4MPEG2 bytes with the colour space tag `tag`: uint8 planes for an 8-bit tag, uint16 planes
    (LSB-aligned samples, written little-endian) for C420pN / C422pN / C444pN."""
    _, (sx, sy), _, depth = y4m_tag(tag)
    H, W = y.shape
    want = ((H + sy - 1) // sy, (W + sx - 1) // sx)
    dt = np.uint8 if depth == 8 else np.uint16
    if any(p.dtype != dt for p in (y, cb, cr)) or cb.shape != want or cr.shape != want:
        raise ValueError(f"Y4M: {np.dtype(dt).name} planes {(H, W)} and two of {want} expected for C{tag} (its depth is "
                         f"{depth})")
    if depth > 8 and any(p.size and int(p.max()) >= 1 << depth for p in (y, cb, cr)):
        raise ValueError(f"Y4M: a sample above {(1 << depth) - 1} in a C{tag} frame")
    head = " ".join(["YUV4MPEG2", f"W{W}", f"H{H}"] + list(params) + [f"C{tag}"])
    return head.encode("ascii") + b"\nFRAME\n" + b"".join(
        np.ascontiguousarray(p).astype(p.dtype if depth == 8 else "<u2").tobytes() for p in (y, cb, cr))


def _ext(path: str) -> str:
    return os.path.splitext(path)[1].lower()


def _is_yuv(path: str) -> bool:
    return _ext(path) in (".y4m", ".yuv")


def _size(v: str):
    try:
        w, h = (int(t) for t in v.lower().split("x"))
    except ValueError:
        w = h = 0
    if w < 1 or h < 1:
        raise argparse.ArgumentTypeError(f"WxH expected, got {v!r}")
    return w, h


def _yuv_format(args, sub, site, depth=None):
    """depth: that of a y4m tag; None: --depth (a raw file's, with --msb)."""
    from mlic_amd import codec
    msb = bool(args.msb) if depth is None else False
    depth = (args.depth or 8) if depth is None else depth
    try:
        return codec.YuvFormat(sub=sub, matrix="bt" + args.matrix, full_range=args.range == "full",
                               site_x=args.chroma_site or site, depth=depth, msb=msb)
    except ValueError as e:
        raise SystemExit(str(e)) from None


def load_yuv(path: str, args, size=None):
    """A .y4m or raw .yuv file -> ((y, cb, cr) numpy planes of frame --frame, YuvFormat).  size: (W, H) of a raw
    file when --size is not given (a decode knows it from the bitstream)."""
    from mlic_amd import codec
    with open(path, "rb") as f:
        data = f.read()
    if _ext(path) == ".y4m":
        try:
            y, cb, cr, tag, _ = read_y4m(data, args.frame, max_depth=16)
        except ValueError as e:
            raise SystemExit(f"{path}: {e}") from None
        _, sub, site, depth = y4m_tag(tag)
        if args.depth is not None and args.depth != depth:
            raise SystemExit(f"{path}: the file is C{tag}, {depth} bits deep, --depth says {args.depth}")
        return (y, cb, cr), _yuv_format(args, sub, site, depth)
    size = args.size or size
    if size is None:
        raise SystemExit(f"{path}: a raw .yuv file needs --size WxH")
    W, H = size
    depth = args.depth or 8
    n = codec.yuv_frame_bytes(H, W, args.yuv, depth)
    if len(data) < (args.frame + 1) * n:
        raise SystemExit(f"{path}: frame {args.frame} of {W}x{H} {args.yuv} at depth {depth} needs "
                         f"{(args.frame + 1) * n} bytes, the file has {len(data)}")
    if depth == 8:
        buf = np.frombuffer(data, np.uint8, n, args.frame * n).copy()
    else:  # little-endian words, as a decoder's P010 surface or an I010 file on disk
        buf = np.frombuffer(data, "<u2", n // 2, args.frame * n).astype(np.uint16)
    return codec.split_yuv(buf, H, W, args.yuv, depth), _yuv_format(args, codec._YUV_SUB[args.yuv], "left")


def save_yuv(path: str, planes, fmt, args):
    """(y, cb, cr) numpy planes -> a .y4m file (planar, the tag from the format) or a raw .yuv file in --yuv."""
    from mlic_amd import codec
    y, cb, cr = planes
    H, W = y.shape
    if _ext(path) == ".y4m":
        if fmt.depth == 8:
            tag = {(2, 2): "420jpeg" if fmt.site_x == "centre" else "420mpeg2", (2, 1): "422", (1, 1): "444"}[fmt.sub]
        else:
            if fmt.msb or fmt.depth not in Y4M_DEPTHS or (fmt.sub == (2, 2) and fmt.site_x != "left"):
                raise SystemExit(f"{path}: a .y4m file holds LSB-aligned samples of {Y4M_DEPTHS} bits, 4:2:0 left-sited; "
                                 f"got {fmt!r}")
            tag = {(2, 2): "420", (2, 1): "422", (1, 1): "444"}[fmt.sub] + f"p{fmt.depth}"
        data = write_y4m(y, cb, cr, tag)
    else:
        buf = np.zeros(codec.yuv_frame_samples(H, W, args.yuv), np.uint8 if fmt.depth == 8 else np.uint16)
        for dst, src in zip(codec.split_yuv(buf, H, W, args.yuv, fmt.depth), planes):
            dst[...] = src
        data = buf.tobytes() if fmt.depth == 8 else buf.astype("<u2").tobytes()
    with open(path, "wb") as f:
        f.write(data)


# -------------------------------------------------------------------------------------------- model
def load_model(args):
    import torch
    from mlic_amd import get_model, synthetic
    if not torch.cuda.is_available():
        raise SystemExit("mlic_codec needs a HIP device")
    net = get_model(args.model)
    if args.checkpoint:
        sd = torch.load(args.checkpoint, map_location="cpu")
        sd = sd.get("state_dict", sd) if isinstance(sd, dict) else sd
    else:
        sd = synthetic.synth_state_dict(args.model, args.synthetic)
    net.load_state_dict(sd)
    net = net.to(torch.device("cuda:0")).eval()
    net.update()
    return net


def _level(v: str):
    if v == "auto":
        return v
    try:
        n = int(v)
    except ValueError:
        n = -1
    if n < 0:
        raise argparse.ArgumentTypeError(f"a level number or 'auto' expected, got {v!r}")
    return n


def _budget(v: str) -> float:
    try:
        x = float(v)
    except ValueError:
        x = 0.0
    if not (x > 0 and x != float("inf")):
        raise argparse.ArgumentTypeError(f"a positive finite number of bits per pixel expected, got {v!r}")
    return x


def _full_scale(v: str) -> float:
    try:
        return _budget(v)
    except argparse.ArgumentTypeError:
        raise argparse.ArgumentTypeError(f"a positive finite value expected, got {v!r}") from None


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["encode", "decode", "info", "ratemap", "truncate", "strip"])
    ap.add_argument("src")
    ap.add_argument("dst", nargs="?")
    ap.add_argument("--model", default="MLICPP_L")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--checkpoint")
    g.add_argument("--synthetic", type=int, metavar="SEED")
    ap.add_argument("--level", type=_level, default=None, metavar="N|auto")
    ap.add_argument("--max-bpp", type=_budget, default=None, metavar="X")
    ap.add_argument("--max-passes", type=int, default=8, metavar="N")
    ap.add_argument("--roi", default=None, metavar="MASK")
    ap.add_argument("--roi-levels", type=int, nargs=2, default=None, metavar=("LO", "HI"))
    ap.add_argument("--tile", type=int, default=None, metavar="T")
    ap.add_argument("--overlap", type=int, default=None, metavar="V")
    ap.add_argument("--tile-batch", type=int, default=8, metavar="N")
    ap.add_argument("--region", type=int, nargs=4, default=None, metavar=("Y0", "X0", "H", "W"))
    ap.add_argument("--yuv", choices=["i420", "nv12", "nv21", "yv12", "i422", "i444"], default=None)
    ap.add_argument("--size", type=_size, default=None, metavar="WxH")
    ap.add_argument("--matrix", choices=["601", "709", "2020"], default="709")
    ap.add_argument("--depth", type=int, default=None, metavar="D")
    ap.add_argument("--msb", action="store_true")
    ap.add_argument("--range", choices=["full", "limited"], default="limited")
    ap.add_argument("--chroma-site", choices=["left", "centre"], default=None)
    ap.add_argument("--frame", type=int, default=0, metavar="N")
    ap.add_argument("--ref", default=None, metavar="SRC")
    ap.add_argument("--scale", default=None, metavar="N/D")
    ap.add_argument("--coded-size", type=_size, default=None, metavar="WxH")
    ap.add_argument("--filter", choices=["lanczos3", "bicubic", "triangle"], default=None)
    ap.add_argument("--out-size", type=_size, default=None, metavar="WxH")
    ap.add_argument("-o", "--output", default=None, metavar="HEAT")
    ap.add_argument("--what", nargs="+", default=None, metavar="bits|slice K|z|error")
    ap.add_argument("--cmap", choices=["hot", "gray"], default=None)
    ap.add_argument("--alpha", type=int, default=None, metavar="A")
    ap.add_argument("--hi", type=_full_scale, default=None, metavar="X")
    ap.add_argument("--csv", default=None, metavar="FILE")
    ap.add_argument("--layered", action="store_true")
    ap.add_argument("--slices", type=int, default=None, metavar="K")
    ap.add_argument("--fill", choices=["mean", "zero"], default=None)
    ap.add_argument("-k", "--keep", type=int, default=None, metavar="K")
    ap.add_argument("--max-error", type=int, default=None, metavar="T")
    ap.add_argument("--lossless", action="store_true")
    ap.add_argument("--base-only", action="store_true")
    ap.add_argument("--residual-segment", type=int, default=None, metavar="L")
    ap.add_argument("--residual-coder", choices=["host", "device"], default=None)
    ap.add_argument("--residual-shift", type=int, default=None, metavar="S")
    ap.add_argument("--frame-max-error", type=int, default=None, metavar="T")
    ap.add_argument("--frame-lossless", action="store_true")
    args = ap.parse_args(argv)
    if args.mode == "strip":
        if args.dst is not None or args.output is None:
            ap.error("strip takes one residual file and -o OUT")
        given = {k: v for k, v in vars(args).items() if k not in ("mode", "src", "dst", "output", "model")}
        if given != {k: ap.get_default(k) for k in given}:
            ap.error("strip goes with -o alone (it needs no model)")
        args.frame_file = False
        return args
    if args.lossless:
        if args.max_error not in (None, 0):
            ap.error("--lossless is --max-error 0")
        args.max_error = 0
    if args.frame_lossless:
        if args.frame_max_error not in (None, 0):
            ap.error("--frame-lossless is --frame-max-error 0")
        args.frame_max_error = 0
    if args.frame_max_error is not None:
        if args.mode != "encode":
            ap.error("--frame-max-error / --frame-lossless go with encode (a residual file is recognised by its magic)")
        if args.max_error is not None:
            ap.error("--frame-max-error / --frame-lossless and --max-error / --lossless do not go together")
        if not _is_yuv(args.src):
            ap.error("--frame-max-error / --frame-lossless go with a .y4m or .yuv source (an image file takes "
                     "--max-error / --lossless)")
        if not 0 <= args.frame_max_error <= 127:
            ap.error("--frame-max-error: 0 to 127 expected")
        if args.max_bpp is not None or args.level == "auto" or args.roi is not None or args.roi_levels is not None or \
                args.tile is not None or args.scale is not None or args.coded_size is not None or args.layered:
            ap.error("--frame-max-error goes with --level N alone, not with --max-bpp, --level auto, --roi, --tile, "
                     "--scale, --coded-size or --layered")
    if args.residual_segment is not None:
        if args.max_error is None and args.frame_max_error is None:
            ap.error("--residual-segment goes with encode --max-error T / --lossless")
        if not 256 <= args.residual_segment <= 65536:
            ap.error("--residual-segment: 256 to 65536 expected")
    if args.residual_coder is not None and args.mode == "encode" and args.residual_segment is None and \
            args.frame_max_error is None:  # a frame's residual file is always segmented
        ap.error("--residual-coder goes with --residual-segment L (encode) or with decode")
    if args.residual_coder is not None and args.mode not in ("encode", "decode"):
        ap.error("--residual-coder goes with encode and decode")
    if args.residual_shift is not None:
        if args.mode != "encode" or (args.max_error is None and args.frame_max_error is None):
            ap.error("--residual-shift goes with encode --max-error T / --lossless of an image deeper than 8 bits")
        if not 0 <= args.residual_shift <= 9:
            ap.error("--residual-shift: 0 to depth - 7 expected")
    if args.max_error is not None:
        if args.mode != "encode":
            ap.error("--max-error / --lossless go with encode (a residual file is recognised by its magic)")
        if not 0 <= args.max_error <= 127:
            ap.error("--max-error: 0 to 127 expected")
        if args.max_bpp is not None or args.level == "auto" or args.roi is not None or args.roi_levels is not None or \
                args.tile is not None or args.scale is not None or args.coded_size is not None or args.layered or \
                _is_yuv(args.src):
            ap.error("--max-error goes with --level N alone, not with --max-bpp, --level auto, --roi, --tile, --scale, "
                     "--coded-size, --layered or Y'CbCr frames")
    if args.base_only:
        if args.mode != "decode":
            ap.error("--base-only goes with decode")
        if args.slices is not None or args.fill is not None or args.out_size is not None or args.filter is not None or \
                args.region is not None or (args.depth is not None and not _is_yuv(args.dst or "")):
            ap.error("--base-only goes alone: a residual file takes no --slices, --fill, --out-size, --filter, --region "
                     "or --depth")
    if args.mode == "truncate":
        if args.dst is not None or args.output is None or args.keep is None or args.keep < 0:
            ap.error("truncate takes one layered file, -k K (the layers to keep, not negative) and -o OUT")
        given = {k: v for k, v in vars(args).items() if k not in ("mode", "src", "dst", "output", "keep", "model")}
        defaults = {k: ap.get_default(k) for k in given}
        if given != defaults:
            ap.error("truncate goes with -k and -o alone (it needs no model)")
        args.frame_file = False
        return args
    if args.keep is not None:
        ap.error("-k goes with truncate")
    if args.layered:
        if args.mode != "encode":
            ap.error("--layered goes with encode (a layered file is recognised by its magic)")
        if args.max_bpp is not None or args.level == "auto" or args.roi is not None or args.roi_levels is not None or \
                args.tile is not None or args.scale is not None or args.coded_size is not None or _is_yuv(args.src):
            ap.error("--layered goes with --level N alone, not with --max-bpp, --level auto, --roi, --tile, --scale, "
                     "--coded-size or Y'CbCr frames")
    if args.slices is not None or args.fill is not None:
        if args.mode != "decode":
            ap.error("--slices and --fill go with decode")
        if args.slices is not None and args.slices < 0:
            ap.error("--slices must not be negative")
        if args.out_size is not None or args.region is not None or _is_yuv(args.dst or ""):
            ap.error("--slices / --fill together with --out-size, --region or Y'CbCr frames are not supported")
    map_flags = [args.output, args.what, args.cmap, args.alpha, args.hi, args.csv]
    if args.mode != "ratemap":
        if any(v is not None for v in map_flags):
            ap.error("-o, --what, --cmap, --alpha, --hi and --csv go with ratemap")
    else:
        if args.dst is not None or args.output is None:
            ap.error("ratemap takes one image and -o HEAT")
        if _is_yuv(args.src):
            ap.error("ratemap of a Y'CbCr frame is not supported")
        other = [args.max_bpp, args.tile, args.overlap, args.region, args.yuv, args.size, args.depth, args.chroma_site,
                 args.ref, args.scale, args.coded_size, args.filter, args.out_size]
        if any(v is not None for v in other) or args.level == "auto" or args.msb or args.frame != 0:
            ap.error("ratemap goes with --level N or --roi MASK --roi-levels LO HI alone: maps of rate-constrained, "
                     "tiled, scaled, Y'CbCr or deeper-than-8-bit coding are not supported")
        what = args.what or ["bits"]
        if what[0] == "slice" and len(what) == 2 and what[1].isdigit():
            args.what = ("slice", int(what[1]))
        elif len(what) == 1 and what[0] in ("bits", "z", "error"):
            args.what = (what[0], None)
        else:
            ap.error("--what: bits, slice K, z or error expected")
        args.cmap = args.cmap or "hot"
        args.alpha = 256 if args.alpha is None else args.alpha
        if not 0 <= args.alpha <= 256:
            ap.error("--alpha: 0 to 256 expected")
    scaling = args.scale is not None or args.coded_size is not None
    frame_file = args.mode != "info" and _is_yuv(args.src if args.mode == "encode" else (args.dst or ""))
    if frame_file:
        if args.roi is not None or args.roi_levels is not None or args.tile is not None or args.region is not None:
            ap.error("ROI and tiled coding together with Y'CbCr frames are not supported")
        if args.frame < 0:
            ap.error("--frame must not be negative")
        if args.yuv is None:
            args.yuv = "i420"
    elif args.yuv is not None or args.size is not None or args.chroma_site is not None or args.frame != 0 or args.msb:
        ap.error("--yuv, --size, --chroma-site, --frame and --msb go with a .y4m or .yuv frame file")
    if args.depth is not None and not 8 <= args.depth <= 16:
        ap.error("--depth: 8 to 16 expected")
    if args.msb and (args.depth is None or args.depth == 8):
        ap.error("--msb goes with --depth above 8 (a raw .yuv file of MSB-aligned 16-bit words, P010 style)")
    if args.depth is not None and not frame_file and args.mode != "decode":
        ap.error("--depth goes with a raw .yuv frame file, or with decode (an image file knows its own depth)")
    if args.matrix == "2020" and frame_file and args.mode == "encode" and _ext(args.src) == ".yuv" and \
            (args.depth or 8) == 8:
        ap.error("--matrix 2020 needs --depth above 8")
    if (args.depth or 8) > 8 and (args.tile is not None or args.region is not None):
        ap.error("tiled coding at a depth above 8 is not supported (the blend kernel writes bytes)")
    if args.ref is not None and not (frame_file and args.mode == "decode"):
        ap.error("--ref goes with decode to a .y4m or .yuv file")
    args.frame_file = frame_file
    if scaling or args.out_size is not None:
        if args.scale is not None and args.coded_size is not None:
            ap.error("--scale and --coded-size are two ways to say one thing: pass one")
        if scaling and args.mode != "encode":
            ap.error("--scale and --coded-size go with encode (a scaled file is recognised by its magic)")
        if args.out_size is not None and args.mode != "decode":
            ap.error("--out-size goes with decode")
        if frame_file or args.roi is not None or args.tile is not None or args.region is not None or (args.depth or 8) > 8:
            ap.error("scaled coding together with Y'CbCr frames, ROI, tiles or a depth above 8 is not supported")
        if args.scale is not None:
            from fractions import Fraction
            try:
                args.scale = Fraction(args.scale)
            except (ValueError, ZeroDivisionError):
                ap.error("--scale: a fraction N/D expected")
            if not Fraction(1, 8) <= args.scale <= 8:
                ap.error("--scale: 1/8 to 8 expected")
    elif args.filter is not None and args.mode != "decode":
        ap.error("--filter goes with --scale, --coded-size or decode")
    if args.tile is not None:
        if args.mode != "encode":
            ap.error("--tile goes with encode (a tiled file is recognised by its magic)")
        if args.max_bpp is not None or args.level == "auto" or args.roi is not None or args.roi_levels is not None:
            ap.error("--tile goes with --level N alone, not with --max-bpp, --level auto or --roi")
        if args.tile % 64 or args.tile < 128:
            ap.error("--tile: a multiple of 64, at least 128, expected")
    elif args.overlap is not None:
        ap.error("--overlap goes with --tile")
    if args.overlap is None:
        args.overlap = 32
    if args.overlap not in (0, 16, 32, 64) or (args.tile is not None and args.overlap > args.tile // 2):
        ap.error("--overlap: 0, 16, 32 or 64, at most half the tile, expected")
    if args.tile_batch < 1:
        ap.error("--tile-batch must be positive")
    if args.region is not None and args.mode != "decode":
        ap.error("--region goes with decode")
    if args.mode in ("encode", "decode") and args.dst is None:
        ap.error(f"{args.mode} needs a destination file")
    if args.mode != "info" and args.checkpoint is None and args.synthetic is None:
        ap.error("one of the arguments --checkpoint --synthetic is required")
    if args.mode == "info" and args.dst is not None:
        ap.error("info takes one file")
    if (args.roi is None) != (args.roi_levels is None):
        ap.error("--roi and --roi-levels go together")
    if args.roi is not None:
        if args.mode not in ("encode", "ratemap"):
            ap.error("--roi goes with encode (a decode reads the map from the file)")
        if args.max_bpp is not None or args.level is not None:
            ap.error("--roi goes with --roi-levels alone, not with --level or --max-bpp")
        if not 0 <= args.roi_levels[0] <= args.roi_levels[1]:
            ap.error("--roi-levels: 0 <= LO <= HI expected")
    if args.level == "auto" and args.max_bpp is None:
        ap.error("--level auto needs --max-bpp")
    if args.max_passes < 0:
        ap.error("--max-passes must not be negative")
    if args.mode == "decode" and args.max_bpp is not None:
        ap.error("--max-bpp goes with encode")
    return args


def _map_lines(lv) -> str:
    return "\n".join("  " + " ".join(f"{int(v):x}" for v in row) for row in lv)


def _ratemap(args):
    """ratemap IMAGE -o HEAT: codec.rate_map of the image, one plane of it through codec.heat_u8."""
    import torch
    from mlic_amd import codec
    img, depth = load_image(args.src, deep=True)
    if depth != 8:
        raise SystemExit(f"{args.src}: ratemap of an image deeper than 8 bits is not supported")
    H, W = img.shape[:2]
    roi = None
    if args.roi is not None:
        roi = np.ascontiguousarray(load_image(args.roi)[:, :, 0])
        if roi.shape != (H, W):
            raise SystemExit(f"{args.roi}: the mask is {roi.shape[0]} x {roi.shape[1]}, the image {H} x {W}")
    net = load_model(args)
    dev_img = torch.from_numpy(img).to(net.device)
    try:
        r = codec.rate_map(net, dev_img, level=args.level, layout="hwc", roi=roi,
                           roi_levels=None if roi is None else tuple(args.roi_levels))[0]
    except ValueError as e:
        raise SystemExit(f"{args.src}: {e}") from None
    kind, k = args.what
    if kind == "bits":
        plane, cell, name = r["cell_bits"], 16, "bits per 16 x 16 cell"
    elif kind == "slice":
        if k >= r["y_map"].size(0):
            raise SystemExit(f"--what slice {k}: the model has {r['y_map'].size(0)} slices")
        plane, cell, name = r["y_map"][k], 16, f"bits of slice {k} per 16 x 16 cell"
    elif kind == "z":
        plane, cell, name = r["z_map"], 64, "bits of z per 64 x 64 cell"
    else:
        dec = codec.egress_u8(r["x_hat"].unsqueeze(0), H, W, "hwc")
        plane, cell, name = codec.sq_err_blocks(dev_img, dec, block=16, layout="hwc")[0].double(), 16, \
            "squared error per 16 x 16 block"
    plane = plane[:-(-H // cell), :-(-W // cell)].contiguous()  # the cells that show in the image
    heat = codec.heat_u8(plane, H, W, cell, 0.0, args.hi, args.cmap, under=dev_img if args.alpha < 256 else None,
                         alpha=args.alpha, layout="hwc")
    save_image(args.output, heat[0].cpu().numpy())
    sb = r["slice_bits"].cpu().tolist()
    if args.csv is not None:
        with open(args.csv, "w") as f:
            f.write("slice_bits," + ",".join(repr(v) for v in sb[:-1]) + "\n")
            f.write("z_bits," + repr(sb[-1]) + "\n")
            f.write(f"plane,{kind if k is None else f'{kind} {k}'},cell,{cell}\n")
            for row in plane.cpu().tolist():
                f.write(",".join(repr(v) for v in row) + "\n")
    print(f"{args.src}: {H} x {W}, {r['bits']:.1f} bits, {r['bpp']:.4f} bpp (y slices " +
          " ".join(f"{v:.0f}" for v in sb[:-1]) + f", z {sb[-1]:.0f}); {name}, maximum {float(plane.max()):.3f} -> "
          f"{args.output}")


def main(argv=None):
    args = parse_args(argv)
    from mlic_amd import codec
    if args.mode == "ratemap":
        return _ratemap(args)
    if args.mode == "truncate":
        with open(args.src, "rb") as f:
            data = f.read()
        if not codec.is_layered_file(data):
            raise SystemExit(f"{args.src}: not a layered file (no MLL1 magic): encode --layered writes one")
        try:
            cut = codec.truncate_layered(data, args.keep)
        except ValueError as e:
            raise SystemExit(f"{args.src}: {e}") from None
        with open(args.output, "wb") as f:
            f.write(cut)
        print(f"{args.src}: {len(data)} bytes -> {args.output}: {len(cut)} bytes, {args.keep} layers")
        return
    if args.mode == "strip":
        with open(args.src, "rb") as f:
            data = f.read()
        if not (codec.is_residual_file(data) or codec.is_residual_deep_file(data) or codec.is_residual_yuv_file(data)):
            raise SystemExit(f"{args.src}: not a residual file (no MLR1 / MLR2 magic): encode --max-error T writes one")
        inner = codec.strip_residual(data)
        with open(args.output, "wb") as f:
            f.write(inner)
        print(f"{args.src}: {len(data)} bytes -> {args.output}: {len(inner)} bytes (the base file)")
        return
    if args.mode == "info":
        from mlic_amd import spec
        with open(args.src, "rb") as f:
            data = f.read()
        vbr = bool(spec.get_config(args.model).vbr)
        if codec.is_tiled_file(data):  # the file's own flag against the model, before any tile is parsed
            flag = bool(codec.parse_container_tiled(data).vbr)
            if flag != vbr:
                raise SystemExit(f"{args.src}: the tiles {'carry a' if flag else 'have no'} level word, "
                                 f"{args.model} is {'variable' if vbr else 'fixed'}-rate")
        d = codec.peek(data, vbr=vbr, n_levels=len(spec.vbr_lambdas(args.model)) if vbr else None)
        if d.get("layered"):
            if d["vbr"] != vbr:
                raise SystemExit(f"{args.src}: the file {'carries a' if d['vbr'] else 'has no'} level word, "
                                 f"{args.model} is {'variable' if vbr else 'fixed'}-rate")
            print(f"{args.src}: {d['H']} x {d['W']}, layered: {d['layers_present']} of {d['slices']} layers"
                  f"{'' if d['layers_present'] == d['slices'] else ' (truncated)'}, level {d['level']}, z grid "
                  f"{d['shape'][0]} x {d['shape'][1]}, z {d['z_len']} B, {d['bytes']} bytes, {d['bpp']:.4f} bpp")
            at = d["header_bytes"] + d["z_len"]
            for k, n in enumerate(d["layer_bytes"]):
                at += 4 + n
                print(f"  layer {k}: {n} B, file up to here {at} B, {8.0 * at / (d['H'] * d['W']):.4f} bpp")
            return
        if d.get("tiled"):
            print(f"{args.src}: {d['H']} x {d['W']}, tiled: tile {d['tile']}, overlap {d['overlap']}, grid "
                  f"{d['grid'][0]} x {d['grid'][1]}, level {d['level']}, {d['bytes']} bytes, {d['bpp']:.4f} bpp")
            for t in d["tiles"]:
                print(f"  tile {t['index']}: at ({t['y0']}, {t['x0']}), {t['H']} x {t['W']}, {t['bytes']} bytes, "
                      f"{t['bpp']:.4f} bpp")
            return
        if d.get("residual"):
            if d["vbr"] != vbr:
                raise SystemExit(f"{args.src}: the inner file {'carries a' if d['vbr'] else 'has no'} level word, "
                                 f"{args.model} is {'variable' if vbr else 'fixed'}-rate")
            print(f"{args.src}: {d['H']} x {d['W']}, residual: max error {d['max_error']}"
                  f"{' (lossless)' if d['max_error'] == 0 else ''}, level {d['level']}, z grid {d['shape'][0]} x "
                  f"{d['shape'][1]}, base {d['base_bytes']} B, residual {d['residual_bytes']} B"
                  + (f" in {d['segments']} segments of {d['residual_segment']}" if "segments" in d else "") +
                  (f", depth {d['depth']}, low bits {d['low_bytes']} B (shift {d['shift']})" if "shift" in d else "") +
                  (f", Y'CbCr frame: sub {d['sub'][0]}x{d['sub'][1]}, matrix {d['matrix']}, "
                   f"{'full' if d['full_range'] else 'limited'} range, chroma sited {d['site_x']}" if "sub" in d else "") +
                  f", header and tables {d['header_bytes']} B, {d['bytes']} bytes, {d['bpp']:.4f} bpp")
            return
        if d.get("scaled"):
            print(f"{args.src}: {d['H']} x {d['W']}, scaled: coded at {d['coded'][0]} x {d['coded'][1]}, filter "
                  f"{d['filter']}, level {d['level']}, z grid {d['shape'][0]} x {d['shape'][1]}, y {d['y_len']} B, "
                  f"z {d['z_len']} B, {d['bytes']} bytes, {d['bpp']:.4f} bpp")
            return
        print(f"{args.src}: {d['H']} x {d['W']}, level {d['level']}, z grid {d['shape'][0]} x {d['shape'][1]}, "
              f"y {d['y_len']} B, z {d['z_len']} B, {d['bytes']} bytes, {d['bpp']:.4f} bpp")
        if "roi_levels" in d:
            print(f"level map ({d['shape'][0]} x {d['shape'][1]} cells of 64 x 64 pixels):\n" + _map_lines(d["roi_levels"]))
        return
    if args.mode == "encode" and args.frame_file:
        planes, fmt = load_yuv(args.src, args)
        net = load_model(args)
        if args.frame_max_error is not None:  # the "MLR4" file: every sample of every plane within the bound
            if args.residual_shift is not None and fmt.depth == 8:
                raise SystemExit(f"{args.src}: --residual-shift goes with a frame deeper than 8 bits")
            try:
                files, info = codec.encode_residual_yuv(
                    net, *planes, fmt, max_error=args.frame_max_error, level=args.level,
                    residual_segment=args.residual_segment or codec.DEFAULT_RESIDUAL_SEGMENT,
                    residual_shift=args.residual_shift, residual_coder=args.residual_coder or "device",
                    return_info=True)
            except ValueError as e:
                raise SystemExit(f"{args.src}: {e}") from None
            with open(args.dst, "wb") as f:
                f.write(files[0])
            d = info[0]
            H, W = planes[0].shape
            print(f"{args.src}: {H} x {W} {fmt!r} -> {len(files[0])} bytes, {d['bpp']:.4f} bpp, max error "
                  f"{args.frame_max_error}: base {d['base_bytes']} B, residual {d['residual_bytes']} B in {d['segments']} "
                  f"segments of {d['residual_segment']}, low bits {d['low_bytes']} B (shift {d['shift']})")
            return
        files, info = codec.encode_yuv(net, *planes, fmt, level=args.level, max_bpp=args.max_bpp,
                                       max_passes=args.max_passes, return_info=True)
        with open(args.dst, "wb") as f:
            f.write(files[0])
        H, W = planes[0].shape
        line = f"{args.src}: {H} x {W} {fmt!r} -> {len(files[0])} bytes, {info[0]['bpp']:.4f} bpp"
        if args.max_bpp is not None:
            line += (f", {info[0]['passes']} passes, level {info[0]['level']}, budget {args.max_bpp:g} bpp "
                     f"{'met' if info[0]['met'] else 'not met'}")
        print(line)
        return
    if args.mode == "decode" and args.frame_file:
        with open(args.src, "rb") as f:
            data = f.read()
        if codec.is_tiled_file(data):
            raise SystemExit(f"{args.src}: a tiled file decodes to an RGB image, not to Y'CbCr planes")
        net = load_model(args)
        fmt = _yuv_format(args, codec._YUV_SUB[args.yuv], "left")
        res_yuv = codec.is_residual_yuv_file(data)
        if args.base_only and not res_yuv:
            raise SystemExit(f"{args.src}: --base-only needs a residual file (encode --frame-max-error T)")
        if res_yuv:  # the file knows its format; the alignment of a raw file's words stays the caller's
            fmt = codec.residual_yuv_format(data, msb=args.msb)
            if args.depth is not None and args.depth != fmt.depth:
                raise SystemExit(f"{args.src}: --depth {args.depth}, but the file (MLR4) holds samples of depth {fmt.depth}")
            want = codec._YUV_SUB[args.yuv]
            if _ext(args.dst) == ".yuv" and want != fmt.sub:
                raise SystemExit(f"{args.src}: --yuv {args.yuv} is {want[0]}x{want[1]} subsampled, the file (MLR4) holds "
                                 f"{fmt.sub[0]}x{fmt.sub[1]}")
        if _ext(args.dst) == ".y4m" and args.msb:
            raise SystemExit(f"{args.dst}: a .y4m file holds LSB-aligned samples (--msb goes with a raw .yuv file)")
        ref = None
        if args.ref is not None:
            d = codec.peek(data, vbr=hasattr(net, "levels"))
            ref, rfmt = load_yuv(args.ref, args, size=(d["W"], d["H"]))
            if _ext(args.ref) == ".y4m" and not res_yuv:
                fmt = rfmt  # the source's subsampling and siting
        rkw = {}
        if res_yuv:
            rkw = {"enhance": not args.base_only, "residual_coder": args.residual_coder or "device"}
        try:
            planes, info = codec.decode_yuv(net, [data], fmt, ref=ref, **rkw)
        except ValueError as e:
            if not res_yuv:
                raise
            raise SystemExit(f"{args.src}: {e}") from None
        save_yuv(args.dst, [p[0].cpu().numpy() for p in planes], fmt, args)
        line = f"{args.src}: {info[0]['H']} x {info[0]['W']}, level {info[0]['level']}, {info[0]['bpp']:.4f} bpp, {fmt!r}"
        if "max_error" in info[0]:
            line += (f", max error {info[0]['max_error']}, residual {info[0]['residual_bytes']} B"
                     f"{' (base only)' if args.base_only else ''}")
        if ref is not None:
            line += (f"\nPSNR Y {info[0]['psnr_y']:.4f} dB, U {info[0]['psnr_u']:.4f} dB, V {info[0]['psnr_v']:.4f} dB, "
                     f"YUV (6:1:1) {info[0]['psnr_yuv']:.4f} dB")
        print(line)
        return
    if args.mode == "encode":
        img, depth = load_image(args.src, deep=True)
        deep = {} if depth == 8 else {"depth": depth}  # a PPM's samples are LSB-aligned
        net = load_model(args)
        if args.tile is not None:
            try:
                data, info = codec.encode_tiled(net, img, tile=args.tile, overlap=args.overlap, level=args.level,
                                                layout="hwc", tile_batch=args.tile_batch, return_info=True, **deep)
            except ValueError as e:
                raise SystemExit(f"{args.src}: {e}") from None
            with open(args.dst, "wb") as f:
                f.write(data)
            print(f"{args.src}: {img.shape[0]} x {img.shape[1]} -> {len(data)} bytes, {info['bpp']:.4f} bpp, tile "
                  f"{args.tile}, overlap {args.overlap}, grid {info['grid'][0]} x {info['grid'][1]}")
            return
        roi = None
        if args.roi is not None:
            roi = np.ascontiguousarray(load_image(args.roi)[:, :, 0])
            if roi.shape != img.shape[:2]:
                raise SystemExit(f"{args.roi}: the mask is {roi.shape[0]} x {roi.shape[1]}, the image "
                                 f"{img.shape[0]} x {img.shape[1]}")
        scaled = {}
        if args.scale is not None or args.coded_size is not None:
            if depth != 8:
                raise SystemExit(f"{args.src}: scaled coding of an image deeper than 8 bits is not supported")
            scaled = {"scale": args.scale, "filter": args.filter or "lanczos3",
                      "coded_size": None if args.coded_size is None else (args.coded_size[1], args.coded_size[0])}
        if args.residual_shift is not None and depth == 8:
            raise SystemExit(f"{args.src}: --residual-shift goes with an image deeper than 8 bits")
        if args.max_error is not None and depth != 8:  # samples of 9..16 bits: the "MLR3" file, always segmented
            try:
                files, info = codec.encode_residual16(
                    net, img, depth, max_error=args.max_error, level=args.level, layout="hwc",
                    residual_segment=args.residual_segment or codec.DEFAULT_RESIDUAL_SEGMENT,
                    residual_coder=args.residual_coder or "device", shift=args.residual_shift, return_info=True)
            except ValueError as e:
                raise SystemExit(f"{args.src}: {e}") from None
            with open(args.dst, "wb") as f:
                f.write(files[0])
            d = info[0]
            print(f"{args.src}: {img.shape[0]} x {img.shape[1]} -> {d['bytes']} bytes, {d['bpp']:.4f} bpp, depth {depth}, "
                  f"max error {args.max_error}: base {d['base_bytes']} B, residual {d['residual_bytes']} B in "
                  f"{d['segments']} segments of {d['residual_segment']}, low bits {d['low_bytes']} B (shift {d['shift']})")
            return
        try:
            files, info = codec.encode_images(net, img, level=args.level, layout="hwc", max_bpp=args.max_bpp,
                                              max_passes=args.max_passes, return_info=True, roi=roi,
                                              roi_levels=None if roi is None else tuple(args.roi_levels), **deep, **scaled,
                                              **({"layered": True} if args.layered else {}),
                                              **({} if args.max_error is None else {"max_error": args.max_error}),
                                              **({} if args.residual_segment is None else
                                                 {"residual_segment": args.residual_segment,
                                                  "residual_coder": args.residual_coder or "device"}))
        except ValueError as e:
            if not scaled:
                raise
            raise SystemExit(f"{args.src}: {e}") from None
        data = files[0]
        with open(args.dst, "wb") as f:
            f.write(data)
        line = (f"{args.src}: {img.shape[0]} x {img.shape[1]} -> {len(data)} bytes, "
                f"{8.0 * len(data) / (img.shape[0] * img.shape[1]):.4f} bpp")
        if depth != 8:
            line += f", depth {depth}"
        if scaled:
            line += f", coded at {info[0]['coded'][0]} x {info[0]['coded'][1]} ({info[0]['filter']})"
        if args.layered:
            line += ", layered: " + " ".join(str(n) for n in info[0]["layer_bytes"]) + " B per slice"
        if args.max_error is not None:
            line += (f", max error {args.max_error}: base {info[0]['base_bytes']} B, residual "
                     f"{info[0]['residual_bytes']} B")
            if args.residual_segment is not None:
                line += f" in {info[0]['segments']} segments of {args.residual_segment}"
        if args.max_bpp is not None:
            line += (f", {info[0]['passes']} passes, level {info[0]['level']}, budget {args.max_bpp:g} bpp "
                     f"{'met' if info[0]['met'] else 'not met'}")
        if roi is not None:
            line += f", ROI levels {args.roi_levels[0]}..{args.roi_levels[1]}:\n" + _map_lines(info[0]["roi_levels"])
        print(line)
    else:
        with open(args.src, "rb") as f:
            data = f.read()
        net = load_model(args)
        if codec.is_tiled_file(data):
            if args.slices is not None or args.fill is not None:
                raise SystemExit(f"{args.src}: --slices / --fill on a tiled file are not supported")
            img, info = codec.decode_tiled(net, data, region=args.region, tile_batch=args.tile_batch)
            save_image(args.dst, img.cpu().numpy())
            y0, x0, h, w = info["region"]
            print(f"{args.src}: {info['H']} x {info['W']}, level {info['level']}, {info['bpp']:.4f} bpp, region "
                  f"{h} x {w} at ({y0}, {x0}), {len(info['tiles_decoded'])} of {info['grid'][0] * info['grid'][1]} tiles "
                  f"decoded")
            return
        if args.region is not None:
            raise SystemExit(f"{args.src}: --region needs a tiled file (encode --tile T)")
        depth = args.depth or 8
        if codec.is_residual_deep_file(data):  # the file knows its depth
            depth = codec.peek(data, n_levels=getattr(net, "levels", None))["depth"]
            if args.depth not in (None, depth):
                raise SystemExit(f"{args.src}: --depth {args.depth}, but the file holds samples of depth {depth}")
        kw = {} if depth == 8 or codec.is_residual_deep_file(data) else {"depth": depth}
        if args.out_size is not None:
            kw["out_size"] = (args.out_size[1], args.out_size[0])
        if args.filter is not None:
            kw["filter"] = args.filter
        if args.slices is not None:
            kw["slices"] = args.slices
        if args.fill is not None:
            kw["fill"] = args.fill
        if args.base_only:
            if not (codec.is_residual_file(data) or codec.is_residual_deep_file(data)):
                raise SystemExit(f"{args.src}: --base-only needs a residual file (encode --max-error T)")
            kw["enhance"] = False
        if args.residual_coder is not None:
            kw["residual_coder"] = args.residual_coder
        try:
            img, info = codec.decode_images(net, [data], **kw)
        except ValueError as e:
            if not (args.out_size or args.filter or codec.is_scaled_file(data) or args.slices is not None or
                    args.fill is not None or codec.is_layered_file(data) or codec.is_residual_file(data) or
                    codec.is_residual_deep_file(data)):
                raise
            raise SystemExit(f"{args.src}: {e}") from None
        save_image(args.dst, img[0].cpu().numpy(), depth)
        line = f"{args.src}: {info[0]['H']} x {info[0]['W']}, level {info[0]['level']}, {info[0]['bpp']:.4f} bpp"
        if "coded" in info[0]:
            line += (f", display {info[0]['display'][0]} x {info[0]['display'][1]}, coded at {info[0]['coded'][0]} x "
                     f"{info[0]['coded'][1]} ({info[0]['filter']})")
        if "max_error" in info[0]:
            line += (f", max error {info[0]['max_error']}, residual {info[0]['residual_bytes']} B"
                     f"{' (base only)' if args.base_only else ''}")
            if "shift" in info[0]:
                line += f", depth {info[0]['depth']}, low bits {info[0]['low_bytes']} B (shift {info[0]['shift']})"
        if "slices" in info[0]:
            line += f", {info[0]['slices']} slices decoded ({args.fill or 'mean'} fill)"
        print(line)


if __name__ == "__main__":
    main()
