"""CPU-side checks of libmlic_hip.so: it loads, exports the whole C ABI, and its host entropy
coder / CDF quantizer match the restated compressai behaviour and the reference fixtures."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import rans_ref
from mlic_amd import _lib, entropy, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "mlic_hip.h")).read()
    names = sorted(set(re.findall(r"\b(mlic_[a-z0-9_]+)\s*\(", hdr)))
    assert len(names) >= 15
    lib = _lib.lib()
    for n in names:
        assert hasattr(lib, n), n
    assert lib.mlic_version().startswith(b"mlic_hip")


def test_null_handle_is_an_error_not_a_crash():
    import ctypes as C
    hs = [C.c_double() for _ in range(3)]
    with pytest.raises(_lib.MlicError, match="null mlic_model handle"):
        _lib.call("mlic_host_stats", None, *[C.byref(v) for v in hs], 1)
    with pytest.raises(_lib.MlicError, match="null mlic_model handle"):
        _lib.call("mlic_set_lanes", None, 2)


def test_conv_choice_is_batch_independent():
    """The kernel family of every conv shape the models run (and a sweep around them) is the same for
    any batch size: families round differently, and a stream coded in a batch must decode alone."""
    shapes = []
    for H, W in ((68, 120), (32, 48), (136, 240), (272, 480), (544, 960), (17, 30), (8, 12), (64, 64)):
        for Cin, Cout, K in ((192, 192, 1), (128, 128, 1), (96, 96, 1), (160, 160, 1), (640, 6400, 1),
                             (480, 640, 1), (496, 224, 1), (224, 128, 1), (128, 32, 1), (32, 96, 1),
                             (192, 768, 3), (192, 192, 3), (320, 320, 5), (256, 64, 5), (3, 192, 1),
                             (192, 12, 3), (320, 640, 3)):
            for stride in ((1, 2) if K != 5 else (1,)):
                shapes.append((Cin, Cout, H, W, K, stride))
    impl = C.c_int()
    for Cin, Cout, H, W, K, stride in shapes:
        got = set()
        for B in (1, 2, 3, 8, 16, 64):
            _lib.call("mlic_conv_choice", B, Cin, Cout, H, W, K, stride, 0, C.byref(impl))
            got.add(impl.value)
        assert len(got) == 1, (Cin, Cout, H, W, K, stride, got)


def test_linatt_split_policy_never_leaves_a_split_empty():
    """The linear attention's key-split policy (the function the model itself calls) over every latent
    size up to 200 000 pixels: 1..64 splits, none of fewer than 256 keys unless there is only one, and
    with ceil(HW / n) keys per split the last split still starts inside the image -- the contract
    ctx_partial_kernel's loop bounds rest on (an empty split's record would carry the max sentinel)."""
    fn = _lib.lib().mlic_linatt_splits
    n = C.c_int()
    ref = C.byref(n)
    for HW in range(1, 200001):
        assert fn(HW, ref) == 0, HW
        v = n.value
        assert 1 <= v <= 64, (HW, v)
        assert v <= max(1, HW // 256), (HW, v)
        assert (v - 1) * -(-HW // v) < HW, (HW, v)
    assert [fn(hw, ref) or n.value for hw in (96, 511, 512, 68 * 120, 136 * 240)] == [1, 1, 2, 31, 64]
    for bad in (0, -5):
        with pytest.raises(_lib.MlicError, match="HW must be"):
            _lib.call("mlic_linatt_splits", bad, ref)
    with pytest.raises(_lib.MlicError, match="null nsplit"):
        _lib.call("mlic_linatt_splits", 100, None)


def test_kernel_entries_refuse_bad_arguments_before_any_gpu_call():
    """The kernel-level entries of the linear attention, LayerNorm, tap gather and the entropy front
    (quantisation, scale indexes, dequantisation, reciprocal plane, bottleneck, checkerboard mask) check
    every argument before they touch the GPU: each refusal below comes back as an error on a machine
    without one (the pointers are never dereferenced)."""
    x = C.c_void_p(64)  # non-null, never read
    la = lambda **kw: _lib.call("mlic_linear_attention_run", None, kw.get("k", x), x, x, kw.get("out", x), None,  # noqa: E731
                                kw.get("B", 1), kw.get("heads", 2), kw.get("hd", 32), kw.get("H", 8), kw.get("W", 8),
                                kw.get("nsplit", 1), kw.get("kmask", 0), kw.get("qmask", 0))
    for kw, msg in (({"hd": 17}, "hd must be"), ({"hd": 64}, "hd must be"), ({"nsplit": 65}, "nsplit must be"),
                    ({"k": None}, "null tensor"), ({"out": None}, "null tensor"), ({"heads": 0}, "heads must be"),
                    ({"B": 0}, "B must be"), ({"H": 0}, "H, W must be"), ({"W": -3}, "H, W must be"),
                    ({"H": 1 << 16, "W": 1 << 16}, "H, W must be"), ({"B": 40000}, "too many"),
                    ({"kmask": 2}, "kmask, qmask"), ({"qmask": -1}, "kmask, qmask")):
        with pytest.raises(_lib.MlicError, match=msg):
            la(**kw)
    pk = lambda **kw: _lib.call("mlic_linatt_pack_run", None, x, kw.get("ctx", x), x, 1, kw.get("heads", 2),  # noqa: E731
                                kw.get("hd", 16), 8, kw.get("W", 8), kw.get("K", 5), kw.get("qmask", 0))
    for kw, msg in (({"K": 1}, "K must be"), ({"K": 4}, "K must be"), ({"K": 7}, "K must be"), ({"hd": 8}, "hd must be"),
                    ({"heads": 3}, "multiple of 32"), ({"ctx": None}, "null tensor"), ({"W": 0}, "H, W must be"),
                    ({"qmask": 2}, "qmask must be")):
        with pytest.raises(_lib.MlicError, match=msg):
            pk(**kw)
    for args, msg in (((x, x, x, x, 1, 48, 10), "C must be"), ((x, x, x, x, 1, 256, 10), "C must be"),
                      ((x, None, x, x, 1, 32, 10), "null tensor"), ((x, x, x, None, 1, 32, 10), "null tensor"),
                      ((x, x, x, x, 1, 32, 0), "H, W must be"), ((x, x, x, x, 0, 32, 10), "B must be")):
        with pytest.raises(_lib.MlicError, match=msg):
            _lib.call("mlic_ln_channels_run", None, *args)
    for args, msg in (((None, x, x, 1, 4, 4), "null tensor"), ((x, None, None, 1, 4, 4), "null tensor"),
                      ((x, x, x, 1, 0, 4), "H, W must be"), ((x, x, x, 70000, 4, 4), "B must be")):
        with pytest.raises(_lib.MlicError, match=msg):
            _lib.call("mlic_taps_gather_run", None, *args)
    # the entropy front's entries.  A complete, valid descriptor (phase 1 with a likelihood, the narrow streams,
    # per-image gains) with one field changed per case
    n = 3 * 4 * 6
    base = dict(y=64, y_bs=n, params=64, params_bs=2 * n, params_a=64, params_a_bs=2 * n, yh=64, yh_bs=n, lik=64,
                lik_bs=n, sym=64, idx=64, sym16=64, idx8=64, ovf=64, nlim=32767, ntable=64, table=64, phase=1, vbr=1,
                sc=64, rs=64, scp=None, rsp=None, B=2, C=3, H=4, W=6)
    planes = dict(sc=None, rs=None, scp=64, rsp=64)
    quant = [({"y": None}, "null tensor"), ({"params": None}, "null tensor"), ({"yh": None}, "null tensor"),
             ({"table": None}, "null tensor"), ({"W": 5}, "W must be even"), ({"phase": 2}, "phase must be"),
             ({"phase": -1}, "phase must be"), ({"params_a": None}, "lik needs params_a"),
             ({"idx8": None}, "sym16 needs idx8 and ovf"), ({"ovf": None}, "sym16 needs idx8 and ovf"),
             ({"sym16": None}, "idx8 and ovf need sym16"),
             ({"sym": None, "sym16": None, "idx8": None, "ovf": None}, "idx needs sym"),
             ({**planes, "rsp": None}, "both or neither"), ({**planes, "scp": None}, "both or neither"),
             ({**planes, "vbr": 0}, "gain planes need vbr"), ({"sc": None}, "vbr needs sc and rs"),
             ({"rs": None}, "vbr needs sc and rs"), ({"vbr": 2}, "vbr must be"), ({"nlim": 0}, "nlim must be"),
             ({"nlim": 32768}, "nlim must be"), ({"ntable": 1}, "ntable must be"), ({"ntable": 257}, "ntable must be"),
             ({"B": 0}, "B must be"), ({"B": 65536}, "B must be"), ({"H": 0}, "H, W must be"),
             ({"W": 0}, "H, W must be"), ({"H": 1 << 16, "W": 1 << 16}, "H, W must be"), ({"C": 0}, "C must be"),
             ({"C": 1 << 27}, "C must be"), ({"y_bs": n - 1}, "y_bs smaller"),
             ({"params_bs": 2 * n - 1}, "params_bs smaller"), ({"params_a_bs": 2 * n - 1}, "params_a_bs smaller"),
             ({"yh_bs": n - 1}, "yh_bs smaller"), ({"lik_bs": n - 1}, "lik_bs smaller")]
    for kw, msg in quant:
        with pytest.raises(_lib.MlicError, match=msg):
            _lib.call("mlic_quant_phase_run", None, C.byref(_lib.QuantDesc(**{**base, **kw})))
    with pytest.raises(_lib.MlicError, match="null descriptor"):
        _lib.call("mlic_quant_phase_run", None, None)
    for kw, msg in (({"idx8": None, "idx": None}, "null output"), ({"params": None}, "null tensor"),
                    ({"table": None}, "null tensor"), ({"W": 3}, "W must be even"), ({"phase": 3}, "phase must be"),
                    ({"sc": None}, "vbr needs sc"), ({**planes, "vbr": 0}, "gain planes need vbr"),
                    ({"ntable": 300}, "ntable must be"), ({"params_bs": n}, "params_bs smaller"),
                    ({"B": -1}, "B must be")):
        with pytest.raises(_lib.MlicError, match=msg):
            _lib.call("mlic_phase_indexes_run", None, C.byref(_lib.QuantDesc(**{**base, **kw})))
    for kw, msg in (({"sym16": None, "sym": None}, "null input"), ({"yh": None}, "null tensor"),
                    ({"params": None}, "null tensor"), ({"W": 7}, "W must be even"), ({"phase": 2}, "phase must be"),
                    ({"rs": None}, "vbr needs rs"), ({**planes, "vbr": 0}, "gain planes need vbr"),
                    ({"yh_bs": 1}, "yh_bs smaller"), ({"params_bs": 0}, "params_bs smaller"), ({"H": -2}, "H, W must be")):
        with pytest.raises(_lib.MlicError, match=msg):
            _lib.call("mlic_phase_dequant_run", None, C.byref(_lib.QuantDesc(**{**base, **kw})))
    for args, msg in (((None, x, 4), "null tensor"), ((x, None, 4), "null tensor"), ((x, x, 0), "n must be"),
                      ((x, x, (1 << 31) + 1), "n must be")):
        with pytest.raises(_lib.MlicError, match=msg):
            _lib.call("mlic_recip_plane_run", None, *args)
    eb = lambda **kw: _lib.call("mlic_eb_forward_run", None, kw.get("z", x), kw.get("z_hat", x), kw.get("lik", x),  # noqa: E731
                                kw.get("sym", x), kw.get("q", x), *[None if kw.get("hole") == j else x for j in range(14)],
                                kw.get("B", 2), kw.get("C", 5), kw.get("H", 3), kw.get("W", 7))
    for kw, msg in [({"z": None}, "null tensor"), ({"q": None}, "null tensor"),
                    ({"z_hat": None, "lik": None, "sym": None}, "at least one"), ({"B": 0}, "B must be"),
                    ({"C": 0}, "C must be"), ({"W": 0}, "H, W must be"),
                    ({"B": 4096, "C": 4096, "H": 64, "W": 64}, "C must be")] + [({"hole": j}, "null parameter")
                                                                                 for j in range(14)]:
        with pytest.raises(_lib.MlicError, match=msg):
            eb(**kw)
    for args, msg in (((None, x, x, 1, 2, 3, 4), "null tensor"), ((x, None, x, 1, 2, 3, 4), "null tensor"),
                      ((x, x, None, 1, 2, 3, 4), "null tensor"), ((x, x, x, 0, 2, 3, 4), "B must be"),
                      ((x, x, x, 1, 0, 3, 4), "C must be"), ((x, x, x, 1, 2, 0, 4), "H, W must be")):
        with pytest.raises(_lib.MlicError, match=msg):
            _lib.call("mlic_eb_dequant_run", None, *args)
    for args, msg in (((None, 24, x, 24, 1, 2, 3, 4, 0), "null tensor"), ((x, 24, None, 24, 1, 2, 3, 4, 0), "null tensor"),
                      ((x, 23, x, 24, 1, 2, 3, 4, 0), "x_bs smaller"), ((x, 24, x, 23, 1, 2, 3, 4, 1), "y_bs smaller"),
                      ((x, 24, x, 24, 1, 2, 3, 4, 2), "keep_anchor must be"), ((x, 24, x, 24, 0, 2, 3, 4, 0), "B must be"),
                      ((x, 24, x, 24, 1, 0, 3, 4, 0), "C must be"), ((x, 24, x, 24, 1, 2, 3, 0, 0), "H, W must be")):
        with pytest.raises(_lib.MlicError, match=msg):
            _lib.call("mlic_ckbd_mask_run", None, *args)


def test_gaussian_tables_match_reference_update(golden):
    g = golden("scale_table.npz")
    cdf, length, offset, table = entropy.gaussian_tables(entropy.get_scale_table())
    assert torch.equal(table, torch.from_numpy(g["table"]))
    assert np.array_equal(cdf.numpy(), g["quantized_cdf"])
    assert np.array_equal(length.numpy(), g["cdf_length"])
    assert np.array_equal(offset.numpy(), g["offset"])


def _eb_params(sd):
    return {k.split(".", 1)[1]: v for k, v in sd.items() if k.startswith("entropy_bottleneck.")
            and (".quantiles" in k or "._" in k) and not k.endswith(("_offset", "_quantized_cdf", "_cdf_length"))}


def test_bottleneck_tables_match_reference_update(golden):
    g = golden("eb_cdf_L.npz")
    sd = synthetic.synth_state_dict("MLICPP_L", 0)
    cdf, length, offset = entropy.bottleneck_tables(_eb_params(sd))
    assert np.array_equal(cdf.numpy(), g["quantized_cdf"])
    assert np.array_equal(length.numpy(), g["cdf_length"])
    assert np.array_equal(offset.numpy(), g["offset"])


def test_bottleneck_tables_every_weight_set_and_form_diff(golden):
    """EntropyBottleneck.update() (mlicpp.py:470-475 -> compressai 1.2.6) on every fixture weight set:
    the product's z CDF tables equal the reference's, entry for entry.  Also counts how many quantised
    CDF entries the compressai-1.1 sign-trick pmf would change -- the entries where a coder built on the
    wrong form would write z streams a reference decoder cannot read (recorded in $MLIC_PARITY_OUT)."""
    import hashlib
    import json
    g = golden("eb_cdf_sets.npz")
    tags = sorted({k.split(".")[0] for k in g.files})
    assert len(tags) >= 10
    rec = {}
    for tag in tags:
        name, rate = (tag.rsplit("_r", 1)[0], int(tag.rsplit("_r", 1)[1])) if "_r" in tag[-3:] else (tag, None)
        sd = synthetic.synth_state_dict(name, 0, rate=rate)
        h = hashlib.sha256()
        for k in sorted(sd):
            h.update(k.encode())
            h.update(sd[k].contiguous().numpy().tobytes())
        assert h.hexdigest() == str(g[f"{tag}.sd_sha"]), tag
        p = _eb_params(sd)
        cdf, length, offset = entropy.bottleneck_tables(p)
        assert np.array_equal(cdf.numpy(), g[f"{tag}.quantized_cdf"]), tag
        assert np.array_equal(length.numpy(), g[f"{tag}.cdf_length"]), tag
        assert np.array_equal(offset.numpy(), g[f"{tag}.offset"]), tag
        old, _, _ = entropy.bottleneck_tables(p, sign_trick=True)
        diff = old.numpy() != cdf.numpy()
        rec[tag] = {"entries": int(cdf.numel()), "sign_trick_entries_differing": int(diff.sum()),
                    "channels_differing": int(diff.any(axis=1).sum()), "channels": int(cdf.shape[0])}
    out = os.environ.get("MLIC_PARITY_OUT")
    if out:
        old_rec = json.load(open(out)) if os.path.exists(out) else {}
        old_rec["eb_cdf_form_diff"] = rec
        with open(out, "w") as f:
            json.dump(old_rec, f, indent=1, sort_keys=True)
    print(json.dumps(rec))


def _gc_tables(golden):
    g = golden("scale_table.npz")
    return g["quantized_cdf"], g["cdf_length"], g["offset"]


def test_rans_roundtrip_reference_streams(golden):
    cdf, length, offset = _gc_tables(golden)
    f = golden("forward_MLICPP_L_128x192.npz")
    sym, idx = f["y_symbols"], f["y_indexes"]
    data = entropy.rans_encode(sym, idx, cdf, length, offset)
    assert len(data) % 4 == 0
    back = entropy.rans_decode(data, idx, cdf, length, offset)
    assert np.array_equal(back, sym)
    # bytes identical to the pure-Python restatement of compressai's coder
    n = 20000
    ref = rans_ref.encode(sym[:n].tolist(), idx[:n].tolist(), cdf.tolist(), length.tolist(), offset.tolist())
    assert entropy.rans_encode(sym[:n], idx[:n], cdf, length, offset) == ref


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_rans_bypass_and_extremes(golden, seed):
    cdf, length, offset = _gc_tables(golden)
    r = np.random.default_rng(seed)
    n = 5000
    idx = r.integers(0, 64, n).astype(np.int32)
    sym = (r.standard_normal(n) * r.choice([0.5, 3, 40, 3000], n)).astype(np.int32)
    sym[:8] = [0, -1, 1, 2 ** 20, -(2 ** 20), 2 ** 30, -(2 ** 30), 123456]
    data = entropy.rans_encode(sym, idx, cdf, length, offset)
    assert np.array_equal(entropy.rans_decode(data, idx, cdf, length, offset), sym)
    ref = rans_ref.encode(sym.tolist(), idx.tolist(), cdf.tolist(), length.tolist(), offset.tolist())
    assert data == ref


def _decode_narrow(data, idx8, nparts, cdf, length, offset):
    cdf_, length_, offset_ = (np.ascontiguousarray(np.asarray(v), dtype=np.int32) for v in (cdf, length, offset))
    out = np.zeros(idx8.size, np.int32)
    widened = C.c_int(-1)
    _lib.call("mlic_rans_decode_narrow", data, len(data), idx8.ctypes.data, idx8.size, nparts, cdf_.ctypes.data,
              length_.ctypes.data, offset_.ctypes.data, cdf_.shape[0], cdf_.shape[1], out.ctypes.data,
              C.byref(widened))
    return out, widened.value


@pytest.mark.parametrize("limit", [0, 40, 3])
def test_rans_narrow_decode_fallback(golden, limit):
    """The decompress path's narrow decode: each phase is decoded into int16 and, when a value
    leaves the narrow range, the decoder resets to the phase's start and decodes it again into int32
    (PhaseDecoder::run -> rans_decode_piece).  The narrow range is lowered with the "narrow_limit" knob so
    that the fallback runs here: the symbols must come back exactly, the pieces that widen are exactly the
    ones holding an out-of-range value, and the stream is consumed in step (later pieces decode right)."""
    cdf, length, offset = _gc_tables(golden)
    r = np.random.default_rng(11)
    nparts, npiece = 20, 750
    idx8 = r.integers(0, 64, nparts * npiece).astype(np.uint8)
    sym = (r.standard_normal(nparts * npiece) * 4).astype(np.int32)
    sym[3 * npiece + 7] = 70000            # beyond int16: piece 3 must widen at every limit
    sym[8 * npiece + 100] = -40000         # piece 8 too
    sym[12 * npiece + 5] = 41              # beyond the limit of 40 only
    data = entropy.rans_encode(sym, idx8.astype(np.int32), cdf, length, offset)
    try:
        _lib.call("mlic_set_kernel_option", b"narrow_limit", limit)
        back, widened = _decode_narrow(data, idx8, nparts, cdf, length, offset)
    finally:
        _lib.call("mlic_set_kernel_option", b"narrow_limit", 0)
    assert np.array_equal(back, sym)
    lim = 32767 if limit <= 0 else limit
    want = sum(1 for k in range(nparts) if np.any((sym[k * npiece:(k + 1) * npiece] > lim) |
                                                  (sym[k * npiece:(k + 1) * npiece] < -lim - 1)))
    assert widened == want and widened >= 2
    # the plain int32 decoder agrees on the same stream
    assert np.array_equal(entropy.rans_decode(data, idx8.astype(np.int32), cdf, length, offset), sym)


# The kernel options (csrc/options.cpp): name -> (environment variable, default).  _effective restates each
# option's rule: `o` is the value last given to mlic_set_kernel_option (-1: never set), the result is what
# mlic_get_kernel_option must report.
OPTIONS = {"x4_halo": ("MLIC_X4_HALO", 1), "x4_splitk": ("MLIC_X4_SPLITK", 0), "linatt_fused": ("MLIC_LINATT_FUSED", 1),
           "dw_strip": ("MLIC_DW_STRIP", 1), "ep_half": ("MLIC_EP_HALF", 1), "chain_nj": ("MLIC_CHAIN_NJ", 1),
           "dwpw2": ("MLIC_DWPW2", 2), "pw3": ("MLIC_PW3", 1), "narrow_limit": (None, 32767),
           "image_io_path": (None, -1)}


def _effective(name, o, environ):
    var, default = OPTIONS[name]
    env = default
    if var is not None and var in environ:  # atoi
        m = re.match(r"\s*[+-]?\d+", environ[var])
        env = int(m.group()) if m else 0
    if name == "x4_halo":
        return (0 if o == 0 else 2) if o >= 0 else env
    if name in ("x4_splitk", "linatt_fused", "dw_strip", "ep_half"):
        return int(o != 0) if o >= 0 else int(env != 0)
    if name == "chain_nj":
        return 2 if (o if o > 0 else env) == 2 else 1
    if name == "narrow_limit":
        return 32767 if o <= 0 or o > 32767 else o
    return o if o >= 0 else env  # dwpw2, pw3, image_io_path


def _get_option(name):
    v = C.c_int(-99)
    _lib.call("mlic_get_kernel_option", name.encode(), C.byref(v))
    return v.value


@pytest.mark.parametrize("name", sorted(OPTIONS))
def test_kernel_option_default_set_and_revert(name):
    revert = 0 if name == "narrow_limit" else -1
    default = _effective(name, -1, os.environ)
    if OPTIONS[name][0] is None or OPTIONS[name][0] not in os.environ:
        assert default == OPTIONS[name][1]
    assert _get_option(name) == default
    try:
        for v in (-1, 0, 1, 2, 3) + ((40, 40000) if name == "narrow_limit" else ()):
            if name == "image_io_path" and v == 3:  # out of range: refused, the 2 stays
                with pytest.raises(_lib.MlicError):
                    _lib.call("mlic_set_kernel_option", name.encode(), v)
                assert _get_option(name) == 2
                continue
            _lib.call("mlic_set_kernel_option", name.encode(), v)
            assert _get_option(name) == _effective(name, v, os.environ), v
    finally:
        _lib.call("mlic_set_kernel_option", name.encode(), revert)
    assert _get_option(name) == default


def test_kernel_option_errors_change_nothing():
    try:
        _lib.call("mlic_set_kernel_option", b"image_io_path", 1)
        for bad in (3, -2):
            with pytest.raises(_lib.MlicError, match=r"mlic: image_io_path must be -1 \(by layout\), 0, 1 or 2"):
                _lib.call("mlic_set_kernel_option", b"image_io_path", bad)
            assert _get_option("image_io_path") == 1
    finally:
        _lib.call("mlic_set_kernel_option", b"image_io_path", -1)
    before = {n: _get_option(n) for n in OPTIONS}
    with pytest.raises(_lib.MlicError, match="mlic: unknown kernel option x4_hallo"):
        _lib.call("mlic_set_kernel_option", b"x4_hallo", 1)
    with pytest.raises(_lib.MlicError, match="mlic: unknown kernel option x4_hallo"):
        _get_option("x4_hallo")
    assert {n: _get_option(n) for n in OPTIONS} == before


# a fresh process per case (this one has read its environment already), on ctypes alone: the getter's values
# as the process starts, then after each (name, value) set
_OPTION_CHILD = """
import ctypes as C, json, sys
lib = C.CDLL(sys.argv[1])
def get(n):
    v = C.c_int(-99)
    assert lib.mlic_get_kernel_option(n.encode(), C.byref(v)) == 0
    return v.value
out = {"start": {n: get(n) for n in json.loads(sys.argv[2])}, "steps": []}
for n, v in json.loads(sys.argv[3]):
    assert lib.mlic_set_kernel_option(n.encode(), C.c_int(v)) == 0
    out["steps"].append(get(n))
print(json.dumps(out))
"""


@pytest.mark.parametrize("var,value,name,sets", [
    ("MLIC_CHAIN_NJ", "2", "chain_nj", (1, -1, 1, 0, 3, -1)),
    ("MLIC_X4_HALO", "0", "x4_halo", (1, -1, 0, -1)),
    ("MLIC_X4_HALO", "2", "x4_halo", (0, -1, 1, -1)),
    ("MLIC_EP_HALF", "0", "ep_half", (1, -1, 0, -1)),
    ("MLIC_DWPW2", "0", "dwpw2", (2, -1, 1, -1)),
    ("MLIC_X4_SPLITK", "1", "x4_splitk", (0, -1, 1, -1)),
    ("MLIC_LINATT_FUSED", "0", "linatt_fused", (1, -1)),
    ("MLIC_DW_STRIP", "0", "dw_strip", (1, -1)),
    ("MLIC_PW3", "2", "pw3", (0, -1)),
])
def test_kernel_option_environment_fallback(var, value, name, sets):
    """An option starts at its environment variable, a set overrides the variable, and -1 (for chain_nj 0 as
    well) returns to the variable, not to the built-in default; the other options keep their defaults."""
    import json
    import subprocess
    import sys
    environ = {k: v for k, v in os.environ.items() if k not in {e for e, _ in OPTIONS.values()}}
    environ[var] = value
    r = subprocess.run([sys.executable, "-c", _OPTION_CHILD, _lib.LIB_PATH, json.dumps(sorted(OPTIONS)),
                        json.dumps([(name, v) for v in sets])], env=environ, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    assert out["start"] == {n: _effective(n, -1, environ) for n in OPTIONS}
    assert out["start"][name] != OPTIONS[name][1]  # the case's variable moves its option off the default
    assert out["steps"] == [_effective(name, v, environ) for v in sets]
    assert out["steps"][-1] == out["start"][name]


def test_rans_empty_stream(golden):
    cdf, length, offset = _gc_tables(golden)
    data = entropy.rans_encode(np.zeros(0, np.int32), np.zeros(0, np.int32), cdf, length, offset)
    assert len(data) == 8
    assert entropy.rans_decode(data, np.zeros(0, np.int32), cdf, length, offset).size == 0


def test_pmf_to_quantized_cdf_properties():
    r = np.random.default_rng(3)
    for n in (2, 5, 37, 300):
        p = r.dirichlet(np.ones(n) * 0.3).astype(np.float32)
        p[r.integers(0, n)] = 0.0  # zero-probability symbols must still get frequency >= 1
        c = entropy.pmf_to_quantized_cdf(p)
        assert c[0] == 0 and c[-1] == 1 << 16
        assert np.all(np.diff(c) >= 1)


def test_conv_choice_pins_the_measured_selection():
    """The kernel family per layer shape that the A/B measurements chose; a
    regression here changes speed (and, as families round differently, the exact bits)."""
    F32, X3, X3V2, PW, NARROW, SMALLCIN, HALO, X4 = range(8)
    impl = C.c_int()

    def choice(Cin, Cout, H, W, K, stride=1, B=8, epi=0):
        _lib.call("mlic_conv_choice", B, Cin, Cout, H, W, K, stride, epi, C.byref(impl))
        return impl.value

    assert choice(192, 768, 272, 480, 3) == X4            # g_s subpel convs
    assert choice(320, 1280, 8, 12, 3) == X4              # h_s subpel at the Kodak z grid (split-K)
    assert choice(192, 192, 544, 960, 1) == PW            # full-resolution point convs
    assert choice(224, 128, 32, 48, 1, epi=1) == PW       # Kodak-size LRP.2 (GELU): resident from 1 K px
    assert choice(224, 128, 17, 30, 1, epi=1) != PW       # below 1 K px/image
    assert choice(288, 288, 68, 120, 1) == X4             # context q/k/v (Cin <= 352)
    assert choice(640, 224, 68, 120, 1, epi=1) == X4      # 1080p LRP point conv: 1.07x x3v2
    assert choice(640, 224, 32, 48, 1, epi=1) == X4       # Kodak LRP: 1.3x
    assert choice(160, 96, 68, 120, 1) == X3V2            # narrow latent 1x1s without a resident form
    assert choice(640, 6400, 68, 120, 1) == X4            # hoisted EntropyParameters GEMM
    assert choice(288, 96, 68, 120, 5) == X4              # 5x5 reprojections
    assert choice(192, 192, 544, 960, 3, stride=2) == X4  # small-decoder dense strided conv
    assert choice(96, 128, 68, 120, 3) == X4              # small-decoder channel context: 1.4x x3v2
    assert choice(288, 96, 68, 120, 3, epi=1) == X4       # 1.5x
    assert choice(3, 192, 1088, 1920, 3, stride=2) == SMALLCIN
    assert choice(3, 192, 1088, 1920, 1, stride=2) == SMALLCIN
    assert choice(192, 12, 544, 960, 3) == NARROW
    assert choice(48, 48, 1088, 1920, 1) == PW            # small-decoder g_s width


@pytest.mark.parametrize("vbr", [False, True])
def test_file_bytes_is_the_written_file_size(vbr):
    """bench.py's bpp_file counts the whole file the harness writes (utils/utils.py:71-83)."""
    import io
    from mlic_amd import bitstream
    y, z = b"\x01" * 37, b"\x02" * 5
    buf = io.BytesIO()
    n = bitstream.write_stream(buf, 120, 200, (2, 4), [[y], [z]], level=3 if vbr else None)
    assert n == len(buf.getvalue()) == bitstream.file_bytes(len(y), len(z), vbr=vbr)
    buf.seek(0)
    hdr, strings, shape = bitstream.read_stream(buf, vbr=vbr)
    assert strings == [[y], [z]] and shape == (2, 4) and hdr[:2] == (120, 200)


def test_build_record_matches_tree():
    """The in-tree library carries a record of the sources it was built from (mlic_amd/build.py); it
    matches the tree, and the recorded library digest is the library's."""
    import hashlib
    import json
    from mlic_amd import build
    rec = json.load(open(build.RECORD))
    assert rec["sources_sha256"] == build.source_digest()
    assert rec["library_sha256"] == hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()
    assert rec["target"] == "gfx950"
