"""Spec mirror of the JPEG decoder (include/ccvs_hip_decode.h states the arithmetic): numpy and plain Python,
never imported by `ccvs_amd`.  `decode(data)` gives the RGB pixels of one baseline file -- libjpeg's, bit for bit -- and counts what
the entropy decoder met on the way; tests/golden/make_golden_mjpeg_decode.py and tests/test_mjpeg_decode_host.py hold it against
Pillow (libjpeg-turbo), tests/test_mjpeg_decode_gpu.py holds the kernels against it.  It has its own marker walk and its own split of
the scan into units (a unit: one restart interval, or the whole scan of a file without DRI), written the slow obvious way, so that
`ccvs_amd.tools.mjpeg.parse_jpeg` / `find_units` can be held against them.  Sampling is numbered as Pillow numbers it: 0 = 4:4:4,
1 = 4:2:2 (luminance 2 x 1), 2 = 4:2:0 (luminance 2 x 2)."""
import numpy as np

import jpeg_ref as R

# status of a unit (the kernel's words, include/ccvs_hip_decode.h); the tests compare zero against non-zero
OK, BAD_UNIT, BAD_CODE, OVERRUN, BAD_INDEX, LEFTOVER = 0, 1, 2, 3, 4, 5
SAMPLING = {(1, 1): 0, (2, 1): 1, (2, 2): 2}        # luminance (h, v) factors against 1 x 1 chrominance
FACTORS = {v: k for k, v in SAMPLING.items()}


def new_stats():
    return {"stuffed": 0, "zrl": 0, "no_eob": 0, "max_dc_cat": 0, "long_code": 0, "rst_wrap": 0, "partial_last": 0, "units": 0,
            "partial_mcu_420": 0, "idct_out_of_range": 0}


# ------------------------------------------------------------------ the file
def parse(data):
    """dict of a baseline three-component file: h, w, sampling, q [3][64] natural order per component, huff {class/id byte: (bits,
    vals)} (the Annex K tables where the file has no DHT), dc / ac table ids per component, ri (0: no DRI), scan (bytes)."""
    segs, start = R.segments(data)
    assert data[-2:] == b"\xff\xd9", "no EOI"
    out = {"ri": 0, "scan": bytes(data[start:-2]), "scan_offset": start}
    qt, comps = {}, None
    for marker, p in segs:
        if marker == 0xDB:
            i = 0
            while i < len(p):
                assert p[i] >> 4 == 0, "16-bit quantiser table"
                nat = [0] * 64
                for k in range(64):
                    nat[R.ZIGZAG[k]] = p[i + 1 + k]
                qt[p[i] & 15] = nat
                i += 65
        elif marker == 0xC0:
            assert p[0] == 8 and p[5] == 3
            out["h"], out["w"] = (p[1] << 8) | p[2], (p[3] << 8) | p[4]
            comps = [(p[6 + 3 * c], p[7 + 3 * c] >> 4, p[7 + 3 * c] & 15, p[8 + 3 * c]) for c in range(3)]
        elif marker == 0xDD:
            out["ri"] = (p[0] << 8) | p[1]
        elif marker == 0xDA:
            assert p[0] == 3 and [p[1 + 2 * c] for c in range(3)] == [c[0] for c in comps]
            out["dc"] = [p[2 + 2 * c] >> 4 for c in range(3)]
            out["ac"] = [p[2 + 2 * c] & 15 for c in range(3)]
        else:
            assert marker == 0xC4 or 0xE0 <= marker <= 0xEF or marker == 0xFE, f"marker {marker:#x}"
    assert comps[1][1:3] == (1, 1) and comps[2][1:3] == (1, 1)
    out["sampling"] = SAMPLING[comps[0][1:3]]
    out["q"] = [qt[c[3]] for c in comps]
    out["huff"] = R.dht_tables(segs) or {k: (list(b), list(v)) for k, (b, v) in R.HUFF.items()}
    return out


def geometry(h, w, sampling):
    """(hs, vs, MCUs per row, MCU rows)."""
    hs, vs = FACTORS[sampling]
    return hs, vs, -(-w // (8 * hs)), -(-h // (8 * vs))


def split_units(scan, ri, n_mcu, stats=None):
    """[(offset, length, first MCU, MCUs)] of the units of a scan: a walk over the bytes."""
    if ri == 0:
        return [(0, len(scan), 0, n_mcu)]
    units, start, i, k = [], 0, 0, 0
    while i + 1 < len(scan):
        if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7:
            assert scan[i + 1] == 0xD0 + (k & 7), "restart markers out of order"
            if stats is not None and k >= 8 and (k & 7) == 0:
                stats["rst_wrap"] += 1
            units.append((start, i - start, k * ri, ri))
            k, start, i = k + 1, i + 2, i + 2
        else:
            i += 1
    units.append((start, len(scan) - start, k * ri, n_mcu - k * ri))
    assert len(units) == -(-n_mcu // ri) and 1 <= units[-1][3] <= ri
    if stats is not None and units[-1][3] < ri:
        stats["partial_last"] += 1
    return units


# ------------------------------------------------------------------ entropy decoding
_LUT = {}


def _lut(bits, vals):
    """16 bits of lookahead -> (length << 8) | symbol, 0 where no code starts so (T.81 Annex C gives the codes)."""
    key = (tuple(bits), tuple(vals))
    if key not in _LUT:
        lut = np.zeros(65536, dtype=np.int32)
        code, k = 0, 0
        for length in range(1, 17):
            for _ in range(bits[length - 1]):
                lut[code << (16 - length):(code + 1) << (16 - length)] = (length << 8) | vals[k]
                code, k = code + 1, k + 1
            code <<= 1
        _LUT[key] = lut.tolist()
    return _LUT[key]


class _Bits:
    """The bits of one unit, stuffing undone; what lies behind a 0xFF that no 0x00 follows is never read."""

    def __init__(self, data, stats):
        raw, self.cut = bytearray(), False
        i = 0
        while i < len(data):
            if data[i] == 0xFF:
                if i + 1 < len(data) and data[i + 1] == 0:
                    if stats is not None:
                        stats["stuffed"] += 1
                    raw.append(0xFF)
                    i += 2
                    continue
                self.cut = True
                break
            raw.append(data[i])
            i += 1
        self.total = 8 * len(raw)
        self.big = int.from_bytes(bytes(raw) + b"\0\0\0", "big")
        self.shift = self.total + 24
        self.pos = 0

    def peek16(self):
        return (self.big >> (self.shift - self.pos - 16)) & 0xFFFF

    def take(self, n):                      # None: the unit has fewer bits left
        if self.pos + n > self.total:
            return None
        v = (self.big >> (self.shift - self.pos - n)) & ((1 << n) - 1)
        self.pos += n
        return v


def _symbol(bits, lut, stats):
    e = lut[bits.peek16()]
    if e == 0:
        return None, BAD_CODE
    if bits.take(e >> 8) is None:
        return None, OVERRUN
    if stats is not None and (e >> 8) > 8:
        stats["long_code"] += 1
    return e & 255, OK


def _extend(v, s):
    return v - (1 << s) + 1 if v < (1 << (s - 1)) else v


def decode_unit(data, p, first, count, coef, stats=None):
    """Decodes MCUs first .. first + count - 1 from the unit's bytes into coef {component: int array [block rows, block columns, 64]};
    returns the status.  A unit that fails leaves the coefficients it had written."""
    hs, vs, mcux, _ = geometry(p["h"], p["w"], p["sampling"])
    luts = {k: _lut(*bv) for k, bv in p["huff"].items()}
    bits, pred = _Bits(data, stats), [0, 0, 0]
    for m in range(first, first + count):
        my, mx = divmod(m, mcux)
        for c, (nh, nv) in enumerate(((hs, vs), (1, 1), (1, 1))):
            if p["dc"][c] not in (0, 1) or p["dc"][c] not in luts or (0x10 | p["ac"][c]) not in luts or p["ac"][c] not in (0, 1):
                return BAD_CODE
            dc, ac = luts[p["dc"][c]], luts[0x10 | p["ac"][c]]
            for v in range(nv):
                for hh in range(nh):
                    blk = coef[c][my * nv + v, mx * nh + hh]
                    s, st = _symbol(bits, dc, stats)
                    if st:
                        return st
                    if s > 11:
                        return BAD_CODE
                    if stats is not None:
                        stats["max_dc_cat"] = max(stats["max_dc_cat"], s)
                    diff = 0
                    if s:
                        diff = bits.take(s)
                        if diff is None:
                            return OVERRUN
                        diff = _extend(diff, s)
                    pred[c] += diff
                    blk[0] = pred[c]
                    k = 1
                    while k < 64:
                        rs, st = _symbol(bits, ac, stats)
                        if st:
                            return st
                        r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r != 15:
                                break
                            if stats is not None:
                                stats["zrl"] += 1
                            k += 16
                            continue
                        if s > 10:
                            return BAD_CODE
                        k += r
                        if k > 63:
                            return BAD_INDEX
                        val = bits.take(s)
                        if val is None:
                            return OVERRUN
                        blk[R.ZIGZAG[k]] = _extend(val, s)
                        k += 1
                    else:
                        if stats is not None and k == 64:
                            stats["no_eob"] += 1
    if bits.cut or bits.total - bits.pos >= 8:
        return LEFTOVER
    return OK


def empty_coefficients(p):
    hs, vs, mcux, mcuy = geometry(p["h"], p["w"], p["sampling"])
    return [np.zeros((mcuy * nv, mcux * nh, 64), dtype=np.int64) for nh, nv in ((hs, vs), (1, 1), (1, 1))]


def decode_coefficients(p, stats=None, units=None, scan=None):
    """(coefficients per component, [status per unit]).  units / scan: another unit table or other bytes than the file's own."""
    hs, vs, mcux, mcuy = geometry(p["h"], p["w"], p["sampling"])
    scan = p["scan"] if scan is None else scan
    units = split_units(scan, p["ri"], mcux * mcuy, stats) if units is None else units
    coef = empty_coefficients(p)
    status = [decode_unit(scan[off:off + length], p, first, count, coef, stats) for off, length, first, count in units]
    if stats is not None:
        stats["units"] += len(units)
        if p["sampling"] == 2 and p["w"] % 16 and p["h"] % 16:
            stats["partial_mcu_420"] += 1
    return coef, status


# ------------------------------------------------------------------ the pixels
_C = {name: int(c * 8192 + 0.5) for name, c in (("0.298", 0.298631336), ("0.390", 0.390180644), ("0.541", 0.541196100), ("0.765", 0.765366865),
                                               ("0.899", 0.899976223), ("1.175", 1.175875602), ("1.501", 1.501321110), ("1.847", 1.847759065),
                                               ("1.961", 1.961570560), ("2.053", 2.053119869), ("2.562", 2.562915447), ("3.072", 3.072711026))}


def _idct_1d(d, n):
    """jidctint's pass ("islow", CONST_BITS 13) over the last axis of d [..., 8] (int64), descaled by n bits."""
    z2, z3 = d[..., 2], d[..., 6]
    z1 = (z2 + z3) * _C["0.541"]
    t2, t3 = z1 - z3 * _C["1.847"], z1 + z2 * _C["0.765"]
    t0, t1 = (d[..., 0] + d[..., 4]) << 13, (d[..., 0] - d[..., 4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = d[..., 7], d[..., 5], d[..., 3], d[..., 1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * _C["1.175"]
    t0, t1, t2, t3 = t0 * _C["0.298"], t1 * _C["2.053"], t2 * _C["3.072"], t3 * _C["1.501"]
    z1, z2 = -z1 * _C["0.899"], -z2 * _C["2.562"]
    z3, z4 = -z3 * _C["1.961"] + z5, -z4 * _C["0.390"] + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    half = 1 << (n - 1)
    return np.stack([(t10 + t3 + half) >> n, (t11 + t2 + half) >> n, (t12 + t1 + half) >> n, (t13 + t0 + half) >> n,
                     (t13 - t0 + half) >> n, (t12 - t1 + half) >> n, (t11 - t2 + half) >> n, (t10 - t3 + half) >> n], axis=-1)


def idct_plane(coef, q, stats=None):
    """coef [block rows, block columns, 64] quantised, q [64] -> the uint8 plane padded to whole blocks."""
    by, bx = coef.shape[:2]
    d = (coef * np.asarray(q, dtype=np.int64)).reshape(by, bx, 8, 8)
    d = _idct_1d(d.swapaxes(-1, -2), 11).swapaxes(-1, -2)           # columns
    d = _idct_1d(d, 18)                                             # rows
    if stats is not None:
        stats["idct_out_of_range"] += int(((d < -512) | (d > 511)).sum())
    return np.clip(d + 128, 0, 255).transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)


def upsample_h2v1(c, w):
    """c [rows, ceil(w / 2)] -> [rows, w]: libjpeg's "fancy" (triangle) filter, the ends replicated."""
    left, right = np.concatenate([c[:, :1], c[:, :-1]], axis=1), np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
    out = np.empty((c.shape[0], 2 * c.shape[1]), dtype=np.int64)
    out[:, 0::2] = (3 * c + left + 1) >> 2
    out[:, 1::2] = (3 * c + right + 2) >> 2
    return out[:, :w]


def upsample_h2v2(c, h, w):
    """c [ceil(h / 2), ceil(w / 2)] -> [h, w]."""
    up, down = np.concatenate([c[:1], c[:-1]]), np.concatenate([c[1:], c[-1:]])
    s = np.empty((2 * c.shape[0], c.shape[1]), dtype=np.int64)
    s[0::2], s[1::2] = 3 * c + up, 3 * c + down
    left, right = np.concatenate([s[:, :1], s[:, :-1]], axis=1), np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    out = np.empty((s.shape[0], 2 * s.shape[1]), dtype=np.int64)
    out[:, 0::2] = (3 * s + left + 8) >> 4
    out[:, 1::2] = (3 * s + right + 7) >> 4
    return out[:h, :w]


def pixels(p, coef, stats=None):
    h, w, sampling = p["h"], p["w"], p["sampling"]
    y, cb, cr = (idct_plane(coef[c], p["q"][c], stats) for c in range(3))
    y = y[:h, :w]
    if sampling == 1:
        cb, cr = (upsample_h2v1(c[:h, :-(-w // 2)], w) for c in (cb, cr))
    elif sampling == 2:
        cb, cr = (upsample_h2v2(c[:-(-h // 2), :-(-w // 2)], h, w) for c in (cb, cr))
    else:
        cb, cr = cb[:h, :w], cr[:h, :w]
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def decode(data, stats=None):
    """uint8 [h, w, 3] of a whole file; every unit must decode cleanly."""
    p = parse(data)
    coef, status = decode_coefficients(p, stats)
    assert not any(status), status
    return pixels(p, coef, stats)


# ------------------------------------------------------------------ the case table of tests/golden/mjpeg_decode_cases.npz
def images():
    """name -> uint8 image: those of jpeg_ref.CASES and three more."""
    out = {name: make() for name, (make, _, _) in R.CASES.items()}
    out["noise_17x35"] = R._noise(17, 35, 21)
    out["noise_1x1"] = R._noise(1, 1, 22)
    out["smooth_31x50"] = R.CASES["smooth_64x64"][0]()[:31, :50].copy()
    return out


ALL_Q = (100, 90, 30, 5)
# the larger images keep one or two qualities, so that the fixture stays small (noise does not compress)
THIN = {"smooth_64x64": (90,), "noise_8x520": (30,), "noise_24x40": (100,), "smooth_31x50": (90, 5), "noise_88x8": (30,), "noise_72x8": (100, 30),
        "noise_16x40_r3": (100, 30), "noise_17x35": (100, 30)}
# (image, quality, subsampling): Pillow's optimize=True, files with Huffman tables of their own
OPTIMISED = (("noise_13x21", 90, 2), ("noise_13x21", 5, 2), ("smooth_31x50", 30, 1))      # two of one size: one call, two sets of tables


def rows():
    """[(key, image name, quality, subsampling, restart_marker_blocks, optimize)]; 'project/...' is built from `jpeg_header`."""
    out = []
    for name, img in images().items():
        if name == "smooth_256x256":
            continue
        for q in THIN.get(name, ALL_Q):
            for sub in (0, 1, 2):
                if sub and img.shape[1] <= 4:
                    continue
                for rst in (0, 3):
                    out.append((f"{name}/q{q}/s{sub}/r{rst}", name, q, sub, rst, False))
    out += [(f"{name}/q{q}/s{sub}/opt", name, q, sub, 0, True) for name, q, sub in OPTIMISED]
    out.append(("smooth_256x256/q90/s0/r32", "smooth_256x256", 90, 0, 32, False))
    out.append(("project/noise_24x40/q90/nodht", "noise_24x40", 90, 0, 5, False))
    return out


def load_fixture(path):
    """{row key: (file bytes, Pillow's uint8 [H, W, 3])} of tests/golden/mjpeg_decode_cases.npz, and its Pillow version string."""
    z = np.load(path)
    imgs, off, files, rgb = images(), z["file_offsets"], z["files"].tobytes(), z["rgb"]
    out, at = {}, 0
    for i, (key, name, *_) in enumerate(rows()):
        h, w = imgs[name].shape[:2]
        out[key] = (files[off[i]:off[i + 1]], rgb[at:at + h * w * 3].reshape(h, w, 3))
        at += h * w * 3
    assert at == rgb.size and off[-1] == len(files) and len(off) == len(rows()) + 1
    return out, str(z["pillow_version"])
