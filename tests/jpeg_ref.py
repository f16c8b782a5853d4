"""Spec mirror of the JPEG encoder of the output stage (include/ccvs_hip_output.h states the arithmetic): numpy
and plain Python, one block at a time, never imported by `ccvs_amd`.  `encode_scan` gives the entropy-coded bytes of one frame -- what
lies between the SOS header and EOI, RSTn markers included -- and counts what the coder met on the way; tests/test_mjpeg_host.py holds
it against Pillow (libjpeg), tests/test_mjpeg_gpu.py holds the kernel against it.  It keeps its own copy of the Annex K tables: the host
tests compare them with the ones `ccvs_amd.tools.mjpeg` writes into the headers and with the ones Pillow writes into its files."""
import numpy as np

BASE_Q = np.array([
    [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
    [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32])
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]
# (bits, vals) of Annex K.3 - K.6; keys are the DHT class / id byte: 0x00 DC luminance, 0x01 DC chrominance, 0x10 / 0x11 the AC tables
_AC_TAIL = [r << 4 | c for r in range(16) for c in range(1, 11)]


def _ac_vals(head):
    """The table's first symbols as listed; the rest follow in ascending order."""
    head = [int(v, 16) for v in head.split()]
    return head + [v for v in _AC_TAIL if v not in head]


HUFF = {
    0x00: ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
    0x01: ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
    0x10: ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
           _ac_vals("01 02 03 00 04 11 05 12 21 31 41 06 13 51 61 07 22 71 14 32 81 91 a1 08 23 42 b1 c1 15 52 d1 f0 24 33 62 72 82")),
    0x11: ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119],
           _ac_vals("00 01 02 03 11 04 05 21 31 06 12 41 51 07 61 71 13 22 32 81 08 14 42 91 a1 b1 c1 09 23 33 52 f0 15 62 72 d1 0a 16 24 34 "
                    "e1 25 f1 17 18 19 1a 26 27 28 29 2a 35 36 37 38 39 3a 43 44 45 46 47 48 49 4a 53 54 55 56 57 58 59 5a 63 64 65 66 67 68 "
                    "69 6a 73 74 75 76 77 78 79 7a")),
}


def huff_codes(bits, vals):
    """symbol -> (code, length), T.81 Annex C."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def quant_tables(quality):
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((BASE_Q * scale + 50) // 100, 1, 255)


def default_restart(w):
    return min((w + 7) // 8, 32)


def _fix(x):
    return int(x * 65536 + 0.5)


def ycc(rgb):
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (_fix(.299) * r + _fix(.587) * g + _fix(.114) * b + 32768) >> 16
    cb = (-_fix(.16874) * r - _fix(.33126) * g + _fix(.5) * b + (128 << 16) + 32767) >> 16
    cr = (_fix(.5) * r - _fix(.41869) * g - _fix(.08131) * b + (128 << 16) + 32767) >> 16
    return np.stack([y, cb, cr], axis=-1)


_C = {name: int(c * 8192 + 0.5) for name, c in (("0.298", 0.298631336), ("0.390", 0.390180644), ("0.541", 0.541196100), ("0.765", 0.765366865),
                                               ("0.899", 0.899976223), ("1.175", 1.175875602), ("1.501", 1.501321110), ("1.847", 1.847759065),
                                               ("1.961", 1.961570560), ("2.053", 2.053119869), ("2.562", 2.562915447), ("3.072", 3.072711026))}


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, first):
    """jfdctint's pass over the last axis of d [..., 8] (int64)."""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    out = [None] * 8
    out[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    out[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * _C["0.541"]
    out[2] = _descale(z1 + t13 * _C["0.765"], n)
    out[6] = _descale(z1 - t12 * _C["1.847"], n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * _C["1.175"]
    t4, t5, t6, t7 = t4 * _C["0.298"], t5 * _C["2.053"], t6 * _C["3.072"], t7 * _C["1.501"]
    z1, z2 = -z1 * _C["0.899"], -z2 * _C["2.562"]
    z3, z4 = -z3 * _C["1.961"] + z5, -z4 * _C["0.390"] + z5
    out[7], out[5], out[3], out[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(out, axis=-1)


def quantised_blocks(rgb, quality):
    """int64 [MCU rows, MCU columns, 3, 64]: the quantised coefficients of every block in natural order."""
    h, w = rgb.shape[:2]
    hp, wp = -(-h // 8) * 8, -(-w // 8) * 8
    img = np.pad(ycc(rgb), ((0, hp - h), (0, wp - w), (0, 0)), mode="edge") - 128
    blocks = img.reshape(hp // 8, 8, wp // 8, 8, 3).transpose(0, 2, 4, 1, 3)          # [my, mx, c, row, col]
    d = _fdct_1d(blocks, True)                                                          # rows: along col
    d = _fdct_1d(d.swapaxes(-1, -2), False).swapaxes(-1, -2)                            # columns
    q = quant_tables(quality)[[0, 1, 1]].reshape(3, 8, 8) << 3
    mag = (np.abs(d) + (q >> 1)) // q
    return (np.sign(d) * mag).reshape(hp // 8, wp // 8, 3, 64)


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n, self.stuffed = bytearray(), 0, 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            self.n -= 8
            byte = (self.acc >> self.n) & 255
            self.out.append(byte)
            if byte == 255:
                self.out.append(0)
                self.stuffed += 1
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def new_stats():
    return {"stuffed": 0, "zrl": 0, "no_eob": 0, "max_dc_cat": 0, "max_ac_cat": 0, "rst_wrap": 0, "partial_last": 0, "intervals": 0}


def encode_scan(rgb, quality, restart_mcus=None, stats=None):
    """The scan of one uint8 [H, W, 3] frame as bytes.  `stats`: a dict of `new_stats()` to add this frame's counts to."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
    R = default_restart(rgb.shape[1]) if restart_mcus is None else int(restart_mcus)
    stats = new_stats() if stats is None else stats
    coef = quantised_blocks(rgb, quality)
    coef = coef.reshape(-1, 3, 64)
    dc_codes = [huff_codes(*HUFF[0x00]), huff_codes(*HUFF[0x01])]
    ac_codes = [huff_codes(*HUFF[0x10]), huff_codes(*HUFF[0x11])]
    out = bytearray()
    n_mcu = coef.shape[0]
    n_int = -(-n_mcu // R)
    for i in range(n_int):
        bits, pred = _Bits(), [0, 0, 0]
        mcus = range(i * R, min(n_mcu, (i + 1) * R))
        for m in mcus:
            for c in range(3):
                t = 0 if c == 0 else 1
                zz = [int(coef[m, c, ZIGZAG[k]]) for k in range(64)]
                diff, pred[c] = zz[0] - pred[c], zz[0]
                cat = abs(diff).bit_length()
                stats["max_dc_cat"] = max(stats["max_dc_cat"], cat)
                bits.put(*dc_codes[t][cat])
                bits.put((diff - 1 if diff < 0 else diff) & ((1 << cat) - 1), cat)
                run = 0
                for k in range(1, 64):
                    v = zz[k]
                    if v == 0:
                        run += 1
                        continue
                    while run > 15:
                        bits.put(*ac_codes[t][0xF0])
                        stats["zrl"] += 1
                        run -= 16
                    cat = abs(v).bit_length()
                    stats["max_ac_cat"] = max(stats["max_ac_cat"], cat)
                    bits.put(*ac_codes[t][run << 4 | cat])
                    bits.put((v - 1 if v < 0 else v) & ((1 << cat) - 1), cat)
                    run = 0
                if run:
                    bits.put(*ac_codes[t][0x00])
                else:
                    stats["no_eob"] += 1
        bits.flush()
        stats["stuffed"] += bits.stuffed
        out += bits.out
        if i < n_int - 1:
            out += bytes([0xFF, 0xD0 + (i & 7)])
            stats["rst_wrap"] += int(i >= 8 and (i & 7) == 0)
        elif len(mcus) < R:
            stats["partial_last"] += 1
    stats["intervals"] += n_int
    return bytes(out)


# ------------------------------------------------------------------ JPEG files
def segments(data):
    """[(marker, payload)] of the header of a JPEG file up to and including SOS, and the offset at which the scan starts."""
    assert data[:2] == b"\xff\xd8", "no SOI"
    out, i = [], 2
    while True:
        assert data[i] == 0xFF and data[i + 1] not in (0x00, 0xFF), f"no marker at {i}"
        marker, length = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        assert length >= 2 and i + 2 + length <= len(data), f"segment {marker:#x} at {i} has length {length}"
        out.append((marker, bytes(data[i + 4:i + 2 + length])))
        i += 2 + length
        if marker == 0xDA:
            return out, i


def scan_of(data):
    """The entropy-coded bytes of a baseline JPEG file with one scan."""
    assert data[-2:] == b"\xff\xd9", "no EOI"
    return bytes(data[segments(data)[1]:-2])


def dht_tables(segs):
    """{class/id byte: (bits, vals)} of the DHT segments of `segments(...)`."""
    out = {}
    for marker, seg in segs:
        p = 0
        while marker == 0xC4 and p < len(seg):
            bits = list(seg[p + 1:p + 17])
            out[seg[p]] = (bits, list(seg[p + 17:p + 17 + sum(bits)]))
            p += 17 + sum(bits)
    return out


# ------------------------------------------------------------------ the case table of the fixture tests/golden/mjpeg_cases.npz
def _noise(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def _smooth(h, w):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    r = 127.5 + 127.5 * np.sin(2 * np.pi * (x / w + 0.3 * y / h))
    g = 255.0 * (x + y) / (h + w - 2)
    b = 127.5 + 127.5 * np.cos(2 * np.pi * (1.5 * y / h - 0.5 * x / w)) * np.exp(-((x - w / 2) ** 2 + (y - h / 2) ** 2) / (0.18 * h * w))
    return np.clip(np.rint(np.stack([r, g, b], axis=-1)), 0, 255).astype(np.uint8)


def _checker(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)


def _sparse(h, w, seed):
    return np.repeat(((np.random.RandomState(seed).rand(h, w) < 0.02) * 255).astype(np.uint8)[..., None], 3, axis=2)


def _blocks(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.repeat(((((x >> 3) + (y >> 3)) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)


ALL_Q = (100, 90, 75, 30, 5)
# name -> (image, qualities, restart interval in MCUs: None = the default, min(MCUs per row, 32))
CASES = {
    "constant_8x8": (lambda: np.full((8, 8, 3), (100, 150, 200), dtype=np.uint8), ALL_Q, None),        # EOB-only blocks
    "noise_8x8": (lambda: _noise(8, 8, 1), ALL_Q, None),
    "noise_24x40": (lambda: _noise(24, 40, 2), ALL_Q, None),                                            # q = 100: the scan exceeds the raw size
    "noise_13x21": (lambda: _noise(13, 21, 3), ALL_Q, None),                                            # edge replication on both axes
    "checker_16x16": (lambda: _checker(16, 16), ALL_Q, None),
    "smooth_64x64": (lambda: _smooth(64, 64), ALL_Q, None),
    "sparse_32x32": (lambda: _sparse(32, 32, 4), ALL_Q, None),
    "blocks_16x16": (lambda: _blocks(16, 16), ALL_Q, None),                                             # black / white blocks: DC category 11
    "noise_72x8": (lambda: _noise(72, 8, 5), ALL_Q, None),                                              # nine intervals: RST7 -> RST0
    "noise_88x8": (lambda: _noise(88, 8, 8), (100, 30), None),                                          # eleven intervals: the counter wraps twice over
    "noise_16x40_r3": (lambda: _noise(16, 40, 6), ALL_Q, 3),                                            # intervals straddle MCU rows, last one partial
    "noise_8x520": (lambda: _noise(8, 520, 7), ALL_Q, None),                                            # 65 MCUs per row: intervals of 32 / 32 / 1
    "smooth_256x256": (lambda: _smooth(256, 256), (90,), None),                                         # the workload's 32-MCU interval
}


def rows():
    """[(key, case name, quality, restart interval)] of the fixture."""
    out = []
    for name, (make, qualities, r) in CASES.items():
        h, w = make().shape[:2]
        for q in qualities:
            out.append((f"{name}/q{q}", name, q, default_restart(w) if r is None else r))
    return out
