"""Spec mirror of the subsampled modes of the JPEG encoder (4:2:2 = h2v1, 4:2:0 = h2v2; include/ccvs_hip_output_sampled.h states the
arithmetic): numpy and plain Python, never imported by `ccvs_amd`.  The shared pieces -- colour conversion, jfdctint, the quantiser and
Huffman tables, the bit writer, the file walkers and the image makers -- are tests/jpeg_ref.py's, imported and not copied; what is new
here is what sampling adds: the chrominance planes' box filter with libjpeg's alternating bias, the two steps of vertical padding, the
MCU of 4 or 6 blocks, dummy blocks and the luminance predictor that runs through them.  tests/test_mjpeg_sub_host.py holds
`encode_scan_sub` against Pillow (libjpeg), tests/test_mjpeg_sub_gpu.py holds the kernel against it."""
import numpy as np

from jpeg_ref import ALL_Q, HUFF, ZIGZAG, _Bits, _blocks, _fdct_1d, _noise, _smooth, huff_codes, quant_tables, scan_of, segments, ycc  # noqa: F401

FACTORS = ((1, 1), (2, 1), (2, 2))       # luminance (h, v) per sampling code: 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0 (Pillow's `subsampling`)
MAX_RESTART = (32, 24, 16)               # 96 blocks per interval / blocks per MCU


def mcu_grid(h, w, sampling):
    hs, vs = FACTORS[sampling]
    return -(-w // (8 * hs)), -(-h // (8 * vs))


def default_restart(w, sampling=0):
    return min(mcu_grid(1, w, sampling)[0], MAX_RESTART[sampling])


def new_stats():
    return {"stuffed": 0, "zrl": 0, "no_eob": 0, "max_dc_cat": 0, "max_ac_cat": 0, "rst_wrap": 0, "partial_last": 0, "intervals": 0,
            "dummy_right": 0, "dummy_bottom": 0, "mcu_with_both": 0}


def downsample(plane, hs, vs, rows_out, cols_out):
    """A full-resolution chrominance plane [h, w] -> [rows_out, cols_out] (multiples of 8: the component's size in blocks)."""
    h, w = plane.shape
    p = np.pad(plane, ((0, 0), (0, hs * cols_out - w)), mode="edge")                 # the right column, up to the width the blocks read
    p = np.pad(p, ((0, -h % vs), (0, 0)), mode="edge")                               # the bottom row, up to a multiple of the vertical factor only
    x_odd = np.arange(cols_out) & 1
    if (hs, vs) == (2, 2):
        p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 1 + x_odd) >> 2
    elif (hs, vs) == (2, 1):
        p = (p[:, 0::2] + p[:, 1::2] + x_odd) >> 1
    return np.pad(p, ((0, rows_out - p.shape[0]), (0, 0)), mode="edge")              # the last DOWN-SAMPLED row, up to whole blocks


def _quantised(plane, table):
    """int64 [block rows, block columns, 64] (natural order) of a plane whose sides are multiples of 8."""
    hb, wb = plane.shape[0] // 8, plane.shape[1] // 8
    blocks = (plane - 128).reshape(hb, 8, wb, 8).transpose(0, 2, 1, 3)
    d = _fdct_1d(blocks, True)
    d = _fdct_1d(d.swapaxes(-1, -2), False).swapaxes(-1, -2)
    q = table.reshape(8, 8) << 3
    return (np.sign(d) * ((np.abs(d) + (q >> 1)) // q)).reshape(hb, wb, 64)


def component_blocks(rgb, quality, sampling):
    """[Y, Cb, Cr]: the quantised blocks of every component, each at its own size in blocks -- ceil(w ch / (8 hs)) x ceil(h cv / (8 vs)),
    not rounded up to whole MCUs."""
    hs, vs = FACTORS[sampling]
    h, w = rgb.shape[:2]
    img = ycc(rgb)
    tables = quant_tables(quality)
    hb, wb = -(-h // 8), -(-w // 8)
    y = np.pad(img[..., 0], ((0, 8 * hb - h), (0, 8 * wb - w)), mode="edge")
    mx, my = mcu_grid(h, w, sampling)
    return [_quantised(y, tables[0])] + [_quantised(downsample(img[..., c], hs, vs, 8 * my, 8 * mx), tables[1]) for c in (1, 2)]


def _code_block(bits, zz, diff, dc_codes, ac_codes, stats):
    cat = abs(diff).bit_length()
    stats["max_dc_cat"] = max(stats["max_dc_cat"], cat)
    bits.put(*dc_codes[cat])
    bits.put((diff - 1 if diff < 0 else diff) & ((1 << cat) - 1), cat)
    run = 0
    for k in range(1, 64):
        v = zz[k]
        if v == 0:
            run += 1
            continue
        while run > 15:
            bits.put(*ac_codes[0xF0])
            stats["zrl"] += 1
            run -= 16
        cat = abs(v).bit_length()
        stats["max_ac_cat"] = max(stats["max_ac_cat"], cat)
        bits.put(*ac_codes[run << 4 | cat])
        bits.put((v - 1 if v < 0 else v) & ((1 << cat) - 1), cat)
        run = 0
    if run:
        bits.put(*ac_codes[0x00])
    else:
        stats["no_eob"] += 1


def encode_scan_sub(rgb, quality, sampling, restart_mcus=None, stats=None):
    """The scan of one uint8 [H, W, 3] frame as bytes, for sampling 0 / 1 / 2.  `stats`: a dict of `new_stats()` to add the counts to."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3 and sampling in (0, 1, 2)
    hs, vs = FACTORS[sampling]
    h, w = rgb.shape[:2]
    R = default_restart(w, sampling) if restart_mcus is None else int(restart_mcus)
    assert 1 <= R <= MAX_RESTART[sampling]
    stats = new_stats() if stats is None else stats
    Y, Cb, Cr = component_blocks(rgb, quality, sampling)
    dc_codes = [huff_codes(*HUFF[0x00]), huff_codes(*HUFF[0x01])]
    ac_codes = [huff_codes(*HUFF[0x10]), huff_codes(*HUFF[0x11])]
    mcux, mcuy = mcu_grid(h, w, sampling)
    n_mcu = mcux * mcuy
    n_int = -(-n_mcu // R)
    out = bytearray()
    zero = [0] * 64
    for i in range(n_int):
        bits, pred = _Bits(), [0, 0, 0]
        mcus = range(i * R, min(n_mcu, (i + 1) * R))
        for m in mcus:
            my, mx = divmod(m, mcux)
            last, right, bottom = None, 0, 0                      # `last`: the DC of the block before this one in the MCU
            for by in range(vs):
                for bx in range(hs):
                    yy, xx = my * vs + by, mx * hs + bx
                    if yy < Y.shape[0] and xx < Y.shape[1]:
                        zz = [int(Y[yy, xx, ZIGZAG[k]]) for k in range(64)]
                    else:                                           # a dummy block: no AC, the DC of the block before it (maybe a dummy too)
                        zz = [last] + zero[1:]
                        right += xx >= Y.shape[1]
                        bottom += yy >= Y.shape[0]
                    _code_block(bits, zz, zz[0] - pred[0], dc_codes[0], ac_codes[0], stats)
                    pred[0] = last = zz[0]
            stats["dummy_right"] += right
            stats["dummy_bottom"] += bottom
            stats["mcu_with_both"] += int(right > 0 and bottom > 0)
            for c, plane in ((1, Cb), (2, Cr)):
                zz = [int(plane[my, mx, ZIGZAG[k]]) for k in range(64)]
                _code_block(bits, zz, zz[0] - pred[c], dc_codes[1], ac_codes[1], stats)
                pred[c] = zz[0]
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


# ------------------------------------------------------------------ the case table of the fixture tests/golden/mjpeg_sub_cases.npz
SAMPLINGS = (1, 2)
# name -> (image, qualities, restart interval in MCUs: None = the default, one row of MCUs capped at the sampling's limit)
CASES = {
    "noise_8x8": (lambda: _noise(8, 8, 21), ALL_Q, None),                      # one MCU whose luminance blocks are mostly dummies
    "noise_1x1": (lambda: _noise(1, 1, 22), ALL_Q, None),
    "smooth_8x8": (lambda: _smooth(64, 64)[20:28, 30:38].copy(), (90,), None),
    "noise_16x16": (lambda: _noise(16, 16, 23), ALL_Q, None),                  # exactly one 4:2:0 MCU, no padding anywhere
    "blocks_16x16": (lambda: _blocks(16, 16), (100, 30), None),                # black / white luminance blocks: DC category 11
    "noise_24x40": (lambda: _noise(24, 40, 24), ALL_Q, None),                  # 4:2:0: a bottom row of dummies; width 40: a right column too
    "smooth_24x40": (lambda: _smooth(24, 40), (90, 30), None),
    "noise_40x24": (lambda: _noise(40, 24, 25), (100, 75, 5), None),                  # width 24: right dummies in both samplings
    "noise_24x24": (lambda: _noise(24, 24, 26), (100, 90, 30), None),                  # the corner MCU has both
    "noise_13x21": (lambda: _noise(13, 21, 27), ALL_Q, None),                  # odd rows and columns: both padding steps
    "noise_17x33": (lambda: _noise(17, 33, 28), ALL_Q, None),
    "smooth_17x33": (lambda: _smooth(17, 33), (90, 30), None),
    "noise_9x9": (lambda: _noise(9, 9, 29), ALL_Q, None),
    "noise_33x7": (lambda: _noise(33, 7, 30), ALL_Q, None),
    "noise_7x33": (lambda: _noise(7, 33, 31), ALL_Q, None),
    "noise_25x72": (lambda: _noise(25, 72, 32), (100, 30), None),
    "smooth_25x72": (lambda: _smooth(25, 72), (75,), None),
    "noise_16x520": (lambda: _noise(16, 520, 33), (100, 30), None),            # 33 MCUs per row: 16 / 16 / 1 in 4:2:0, 24 / 24 / 18 over two rows in 4:2:2
    "noise_280x8": (lambda: _noise(280, 8, 34), (100, 30), None),              # 18 (4:2:0) / 35 (4:2:2) intervals: RSTn wraps twice and more
    "noise_56x72_r3": (lambda: _noise(56, 72, 35), (90, 5), 3),           # intervals straddle MCU rows, the last one is partial
    "smooth_256x256": (lambda: _smooth(256, 256), (90,), None),                # the workload's frame: 16 MCUs = 96 blocks per interval in 4:2:0
}


def rows():
    """[(key, case name, sampling, quality, restart interval)] of the fixture."""
    out = []
    for name, (make, qualities, r) in CASES.items():
        w = make().shape[1]
        for s in SAMPLINGS:
            for q in qualities:
                out.append((f"{name}/s{s}/q{q}", name, s, q, default_restart(w, s) if r is None else r))
    return out
