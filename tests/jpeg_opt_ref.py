"""Spec mirror of the optimised-Huffman mode of the JPEG encoder (include/ccvs_hip_output_optimized.h states
the contract): numpy and plain Python, never imported by `ccvs_amd`.  The coefficients are tests/jpeg_sub_ref.py's (`component_blocks`,
all three samplings), the bit writer and the file walkers tests/jpeg_ref.py's -- imported, not copied.  What is new here is libjpeg's
`optimize_coding`: the symbols a frame's scan emits are counted per table (`symbol_counts`), `jpeg_gen_optimal_table` turns each
histogram into (bits, vals) (`optimal_table`), and the same symbols are then coded with those tables (`encode_scan_optimized`).
tests/test_mjpeg_opt_host.py holds all three against Pillow (libjpeg), tests/test_mjpeg_opt_gpu.py holds the kernels against the fixture."""
import numpy as np

from jpeg_ref import HUFF, ZIGZAG, _Bits, _checker, _noise, _smooth, _sparse, huff_codes, scan_of, segments, dht_tables  # noqa: F401
from jpeg_sub_ref import FACTORS, MAX_RESTART, component_blocks, default_restart, mcu_grid  # noqa: F401

# the four tables of a frame in the order libjpeg writes their DHT segments (and the rows of the `tables` tensor): class / id bytes
TABLE_KEYS = (0x00, 0x10, 0x01, 0x11)      # DC luminance, AC luminance, DC chrominance, AC chrominance
MAX_CLEN = 32                              # libjpeg's limit on the depth of the tree before limiting


def _block_symbols(zz, diff, t, out):
    """What `code_block` emits for one block, as (table, symbol, extra bits, their number): t = 0 luminance, 1 chrominance."""
    cat = abs(diff).bit_length()
    out.append((2 * t, cat, (diff - 1 if diff < 0 else diff) & ((1 << cat) - 1), cat))
    run = 0
    for k in range(1, 64):
        v = zz[k]
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append((2 * t + 1, 0xF0, 0, 0))
            run -= 16
        cat = abs(v).bit_length()
        out.append((2 * t + 1, run << 4 | cat, (v - 1 if v < 0 else v) & ((1 << cat) - 1), cat))
        run = 0
    if run:
        out.append((2 * t + 1, 0x00, 0, 0))


def scan_symbols(rgb, quality, sampling=0, restart_mcus=None):
    """[interval][(table 0 .. 3 in TABLE_KEYS order, symbol, extra bits, number of extra bits)] of one uint8 [H, W, 3] frame: the MCU
    walk of `jpeg_sub_ref.encode_scan_sub` (dummy luminance blocks, the predictors reset at every interval) without the coding."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3 and sampling in (0, 1, 2)
    hs, vs = FACTORS[sampling]
    h, w = rgb.shape[:2]
    R = default_restart(w, sampling) if restart_mcus is None else int(restart_mcus)
    assert 1 <= R <= MAX_RESTART[sampling]
    Y, Cb, Cr = component_blocks(rgb, quality, sampling)
    mcux, mcuy = mcu_grid(h, w, sampling)
    n_mcu = mcux * mcuy
    intervals = []
    for i in range(-(-n_mcu // R)):
        out, pred = [], [0, 0, 0]
        for m in range(i * R, min(n_mcu, (i + 1) * R)):
            my, mx = divmod(m, mcux)
            last = None
            for by in range(vs):
                for bx in range(hs):
                    yy, xx = my * vs + by, mx * hs + bx
                    if yy < Y.shape[0] and xx < Y.shape[1]:
                        zz = [int(Y[yy, xx, ZIGZAG[k]]) for k in range(64)]
                    else:                                   # a dummy block: no AC, the DC of the block before it in the MCU
                        zz = [last] + [0] * 63
                    _block_symbols(zz, zz[0] - pred[0], 0, out)
                    pred[0] = last = zz[0]
            for c, plane in ((1, Cb), (2, Cr)):
                zz = [int(plane[my, mx, ZIGZAG[k]]) for k in range(64)]
                _block_symbols(zz, zz[0] - pred[c], 1, out)
                pred[c] = zz[0]
        intervals.append(out)
    return intervals


def symbol_counts(rgb, quality, sampling=0, restart_mcus=None, symbols=None):
    """int32 [4, 257]: how often the frame's scan emits every symbol of every table (TABLE_KEYS order; slot 256 stays 0)."""
    counts = np.zeros((4, 257), dtype=np.int32)
    for interval in scan_symbols(rgb, quality, sampling, restart_mcus) if symbols is None else symbols:
        for t, sym, _, _ in interval:
            counts[t, sym] += 1
    return counts


def optimal_table(counts):
    """libjpeg's `jpeg_gen_optimal_table` on the counts of one table (256 or 257 values; value 256 is ignored): (bits [16], vals,
    depth) -- `depth` is the longest code BEFORE the Annex K.2 adjustment to 16 bits."""
    freq = [int(c) for c in list(counts)[:256]] + [1]       # the pseudo-symbol 256 keeps the all-ones code unused
    assert all(f >= 0 for f in freq)
    codesize, others = [0] * 257, [-1] * 257
    while True:
        c1, v = -1, 1000000000
        for i in range(257):
            if freq[i] and freq[i] <= v:                    # `<=`: ties go to the larger symbol
                v, c1 = freq[i], i
        c2, v = -1, 1000000000
        for i in range(257):
            if freq[i] and freq[i] <= v and i != c1:
                v, c2 = freq[i], i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    depth = max(codesize)
    assert depth <= MAX_CLEN, "libjpeg stops here (JERR_HUFF_CLEN_OVERFLOW)"
    bits = [0] * (MAX_CLEN + 1)
    for s in codesize:
        if s:
            bits[s] += 1
    for i in range(MAX_CLEN, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1                                            # the pseudo-symbol's code
    vals = [j for i in range(1, MAX_CLEN + 1) for j in range(256) if codesize[j] == i]
    return bits[1:17], vals, depth


def frame_tables(counts):
    """{class/id byte: (bits, vals)} of the four histograms of `symbol_counts`, and the four depths before limiting."""
    tables, depths = {}, []
    for t, key in enumerate(TABLE_KEYS):
        bits, vals, depth = optimal_table(counts[t])
        tables[key] = (bits, vals)
        depths.append(depth)
    return tables, depths


def code_symbols(intervals, tables):
    """The scan of `scan_symbols(...)` coded with `tables` ({class/id byte: (bits, vals)}): bytes, RSTn markers included."""
    codes = [huff_codes(*tables[key]) for key in TABLE_KEYS]
    out = bytearray()
    for i, interval in enumerate(intervals):
        bits = _Bits()
        for t, sym, extra, n in interval:
            bits.put(*codes[t][sym])
            bits.put(extra, n)
        bits.flush()
        out += bits.out
        if i < len(intervals) - 1:
            out += bytes([0xFF, 0xD0 + (i & 7)])
    return bytes(out)


def scan_bits(intervals, tables):
    """The number of bits of the symbols of `intervals` under `tables`, padding, stuffing and markers not counted."""
    codes = [huff_codes(*tables[key]) for key in TABLE_KEYS]
    return sum(codes[t][sym][1] + n for interval in intervals for t, sym, _, n in interval)


def encode_scan_optimized(rgb, quality, sampling=0, restart_mcus=None):
    """(scan bytes, {class/id byte: (bits, vals)}, depths before limiting) of one frame, as libjpeg writes it with optimize_coding."""
    intervals = scan_symbols(rgb, quality, sampling, restart_mcus)
    tables, depths = frame_tables(symbol_counts(None, 0, symbols=intervals))
    return code_symbols(intervals, tables), tables, depths


def spec_bytes(tables):
    """uint8 [4, 272] of a frame's tables: bits[16] + vals, zero-padded -- one row of the encoder's `tables` tensor."""
    out = np.zeros((4, 272), dtype=np.uint8)
    for t, key in enumerate(TABLE_KEYS):
        bits, vals = tables[key]
        out[t, :16] = bits
        out[t, 16:16 + len(vals)] = vals
    return out


# ------------------------------------------------------------------ the case table of the fixture tests/golden/mjpeg_opt_cases.npz
def _flat(h, w):
    return np.full((h, w, 3), (90, 160, 200), dtype=np.uint8)


def limiter_image(seed=1):
    """256 x 256: Gaussian noise around 128 per 8 x 8 block, the block's amplitude 127 exp(U(-6, 0)).  At quality 100 the rare long runs
    and large categories of the quiet blocks beside the common symbols of the loud ones make a tree deeper than 16."""
    rng = np.random.default_rng(seed)
    amp = 127.0 * np.exp(rng.uniform(-6.0, 0.0, size=(32, 32)))
    noise = rng.standard_normal((256, 256, 3)) * np.kron(amp, np.ones((8, 8)))[..., None]
    return np.clip(np.rint(128.0 + noise), 0, 255).astype(np.uint8)


SIZES = ((8, 8), (16, 16), (21, 33), (40, 24), (64, 64))
CONTENT = {"noise": lambda h, w: _noise(h, w, 100 + h), "smooth": _smooth, "checker": _checker, "sparse": lambda h, w: _sparse(h, w, 200 + w),
           "flat": _flat}
QUALITIES = (10, 50, 90, 100)
LIMITER = "limiter_256x256"                # stored as DHT payloads and a SHA-256 of the scan: the file itself would double the fixture


def image(name):
    if name == LIMITER:
        return limiter_image()
    kind, size = name.split("_")
    h, w = (int(v) for v in size.split("x"))
    return CONTENT[kind](h, w)


def images():
    return [f"{kind}_{h}x{w}" for h, w in SIZES for kind in CONTENT]


def rows():
    """[(key, image name, sampling, quality, restart interval)].  Every image at every sampling: the four qualities at the default
    interval (one row of MCUs), and the intervals 1 (more than 8 intervals from 16 x 16 / 40 x 24 on: RSTn wraps), 3 and the sampling's
    largest (larger than every frame but the 64 x 64 one at 4:4:4 and 4:2:2) at one quality that walks through the four."""
    out, k = [], 0
    for name in images():
        w = image(name).shape[1]
        for s in (0, 1, 2):
            for q in QUALITIES:
                out.append((f"{name}/s{s}/q{q}/r{default_restart(w, s)}", name, s, q, default_restart(w, s)))
            for r in (1, 3, MAX_RESTART[s]):
                q = QUALITIES[k % 4]
                k += 1
                key = f"{name}/s{s}/q{q}/r{r}"
                if all(key != o[0] for o in out):
                    out.append((key, name, s, q, r))
    return out


LIMITER_ROW = (f"{LIMITER}/s0/q100/r32", LIMITER, 0, 100, 32)
