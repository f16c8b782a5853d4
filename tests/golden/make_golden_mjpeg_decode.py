"""Writes tests/golden/mjpeg_decode_cases.npz: the fixture of tests/test_mjpeg_decode_host.py and tests/test_mjpeg_decode_gpu.py.
Needs Pillow.

For the rows of `jpeg_decode_ref.rows()`, in that order: the complete files one behind the other (`files`, uint8, row i is
files[file_offsets[i]:file_offsets[i + 1]]) and the pixels Pillow (libjpeg-turbo) decodes from them (`rgb`, uint8, the rows' [H, W, 3]
arrays flattened one behind the other), plus the Pillow version string.  `jpeg_decode_ref.load_fixture` takes them apart again.  The files are Pillow's own
    Image.save(format='JPEG', quality=q, subsampling=s, restart_marker_blocks=r, optimize=o)
except the 'project/...' row: `ccvs_amd.tools.mjpeg.jpeg_header` with its DHT segments taken out, the scan the encoder's mirror
(`jpeg_ref.encode_scan`) writes, EOI -- a frame that relies on the Annex K tables, as Motion-JPEG frames may.

The script asserts that the spec mirror decodes every row to Pillow's pixels, that no inverse DCT value leaves -512 .. 511, and that
the rows contain what the entropy decoder must meet (each count > 0).  Run from the repository root:
    python tests/golden/make_golden_mjpeg_decode.py
"""
import io
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import jpeg_decode_ref as D  # noqa: E402
import jpeg_ref as R  # noqa: E402
from ccvs_amd.tools import mjpeg  # noqa: E402


def without_dht(header):
    segs, end = R.segments(header + b"\xff\xd9")
    assert end == len(header)
    out = b"\xff\xd8"
    for marker, payload in segs:
        if marker != 0xC4:
            out += bytes([0xFF, marker, (len(payload) + 2) >> 8, (len(payload) + 2) & 255]) + payload
    return out


def make_file(img, key, q, sub, rst, opt):
    if key.startswith("project/"):
        return without_dht(mjpeg.jpeg_header(img.shape[0], img.shape[1], q, rst)) + R.encode_scan(img, q, rst) + mjpeg.EOI
    buf = io.BytesIO()
    Image.fromarray(img, "RGB").save(buf, format="JPEG", quality=q, subsampling=sub, restart_marker_blocks=rst, optimize=opt)
    return buf.getvalue()


def main():
    out = {"pillow_version": np.array(PIL.__version__)}
    imgs = D.images()
    stats, rows_with, files, rgbs = D.new_stats(), {}, [], []
    for key, name, q, sub, rst, opt in D.rows():
        data = make_file(imgs[name], key, q, sub, rst, opt)
        rgb = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        one = D.new_stats()
        mine = D.decode(data, one)
        assert mine.shape == rgb.shape and np.array_equal(mine, rgb), (key, int((mine != rgb).sum()))
        for k, v in one.items():
            stats[k] = max(stats[k], v) if k == "max_dc_cat" else stats[k] + v
            rows_with[k] = rows_with.get(k, 0) + (v > 0)
        files.append(data)
        rgbs.append(rgb.reshape(-1))
    print("rows containing:", rows_with)
    print("totals:", stats)
    for k in ("stuffed", "zrl", "no_eob", "long_code", "rst_wrap", "partial_last", "partial_mcu_420"):
        assert rows_with[k] > 0, k
    assert stats["max_dc_cat"] == 11 and stats["idct_out_of_range"] == 0
    out["files"] = np.frombuffer(b"".join(files), dtype=np.uint8)
    out["file_offsets"] = np.cumsum([0] + [len(f) for f in files]).astype(np.int64)
    out["rgb"] = np.concatenate(rgbs)
    path = os.path.join(HERE, "mjpeg_decode_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(D.rows()), "rows, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
