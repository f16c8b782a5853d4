"""Writes tests/golden/mjpeg_opt_cases.npz: the fixture of tests/test_mjpeg_opt_host.py and tests/test_mjpeg_opt_gpu.py.  Needs Pillow.

For every image of `jpeg_opt_ref.images()`: the input (`<image>/in`, uint8 [H, W, 3]), and for every (sampling, quality, restart
interval) row the complete file Pillow (libjpeg) writes for it with per-frame optimal Huffman tables (`<row key>`, uint8):
    Image.save(format='JPEG', quality=q, subsampling=s, restart_marker_blocks=R, optimize=True)
The 256 x 256 row that forces the 16-bit limiter is stored as its four DHT payloads (`<key>/dht`, uint8 [4, 272]: class / id byte
dropped, bits[16] + vals, zero-padded), the length of its scan and the scan's SHA-256 (`<key>/scan_len`, `<key>/scan_sha256`); its input
is `jpeg_opt_ref.limiter_image()`.  Plus the Pillow version string.  Run from the repository root:
    python tests/golden/make_golden_mjpeg_opt.py
"""
import hashlib
import io
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_opt_ref as O  # noqa: E402


def pillow_file(rgb, quality, sampling, restart_mcus, optimize=True):
    buf = io.BytesIO()
    Image.fromarray(rgb, "RGB").save(buf, format="JPEG", quality=quality, subsampling=sampling, restart_marker_blocks=restart_mcus, optimize=optimize)
    return buf.getvalue()


def digest(data):
    """(DHT payloads uint8 [4, 272], scan length, SHA-256 of the scan) of a file."""
    segs, start = O.segments(data)
    return O.spec_bytes(O.dht_tables(segs)), len(data) - 2 - start, hashlib.sha256(data[start:-2]).hexdigest()


def main():
    out = {"pillow_version": np.array(PIL.__version__)}
    for name in O.images():
        out[name + "/in"] = O.image(name)
    for key, name, s, q, r in O.rows():
        out[key] = np.frombuffer(pillow_file(out[name + "/in"], q, s, r), dtype=np.uint8)
    key, name, s, q, r = O.LIMITER_ROW
    dht, n, sha = digest(pillow_file(O.image(name), q, s, r))
    out[key + "/dht"], out[key + "/scan_len"], out[key + "/scan_sha256"] = dht, np.array(n), np.array(sha)
    path = os.path.join(HERE, "mjpeg_opt_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(O.rows()) + 1, "rows, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
