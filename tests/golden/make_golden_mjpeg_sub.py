"""Writes tests/golden/mjpeg_sub_cases.npz: the fixture of tests/test_mjpeg_sub_host.py and tests/test_mjpeg_sub_gpu.py.  Needs Pillow.

For every case of `jpeg_sub_ref.CASES`: the input image (`<case>/in`, uint8 [H, W, 3]), and for every (sampling, quality, restart
interval) row the complete file Pillow (libjpeg) writes for it (`<case>/s<sampling>/q<quality>`, uint8), standard Huffman tables:
    Image.save(format='JPEG', quality=q, subsampling=1 | 2, restart_marker_blocks=R)
plus the Pillow version string.  Run from the repository root:  python tests/golden/make_golden_mjpeg_sub.py
"""
import io
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_sub_ref as S  # noqa: E402


def pillow_file(rgb, quality, sampling, restart_mcus):
    buf = io.BytesIO()
    Image.fromarray(rgb, "RGB").save(buf, format="JPEG", quality=quality, subsampling=sampling, restart_marker_blocks=restart_mcus)
    return buf.getvalue()


def main():
    out = {"pillow_version": np.array(PIL.__version__)}
    for name, (make, _, _) in S.CASES.items():
        out[name + "/in"] = make()
    for key, name, s, q, r in S.rows():
        out[key] = np.frombuffer(pillow_file(out[name + "/in"], q, s, r), dtype=np.uint8)
    path = os.path.join(HERE, "mjpeg_sub_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(S.rows()), "rows, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
