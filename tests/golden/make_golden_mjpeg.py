"""Writes tests/golden/mjpeg_cases.npz: the fixture of tests/test_mjpeg_host.py and tests/test_mjpeg_gpu.py.  Needs Pillow.

For every case of `jpeg_ref.CASES`: the input image (`<case>/in`, uint8 [H, W, 3]), and for every (quality, restart interval) row the
complete file Pillow (libjpeg) writes for it (`<case>/q<quality>`, uint8), 4:4:4, standard Huffman tables:
    Image.save(format='JPEG', quality=q, subsampling=0, restart_marker_blocks=R)
plus the Pillow version string.  Run from the repository root:  python tests/golden/make_golden_mjpeg.py
"""
import io
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_ref as R  # noqa: E402


def pillow_file(rgb, quality, restart_mcus):
    buf = io.BytesIO()
    Image.fromarray(rgb, "RGB").save(buf, format="JPEG", quality=quality, subsampling=0, restart_marker_blocks=restart_mcus)
    return buf.getvalue()


def main():
    out = {"pillow_version": np.array(PIL.__version__)}
    for name, (make, _, _) in R.CASES.items():
        out[name + "/in"] = make()
    for key, name, q, r in R.rows():
        out[key] = np.frombuffer(pillow_file(out[name + "/in"], q, r), dtype=np.uint8)
    path = os.path.join(HERE, "mjpeg_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(R.rows()), "rows, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
