"""Writes tests/golden/ingest_pil.npz: Pillow's own `Image.resize(..., BILINEAR)` of the seeded random frames of tests/ingest_ref.py for
every shape of `ingest_ref.SHAPES`, so that the GPU tests need no Pillow.

    python tests/golden/make_golden_ingest.py

Per shape (key = `ingest_ref.shape_id`): `<id>/out` uint8 [Ho, Wo, 3], Pillow's result for frame 0 of `ingest_ref.source(shape)` cropped
to the shape's box; `<id>/sha` the SHA-256 of that source frame's bytes; `<id>/in` the source frame itself where it is at most 32 KB
(the larger ones are regenerated from their seed and checked against the digest).  `pillow_version` records the Pillow that made them.
The file stays under 300 KB."""
import hashlib
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ingest_ref as R  # noqa: E402


def pil_stage(frame, box, size):
    img = Image.fromarray(frame, "RGB")
    if box is not None:
        top, left, h, w = box
        img = img.crop((left, top, left + w, top + h))
    return np.asarray(img.resize((size[1], size[0]), Image.BILINEAR))


def main():
    out = {"pillow_version": np.array(PIL.__version__)}
    for shape in R.SHAPES:
        _, box, size = shape
        key = R.shape_id(shape)
        frame = R.source(shape)[0]
        out[key + "/out"] = pil_stage(frame, box, size)
        out[key + "/sha"] = np.array(hashlib.sha256(frame.tobytes()).hexdigest())
        if frame.nbytes <= 32 << 10:
            out[key + "/in"] = frame
        assert out[key + "/out"].shape == (*size, 3) and out[key + "/out"].dtype == np.uint8
    path = os.path.join(HERE, "ingest_pil.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes, Pillow", PIL.__version__)
    assert os.path.getsize(path) < 300 << 10


if __name__ == "__main__":
    main()
