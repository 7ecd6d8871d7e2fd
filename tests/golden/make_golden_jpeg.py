#!/usr/bin/env python3
"""Golden fixture for the JPEG stage's closeness to a real codec: Pillow (libjpeg) round trips of jpeg_refs.fixture_image at the sizes
and qualities below, at subsampling 0 (4:4:4) and 2 (4:2:0), written to tests/golden/jpeg_pil.npz.  Keys: in_{H}x{W}_q{Q} = the input,
uint8 [H, W, 3]; out_{H}x{W}_q{Q}_s{subsampling} = what Pillow decodes from what it encoded; qt_q{Q} = the two quantisation tables of
those files, int32 [2, 64] row-major.  tests/test_jpeg_refs.py reads only the npz.  Needs Pillow.  Re-run:  python tests/golden/make_golden_jpeg.py"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from jpeg_refs import fixture_image  # noqa: E402

SIZES = ((24, 24), (17, 13), (8, 8), (48, 40), (9, 31), (3, 20))           # H, W
QUALITIES = (10, 30, 50, 75, 90, 95)

if __name__ == "__main__":
    out = {}
    for H, W in SIZES:
        for q in QUALITIES:
            img = fixture_image(H, W, q)
            out[f"in_{H}x{W}_q{q}"] = img
            for sub in (0, 2):
                buf = io.BytesIO()
                Image.fromarray(img).save(buf, format="JPEG", quality=q, subsampling=sub)
                back = Image.open(io.BytesIO(buf.getvalue()))
                out[f"qt_q{q}"] = np.array([back.quantization[0], back.quantization[1]], np.int32)    # row-major since Pillow 8.3
                out[f"out_{H}x{W}_q{q}_s{sub}"] = np.asarray(back.convert("RGB"))
    path = os.path.join(HERE, "jpeg_pil.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")
