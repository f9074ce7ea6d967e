#!/usr/bin/env python3
"""Write textures/baseline_444_restart.jpg, the JPEG the C++ decoder is held to the Python reader on (tests/test_host_cpp.py).

    python tests/golden/make_jpeg_fixture.py        (needs Pillow; the fixture is committed)

A seeded picture -- smooth gradients, a grid of flat colour patches with hard edges, noise, clipped pixels -- written the way a
photo editor writes one: baseline, three components at full resolution (4:4:4), two quantisation tables, a restart interval
that is not a divisor of the MCU rows, a size that is not a multiple of 8, and EXIF / ICC / comment segments to be skipped."""
import io
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "textures", "baseline_444_restart.jpg")


def picture(width=301, height=213, seed=11):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    img = np.stack([255 * x / width, 255 * y / height, 128 + 100 * np.sin(x / 17.0) * np.cos(y / 23.0)], axis=-1)
    rows, cols = 4, 6
    ph, pw = height // (rows + 1), width // (cols + 1)
    for r in range(rows):
        for c in range(cols):
            y0, x0 = ph // 2 + r * ph + 3, pw // 2 + c * pw + 3
            img[y0 - 3:y0 + ph - 3, x0 - 3:x0 + pw - 3] = 20  # dark frame around each patch
            img[y0:y0 + ph - 6, x0:x0 + pw - 6] = rng.integers(0, 256, 3)
    img += rng.normal(0.0, 6.0, img.shape)
    img[:9, :9] = 255  # a saturated corner and a black one
    img[-9:, -9:] = 0
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def main():
    exif = Image.Exif()
    exif[0x010E] = "seeded test picture"  # ImageDescription
    buf = io.BytesIO()
    Image.fromarray(picture(), "RGB").save(buf, "JPEG", quality=90, subsampling=0, optimize=False, progressive=False, restart_marker_blocks=7,
                                           exif=exif.tobytes(), icc_profile=b"\0" * 128, comment=b"pyrite_amd test fixture")
    with open(OUT, "wb") as f:
        f.write(buf.getvalue())
    print(OUT, len(buf.getvalue()), "bytes")


if __name__ == "__main__":
    main()
