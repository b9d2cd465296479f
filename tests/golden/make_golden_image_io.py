"""Writes tests/golden/image_io.npz: what Pillow's Image.resize returns, recorded, so that the numpy restatement of its arithmetic
(tests/imageio_ref.py) is held against Pillow itself on machines that do not have it.  Imports only PIL and numpy.

    python tests/golden/make_golden_image_io.py

Contents.  For every small case of SHAPES (inputs up to 100 x 75; the same list as tests/imageio_ref.py SMALL_SHAPES) and seeded
random bytes: `bil_<i>` / `nea_<i>`, uint8 [B,out_h,out_w,C], the BILINEAR / NEAREST resize of each image of the batch (mode L for
C = 1, RGB for C = 3), and `sum_<i>`, the sum of the input bytes (the input itself is not stored: random bytes do not compress, and
RandomState's stream is frozen; the sum tells a test that it regenerated the same input).  For the label case: `label_grid`, the
16 x 16 grid of ids 0..18 whose 32 x 32 blocks make the 512 x 512 label, and `label_bil` / `label_nea`, its resize to 64 x 64.
`pillow`: the version that wrote the file.  Under 64 KB."""
import os

import numpy as np
import PIL
from PIL import Image

SMALL_SHAPES = (
    (1, 3, 5, 5, 1, 1),
    (2, 1, 2, 3, 5, 4),
    (1, 3, 9, 7, 16, 16),
    (2, 3, 37, 53, 16, 16),
    (1, 3, 16, 16, 16, 8),
    (1, 1, 16, 24, 4, 24),
    (1, 3, 64, 64, 64, 64),
    (1, 1, 100, 75, 32, 33),
)
FILTERS = {"bil": getattr(Image, "Resampling", Image).BILINEAR, "nea": getattr(Image, "Resampling", Image).NEAREST}


def pil_resize(batch, out_h, out_w, resample):
    """uint8 [B,H,W,C] -> [B,out_h,out_w,C], each image through Image.resize."""
    out = []
    for img in batch:
        pil = Image.fromarray(img[..., 0], "L") if img.shape[2] == 1 else Image.fromarray(img, "RGB")
        r = np.asarray(pil.resize((out_w, out_h), resample))
        out.append(r[..., None] if r.ndim == 2 else r)
    return np.stack(out)


def main():
    data = {"pillow": np.array(PIL.__version__)}
    for i, (b, c, h, w, oh, ow) in enumerate(SMALL_SHAPES):
        x = np.random.RandomState(1000 + i).randint(0, 256, size=(b, h, w, c)).astype(np.uint8)
        data[f"sum_{i}"] = np.array(int(x.sum()), np.int64)
        for name, resample in FILTERS.items():
            data[f"{name}_{i}"] = pil_resize(x, oh, ow, resample)
    grid = np.random.RandomState(7).randint(0, 19, size=(16, 16)).astype(np.uint8)
    label = np.kron(grid, np.ones((32, 32), np.uint8))[None, :, :, None]
    data["label_grid"] = grid
    for name, resample in FILTERS.items():
        data[f"label_{name}"] = pil_resize(label, 64, 64, resample)[0, :, :, 0]
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "image_io.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 64 * 1024


if __name__ == "__main__":
    main()
