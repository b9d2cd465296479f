"""Writes tests/golden/png.npz: a few PNG files that Pillow itself wrote, with what Pillow decodes them to, recorded, so that the
restatement of the decoder (tests/png_ref.py) and the kernels behind it are held against Pillow itself on machines that do not have it.
Imports PIL and numpy only.

    python tests/golden/make_golden_png.py

Contents.  `keys`: the names of the files; file i is blob[offsets[i]:offsets[i + 1]].  For key k: `rgb_k` = np.asarray(
Image.open(f).convert("RGB")) and `raw_k` = np.asarray(Image.open(f)): modes L, P (8-bit, and 4-bit as Pillow writes a 16-colour
palette), RGB, RGBA, LA, one P file with tRNS, one written with optimize=True, compress_level 1 and 9.  `refused_keys` / `refused_blob`
/ `refused_offsets`: one interlaced, one 16-bit and one 1-bit grey file, which image_io.png_parse must refuse.  `pillow`: the version
that wrote the file."""
import io
import os
import struct
import zlib

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
H, W = 37, 45


def save(image, **arguments):
    buf = io.BytesIO()
    image.save(buf, format="PNG", **arguments)
    return buf.getvalue()


def blob(files):
    return np.frombuffer(b"".join(files), np.uint8), np.cumsum([0] + [len(f) for f in files]).astype(np.int64)


def picture(rng, channels):
    """Smooth gradients with noise on top and a few flat patches: every filter gets chosen somewhere."""
    y, x = np.mgrid[0:H, 0:W]
    planes = [(3 * x + 5 * y + 40 * c + rng.integers(0, 12, (H, W))) % 256 for c in range(channels)]
    out = np.stack(planes, axis=2).astype(np.uint8)
    out[5:15, 8:30] = 200
    return out[:, :, 0] if channels == 1 else out


def interlace(data):
    """The same file with the interlace byte of IHDR set (its CRC redone): png_parse must refuse it before it looks at the data."""
    body = bytearray(data[16:29])
    body[12] = 1
    return data[:16] + bytes(body) + struct.pack(">I", zlib.crc32(b"IHDR" + bytes(body))) + data[33:]


def main():
    rng = np.random.default_rng(0)
    labels = (rng.integers(0, 19, (H // 6 + 1, W // 6 + 1), dtype=np.uint8).repeat(6, 0).repeat(6, 1))[:H, :W]
    palette = rng.integers(0, 256, 19 * 3, dtype=np.uint8).tolist()
    p8 = Image.fromarray(labels, "P")
    p8.putpalette(palette)
    p4 = Image.fromarray(labels % 13, "P")
    p4.putpalette(palette[:13 * 3])
    images = {
        "L": (Image.fromarray(labels, "L"), {}),
        "P8": (p8, {"bits": 8}),
        "P4": (p4, {"bits": 4}),
        "P_trns": (p8, {"bits": 8, "transparency": 3}),
        "RGB": (Image.fromarray(picture(rng, 3), "RGB"), {}),
        "RGBA": (Image.fromarray(picture(rng, 4), "RGBA"), {}),
        "LA": (Image.fromarray(picture(rng, 2), "LA"), {}),
        "RGB_optimize": (Image.fromarray(picture(rng, 3), "RGB"), {"optimize": True}),
        "RGB_level1": (Image.fromarray(picture(rng, 3), "RGB"), {"compress_level": 1}),
        "L_level9": (Image.fromarray(picture(rng, 1), "L"), {"compress_level": 9}),
    }
    out, files = {}, []
    for key, (image, arguments) in images.items():
        data = save(image, **arguments)
        files.append(data)
        out["rgb_" + key] = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        out["raw_" + key] = np.asarray(Image.open(io.BytesIO(data)))
    refused = {"interlaced": interlace(save(images["RGB"][0])), "16bit": save(Image.fromarray(picture(rng, 1).astype(np.uint16) * 257)),
               "1bit_grey": save(Image.fromarray(labels > 9).convert("1"))}
    out["blob"], out["offsets"] = blob(files)
    out["refused_blob"], out["refused_offsets"] = blob(list(refused.values()))
    path = os.path.join(HERE, "png.npz")
    np.savez_compressed(path, keys=np.array(list(images)), refused_keys=np.array(list(refused)), pillow=np.array(PIL.__version__), **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, files of {[len(f) for f in files]} bytes")
    assert os.path.getsize(path) <= 100 * 1000


if __name__ == "__main__":
    main()
