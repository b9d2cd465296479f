"""Writes tests/golden/jpeg_decode.npz: what Pillow's `Image.open(fp).convert("RGB")` returns for the cases of tests/jpeg_decode_ref.py,
recorded, so that the numpy restatement of the decoder and the kernels behind it are held against Pillow itself on machines that do
not have it.  Imports PIL, numpy, tests/jpeg_ref.py and tests/jpeg_decode_ref.py (for the case lists, the patterns and jpeg_ref's
ENCODER, whose files equal Pillow's byte for byte; nothing of the decoder restatement's arithmetic goes into the file).

    python tests/golden/make_golden_jpeg_decode.py

Contents.  `enc_keys` / `enc_sha256`: for every file that jpeg_ref.encode writes (encode_cases(): 4:2:0, the Annex K tables), the
SHA-256 of the uint8 [h, w, 3] pixels Pillow decodes it to.  `pil_keys` / `pil_sha256` / `pil_blob` / `pil_offsets`: the files Pillow
itself wrote for pillow_cases() (4:4:4, grey, optimised Huffman tables, qualities 95 and 100; sizes up to 40 x 56), whole -- file i is
pil_blob[pil_offsets[i]:pil_offsets[i + 1]] -- and the digest of their pixels.  `refused_keys` / `refused_blob` / `refused_offsets`:
one file of each kind that image_io.jpeg_parse must refuse (progressive, 4:2:2, CMYK, PNG).  `pillow`: the version that wrote the file."""
import hashlib
import io
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_decode_ref as D  # noqa: E402
import jpeg_ref as R  # noqa: E402


def pillow_pixels(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def digest(x):
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()


def save(image, **arguments):
    buf = io.BytesIO()
    image.save(buf, **arguments)
    return buf.getvalue()


def blob(files):
    return np.frombuffer(b"".join(files), np.uint8), np.cumsum([0] + [len(f) for f in files]).astype(np.int64)


def main():
    enc_keys, enc_sha = [], []
    for key, h, w, make in D.encode_cases():
        x = pillow_pixels(make())
        assert x.shape == (h, w, 3)
        enc_keys.append(key), enc_sha.append(digest(x))
    pil_keys, pil_sha, files = [], [], []
    for key, h, w, (variant, mode, arguments), name, seed in D.pillow_cases():
        data = save(Image.fromarray(D.pillow_input(mode, name, h, w, seed)), format="JPEG", **arguments)
        assert Image.open(io.BytesIO(data)).mode == mode
        pil_keys.append(key), pil_sha.append(digest(pillow_pixels(data))), files.append(data)
    image = Image.fromarray(R.pattern("mixed", 40, 56, 1))
    refused = {"progressive": save(image, format="JPEG", progressive=True), "422": save(image, format="JPEG", subsampling=1),
               "cmyk": save(image.convert("CMYK"), format="JPEG"), "png": save(image, format="PNG")}
    assert tuple(refused) == D.REFUSED
    pil_blob, pil_offsets = blob(files)
    refused_blob, refused_offsets = blob(list(refused.values()))
    data = {"pillow": np.array(PIL.__version__), "enc_keys": np.array(enc_keys), "enc_sha256": np.array(enc_sha), "pil_keys": np.array(pil_keys),
            "pil_sha256": np.array(pil_sha), "pil_blob": pil_blob, "pil_offsets": pil_offsets, "refused_keys": np.array(list(refused)),
            "refused_blob": refused_blob, "refused_offsets": refused_offsets}
    path = os.path.join(HERE, "jpeg_decode.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes,", len(enc_keys), "encoder cases,", len(files), "Pillow files")
    assert os.path.getsize(path) < 400 * 1024


if __name__ == "__main__":
    main()
