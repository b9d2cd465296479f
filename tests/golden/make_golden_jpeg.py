"""Writes tests/golden/jpeg_pillow.npz: what Pillow's `Image.fromarray(x).save(buf, format="JPEG", quality=q)` returns for the cases
of tests/jpeg_ref.py (cases(): every size with every content pattern), recorded, so that the numpy restatement of the encoder and the
kernels behind it are held against Pillow itself on machines that do not have it.  Imports PIL, numpy and tests/jpeg_ref.py (for the
patterns only; nothing of the restatement's arithmetic goes into the file).

    python tests/golden/make_golden_jpeg.py

Contents.  `keys`: one name per case, "<h>x<w>_<pattern>_q<quality>".  `sha256`: the digest of Pillow's file for EVERY case, in the
order of `keys`.  `blob` / `offsets`: the whole files of the cases of at most 40 x 56 pixels, one after the other (file i of
`recorded` is blob[offsets[i]:offsets[i + 1]]; stored as one array so that the 623-byte header they share compresses away).
`sum`: the sum of each case's input bytes (the inputs are not stored: RandomState's stream is frozen, the sum tells a test that it
regenerated the same input).  `pillow`: the version that wrote the file.  Under 64 KB."""
import hashlib
import io
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_ref as R  # noqa: E402


def pillow_jpeg(x, quality):
    buf = io.BytesIO()
    Image.fromarray(x).save(buf, format="JPEG", quality=quality)
    return buf.getvalue()


def pillow_jpeg_default(x):
    """What the reference's save_image ends in: no quality named."""
    buf = io.BytesIO()
    Image.fromarray(x).save(buf, format="JPEG")
    return buf.getvalue()


def main():
    keys, digests, sums, recorded, files = [], [], [], [], []
    for case in R.cases():
        h, w, name, quality, seed = case
        x = R.pattern(name, h, w, seed)
        data = pillow_jpeg(x, quality)
        assert quality != 75 or data == pillow_jpeg_default(x)
        keys.append(R.case_key(*case)), digests.append(hashlib.sha256(data).hexdigest()), sums.append(int(x.sum()))
        if h * w <= R.RECORDED_PIXELS:
            recorded.append(R.case_key(*case)), files.append(data)
    offsets = np.cumsum([0] + [len(f) for f in files]).astype(np.int64)
    data = {"pillow": np.array(PIL.__version__), "keys": np.array(keys), "sha256": np.array(digests), "sum": np.array(sums, np.int64),
            "recorded": np.array(recorded), "offsets": offsets, "blob": np.frombuffer(b"".join(files), np.uint8)}
    path = os.path.join(HERE, "jpeg_pillow.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes,", len(keys), "cases,", len(files), "whole files")
    assert os.path.getsize(path) < 64 * 1024


if __name__ == "__main__":
    main()
