"""Writes tests/golden/png_encode.npz: what the PNG encoder's tests hold the code to, recorded (tests/png_encode_ref.py has the
inputs).  Imports PIL, numpy and the repository's build settings (for the compiler's path); needs no GPU.

    python tests/golden/make_golden_png_encode.py

Contents.
  `names`: the inputs of png_encode_ref.recorded_inputs() -- the corpus of the deflate core, then the filtered rows of the GPU test's
  images and of the size fixtures.  For input i: `lengths[i]` and `sha256[i]` of the zlib stream that tests/png_deflate_host.cpp (the
  core with one lane, built with the sanitizers) makes of it, and the stream itself, blob[offsets[i]:offsets[i + 1]], when it has at
  most png_encode_ref.WHOLE bytes (otherwise the slice is empty).
  `filter_names` / `filter_sha256`: the images of png_encode_ref.filter_cases() and the SHA-256 of what Pillow's own file for each
  inflates to -- Pillow's filtered rows, for machines that do not have Pillow.
  `size_names` / `size_ours` / `size_pillow`: the size fixtures, the bytes of the file around the recorded stream and of Pillow's file.
  `pillow`: the version that wrote the files.
Also writes the size table to profiles/png_encode_sizes.txt."""
import hashlib
import os
import sys
import tempfile

import numpy as np
import PIL

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]
import png_encode_ref as E  # noqa: E402


def main():
    inputs = E.recorded_inputs()
    with tempfile.TemporaryDirectory() as tmp:
        streams, said = E.host_streams(list(inputs.values()), tmp)
    print(said)
    records = [E.record(z) for z in streams]
    whole = [r[2] for r in records]
    cases = E.filter_cases()
    for name, a in cases.items():
        assert E.filter_rows(a) == E.pillow_rows(a), name
    fixtures = E.size_fixtures()
    ours = [len(E.png_file(a, streams[list(inputs).index("rows_" + name)])) for name, a in fixtures.items()]
    pillow = [len(E.pillow_file(a)) for a in fixtures.values()]
    np.savez_compressed(
        os.path.join(HERE, "png_encode.npz"), names=np.array(list(inputs)), lengths=np.array([r[0] for r in records], np.int64),
        sha256=np.array([r[1] for r in records]), blob=np.frombuffer(b"".join(whole), np.uint8),
        offsets=np.cumsum([0] + [len(w) for w in whole]).astype(np.int64), filter_names=np.array(list(cases)),
        filter_sha256=np.array([hashlib.sha256(E.pillow_rows(a)).hexdigest() for a in cases.values()]), size_names=np.array(list(fixtures)),
        size_ours=np.array(ours, np.int64), size_pillow=np.array(pillow, np.int64), pillow=np.array(PIL.__version__))
    lines = [f"{name:10s} ours {o:8d}  Pillow {p:8d}  ratio {o / p:.4f}" for name, o, p in zip(fixtures, ours, pillow)]
    head = (f"# File sizes of the PNG encoder's size fixtures (tests/png_encode_ref.py: size_fixtures), bytes: the file around the stream of the\n"
            f"# deflate core's host build against Pillow {PIL.__version__}'s file for the same pixels.  Written by tests/golden/make_golden_png_encode.py;\n"
            f"# tests/test_png_encode_host.py holds every ratio but the noise's at its value here plus 0.02.\n")
    with open(os.path.join(os.path.dirname(os.path.dirname(HERE)), "profiles", "png_encode_sizes.txt"), "w") as f:
        f.write(head + "\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
