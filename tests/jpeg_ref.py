"""Numpy restatement of the baseline JPEG that Pillow's default `save(format="JPEG")` writes for an RGB image (libjpeg: quality 75,
4:2:0, the Annex K Huffman tables, no optimisation), stage by stage: `tables`, `header`, `coefficients`, `segment`, `encode`.  Own
code, integers from end to end; tests/test_jpeg_host.py holds it against Pillow and against the recorded Pillow bytes of
tests/golden/jpeg_pillow.npz, tests/test_gpu_jpeg.py holds the kernels of csrc/jpeg.hip against it.  Also the shapes and the content
patterns those tests share."""
import numpy as np

# ---- Annex K ----
LUMA_Q = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
          18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
CHROMA_Q = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
DC_LUMA_BITS = (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0)
DC_CHROMA_BITS = (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0)
DC_VALS = tuple(range(12))
AC_LUMA_BITS = (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D)
AC_LUMA_VALS = (
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08,
    0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6,
    0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
    0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA)
AC_CHROMA_BITS = (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77)
AC_CHROMA_VALS = (
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26,
    0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
    0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
    0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA)
HUFFMAN = ((0x00, DC_LUMA_BITS, DC_VALS), (0x10, AC_LUMA_BITS, AC_LUMA_VALS), (0x01, DC_CHROMA_BITS, DC_VALS), (0x11, AC_CHROMA_BITS, AC_CHROMA_VALS))


def _zigzag():
    """ZIGZAG[k] = the natural (row-major) index of the k-th coefficient of the zigzag scan."""
    order = sorted(range(64), key=lambda i: (i // 8 + i % 8, (i // 8) if (i // 8 + i % 8) % 2 else (i % 8)))
    return np.array(order, np.int64)


ZIGZAG = _zigzag()

# ---- the cases the tests share ----
# (H, W) and what each breaks (tests/test_gpu_jpeg.py repeats the table)
SIZES = ((1, 1), (8, 8), (16, 16), (17, 23), (70, 38), (33, 16), (40, 10), (10, 40), (130, 262), (2054, 30))
BATCH_SIZE = (3, 40, 56)        # a batch of three 40 x 56 images
SCAN_SIZE = (264, 520)          # 17 x 33 MCUs = 3366 blocks: past three 1024-block tiles of the prefix sum
QUALITY_SIZE = (48, 40)         # the one shape the other qualities run on
QUALITIES = (1, 30, 95, 100)
PATTERNS = ("random", "ramp", "constant", "checker", "colour_checker", "mixed")
CHECKER_QUALITY = 100           # the checkerboards run at this quality: the largest magnitudes and the longest blocks


def pattern(name, h, w, seed=0):
    """uint8 [h, w, 3].  random: dense blocks, long codes.  ramp: early end-of-block, runs of 16 zeros.  constant: every block only
    an end-of-block.  checker / colour_checker (0/255 per pixel; per channel out of phase): the largest magnitudes, the longest blocks,
    the most 0xFF bytes.  mixed: a ramp with a few random 8 x 8 blocks: long and short blocks under one prefix sum."""
    rng = np.random.RandomState(4000 + seed)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    if name == "random":
        x = rng.randint(0, 256, size=(h, w, 3))
    elif name in ("ramp", "mixed"):
        x = np.stack([(yy * 3 + xx) % 256, (yy + xx * 2) // 3 % 256, 255 - (yy + xx) // 2 % 256], -1)
        if name == "mixed":
            for _ in range(max(1, (h // 8) * (w // 8) // 7)):
                y0, x0 = rng.randint(0, max(1, h - 7)), rng.randint(0, max(1, w - 7))
                x[y0:y0 + 8, x0:x0 + 8] = rng.randint(0, 256, size=x[y0:y0 + 8, x0:x0 + 8].shape)
    elif name == "constant":
        x = np.zeros((h, w, 3), np.int64) + np.array([200, 30, 90])
    elif name == "checker":
        x = np.repeat((((yy + xx) & 1) * 255)[..., None], 3, -1)
    elif name == "colour_checker":
        x = np.stack([((yy + xx) & 1) * 255, ((yy + xx + 1) & 1) * 255, (yy & 1) * 255], -1)
    else:
        raise ValueError(name)
    return np.ascontiguousarray(x.astype(np.uint8))


ALL_SIZES = SIZES + (BATCH_SIZE[1:], SCAN_SIZE, QUALITY_SIZE)
RECORDED_PIXELS = 40 * 56  # tests/golden/jpeg_pillow.npz holds Pillow's whole file up to this size, and its SHA-256 for every case


def cases():
    """Every (h, w, pattern, quality, seed) the host and GPU tests run: each size with each content at quality 75, the checkerboards
    also at 100, and every content at the other qualities on QUALITY_SIZE."""
    out = []
    for seed, (h, w) in enumerate(ALL_SIZES):
        out += [(h, w, name, 75, seed) for name in PATTERNS]
        out += [(h, w, name, CHECKER_QUALITY, seed) for name in ("checker", "colour_checker")]
        if (h, w) == QUALITY_SIZE:
            out += [(h, w, name, q, seed) for name in PATTERNS for q in QUALITIES if (q, name) not in ((100, "checker"), (100, "colour_checker"))]
    return out


def case_key(h, w, name, quality, seed):
    return f"{h}x{w}_{name}_q{quality}"


def photo(h, w, seed=0):
    """Smooth plus noise, the statistics of a generated face more than of any pattern above: uint8 [h, w, 3]."""
    rng = np.random.RandomState(5000 + seed)
    yy, xx = np.meshgrid(np.arange(h) / h, np.arange(w) / w, indexing="ij")
    base = np.stack([128 + 100 * np.sin(6.0 * xx + 2.0 * yy), 128 + 100 * np.cos(5.0 * yy - xx), 128 + 90 * np.sin(9.0 * xx * yy)], -1)
    return np.clip(base + rng.normal(0, 6, size=base.shape), 0, 255).astype(np.uint8)


# ---- stage by stage ----

def tables(quality=75):
    """(luminance, chrominance) int64 [64] in natural order: libjpeg's jpeg_set_quality with baseline forced."""
    q = int(quality)
    assert 1 <= q <= 100
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((np.array(t, np.int64) * scale + 50) // 100, 1, 255) for t in (LUMA_Q, CHROMA_Q))


def _seg(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def header(h, w, quality=75):
    """SOI .. SOS, the bytes before the entropy-coded segment."""
    ql, qc = tables(quality)
    out = b"\xff\xd8" + _seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    out += _seg(0xDB, bytes([0]) + bytes(ql[ZIGZAG].tolist())) + _seg(0xDB, bytes([1]) + bytes(qc[ZIGZAG].tolist()))
    out += _seg(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, bits, vals in HUFFMAN:
        out += _seg(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    return out + _seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def geometry(h, w):
    """(MCUs across, MCUs down, blocks per image)."""
    mx, my = -(-w // 16), -(-h // 16)
    return mx, my, 6 * mx * my


def _fix(x):
    return int(x * 65536 + 0.5)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """One pass of jfdctint over the last axis of int64 [..., 8]."""
    c = {"0.298631336": 2446, "0.390180644": 3196, "0.541196100": 4433, "0.765366865": 6270, "0.899976223": 7373, "1.175875602": 9633,
         "1.501321110": 12299, "1.847759065": 15137, "1.961570560": 16069, "2.053119869": 16819, "2.562915447": 20995, "3.072711026": 25172}
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    out = [None] * 8
    n = 11 if first else 15
    if first:
        out[0], out[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        out[0], out[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * c["0.541196100"]
    out[2] = _descale(z1 + t13 * c["0.765366865"], n)
    out[6] = _descale(z1 - t12 * c["1.847759065"], n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * c["1.175875602"]
    t4, t5, t6, t7 = t4 * c["0.298631336"], t5 * c["2.053119869"], t6 * c["3.072711026"], t7 * c["1.501321110"]
    z1, z2 = -z1 * c["0.899976223"], -z2 * c["2.562915447"]
    z3, z4 = -z3 * c["1.961570560"] + z5, -z4 * c["0.390180644"] + z5
    out[7], out[5], out[3], out[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(out, -1)


def _blocks(plane, q):
    """int64 [8r, 8c] samples -> quantised coefficients int64 [r, c, 64] in zigzag order."""
    r, c = plane.shape[0] // 8, plane.shape[1] // 8
    b = plane.reshape(r, 8, c, 8).transpose(0, 2, 1, 3) - 128
    b = _fdct_pass(b, True)                                        # rows
    b = _fdct_pass(b.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)  # columns
    b = b.reshape(r, c, 64)
    d = 8 * q
    return (np.sign(b) * ((np.abs(b) + d // 2) // d))[..., ZIGZAG]


def planes(x):
    """uint8 [H,W,3] -> (Y [8 ceil(H/8), 8 ceil(W/8)], Cb, Cr [8 ch, 8 cw]) int64: colour conversion, edge repetition, down-sampling."""
    h, w, _ = x.shape
    r, g, b = (x[..., i].astype(np.int64) for i in range(3))
    y = (_fix(.299) * r + _fix(.587) * g + _fix(.114) * b + 32768) >> 16
    cb = (-_fix(.16874) * r - _fix(.33126) * g + _fix(.5) * b + (128 << 16) + 32767) >> 16
    cr = (_fix(.5) * r - _fix(.41869) * g - _fix(.08131) * b + (128 << 16) + 32767) >> 16
    y = np.pad(y, ((0, -h % 8), (0, -w % 8)), mode="edge")
    cw, ch = -(-(-(-w // 2)) // 8), -(-(-(-h // 2)) // 8)
    out = [y]
    for c in (cb, cr):
        c = np.pad(c, ((0, h % 2), (0, 16 * cw - w)), mode="edge")
        bias = np.tile(np.array([1, 2], np.int64), 8 * cw // 2)[None, :]
        d = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
        out.append(np.pad(d, ((0, 8 * ch - d.shape[0]), (0, 0)), mode="edge"))
    return tuple(out)


def coefficients(x, quality=75):
    """uint8 [H,W,3] -> int16 [blocks, 64], zigzag order, blocks in scan order (per MCU: Y00 Y01 Y10 Y11 Cb Cr), dummies included:
    all AC zero, DC that of the previous block of the component."""
    h, w, _ = x.shape
    mx, my, nblocks = geometry(h, w)
    ql, qc = tables(quality)
    y, cb, cr = planes(x)
    yb, cbb, crb = _blocks(y, ql), _blocks(cb, qc), _blocks(cr, qc)
    out = np.zeros((my, mx, 6, 64), np.int64)
    for j in range(4):
        by, bx = j // 2, j % 2
        real = yb[by::2, bx::2]
        out[:real.shape[0], :real.shape[1], j] = real
    out[:, :, 4], out[:, :, 5] = cbb, crb
    rows, cols = yb.shape[0], yb.shape[1]
    for m_y in range(my):       # the dummies: DC of the previous Y block in scan order (always inside the MCU: Y00 is never a dummy)
        for m_x in range(mx):
            for j in range(1, 4):
                if 2 * m_y + j // 2 >= rows or 2 * m_x + j % 2 >= cols:
                    out[m_y, m_x, j] = 0
                    out[m_y, m_x, j, 0] = out[m_y, m_x, j - 1, 0]
    return out.reshape(nblocks, 64).astype(np.int16)


def huffman_codes(bits, vals):
    """Annex C: {symbol: (code, length)}."""
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return codes


def _code_arrays(bits, vals):
    code, length = np.zeros(256, np.int64), np.zeros(256, np.int64)
    for s, (c, n) in huffman_codes(bits, vals).items():
        code[s], length[s] = c, n
    return code, length


def _bitlen(a):
    n = np.zeros(a.shape, np.int64)
    for k in range(12):
        n += (a >> k) > 0
    return n


def segment(coef):
    """int16 [blocks, 64] -> the entropy-coded segment BEFORE byte stuffing, filled with 1-bits to a byte.  Every token (code or value
    bits) of the scan is computed as arrays, then laid down bit by bit with one cumulative sum (so 1024^2 takes a second or two)."""
    c = coef.astype(np.int64)
    nb = c.shape[0]
    comp = np.maximum(np.arange(nb) % 6 - 3, 0)  # 0 Y, 1 Cb, 2 Cr
    chroma = (comp > 0).astype(np.int64)
    dc = c[:, 0]
    diff = np.zeros(nb, np.int64)
    for k in range(3):
        idx = np.nonzero(comp == k)[0]
        diff[idx] = np.diff(dc[idx], prepend=0)
    tabs = [_code_arrays(b, v) for _, b, v in HUFFMAN]  # DC0 AC0 DC1 AC1
    dc_code = np.stack([tabs[0][0], tabs[2][0]])
    dc_len = np.stack([tabs[0][1], tabs[2][1]])
    ac_code = np.stack([tabs[1][0], tabs[3][0]])
    ac_len = np.stack([tabs[1][1], tabs[3][1]])

    def value_bits(v, n):
        return np.where(v < 0, v + (1 << n) - 1, v)

    # tokens as (block, position within the block's token list, bits, length); position keys keep the scan order under one sort
    n = _bitlen(np.abs(diff))
    tok = [(np.arange(nb), np.zeros(nb, np.int64), dc_code[chroma, n], dc_len[chroma, n]), (np.arange(nb), np.ones(nb, np.int64), value_bits(diff, n), n)]
    blk, k = np.nonzero(c[:, 1:])
    k = k + 1
    v = c[blk, k]
    first = np.ones(len(blk), bool)
    first[1:] = blk[1:] != blk[:-1]
    prev = np.where(first, 0, np.concatenate([[0], k[:-1]]))
    run = k - prev - 1
    size = _bitlen(np.abs(v))
    ch = chroma[blk]
    for z in range(1, 4):  # up to three 0xF0 before a coefficient
        m = run >= 16 * z
        tok.append((blk[m], 8 * k[m] + z, ac_code[ch[m], 0xF0], ac_len[ch[m], 0xF0]))
    sym = ((run & 15) << 4) | size
    tok.append((blk, 8 * k + 4, ac_code[ch, sym], ac_len[ch, sym]))
    tok.append((blk, 8 * k + 5, value_bits(v, size), size))
    eob = np.nonzero(c[:, 63] == 0)[0]
    tok.append((eob, np.full(len(eob), 8 * 64, np.int64), ac_code[chroma[eob], 0], ac_len[chroma[eob], 0]))
    tb, tp, tv, tl = (np.concatenate([t[i] for t in tok]) for i in range(4))
    order = np.lexsort((tp, tb))
    tv, tl = tv[order], tl[order]
    keep = tl > 0
    tv, tl = tv[keep], tl[keep]
    total = int(tl.sum())
    start = np.cumsum(tl) - tl
    which = np.repeat(np.arange(len(tl)), tl)
    within = np.arange(total) - start[which]
    bits = ((tv[which] >> (tl[which] - 1 - within)) & 1).astype(np.uint8)
    bits = np.concatenate([bits, np.ones(-total % 8, np.uint8)])
    return np.packbits(bits).tobytes()


def encode(x, quality=75):
    """uint8 [H,W,3] -> the file Pillow writes for Image.fromarray(x).save(fp, format="JPEG", quality=quality)."""
    h, w, _ = x.shape
    return header(h, w, quality) + segment(coefficients(x, quality)).replace(b"\xff", b"\xff\x00") + b"\xff\xd9"
