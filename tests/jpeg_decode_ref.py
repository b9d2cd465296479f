"""Numpy restatement of the baseline JPEG decoder that `PIL.Image.open(fp).convert("RGB")` runs (libjpeg: Huffman decoding, the accurate
integer inverse DCT, fancy chroma up-sampling, 16.16 fixed-point colour conversion), for the files in scope of
where2edit_amd.image_io.from_jpeg: SOF0, 8 bits, one scan, no restart interval, 4:2:0 / 4:4:4 / grey.  Own code, integers from end to
end.  Four parts: `parse`, the sequential Huffman decoder as the total function `f` over decoder states, the relaxation that the
kernels of csrc/jpeg_decode.hip run (`relax`: one level; `relax_two_level`: workgroups of 256 subsequences, one launch after the
other), and the pixel rules (`pixels`).  tests/test_jpeg_decode_host.py holds it against Pillow and against the recorded hashes of
tests/golden/jpeg_decode.npz; tests/test_gpu_jpeg_decode.py holds the kernels against it.  Also the case list those tests share."""
import functools

import numpy as np

import jpeg_ref as R

BLOCKS_PER_MCU = {"420": 6, "444": 3, "grey": 1}
SLOT_COMPONENT = {"420": (0, 0, 0, 0, 1, 2), "444": (0, 1, 2), "grey": (0,)}
GROUP = 256                      # subsequences of one workgroup of the relaxation
SUB_BITS = (32, 128, 1024)       # the subsequence lengths the GPU tests run
STATUS_COUNT, STATUS_CATEGORY, STATUS_INSIDE = 1, 2, 4

# ---- the cases the tests share ----
PHOTO_SIZE = (256, 256)
PHOTO_QUALITIES = (75, 95)
# Pillow-made files, recorded whole in the fixture: (name, mode, the arguments of save()).  4:4:4, grey, optimised Huffman tables
# (the file's own DHT lists), the high qualities.
PILLOW_VARIANTS = (("444", "RGB", {"quality": 75, "subsampling": 0}), ("grey", "L", {"quality": 75}),
                   ("420opt", "RGB", {"quality": 75, "optimize": True}), ("444opt95", "RGB", {"quality": 95, "subsampling": 0, "optimize": True}),
                   ("grey100", "L", {"quality": 100}), ("420opt100", "RGB", {"quality": 100, "optimize": True}))
PILLOW_PATTERNS = ("mixed", "random", "constant", "colour_checker")
PILLOW_SIZES = tuple(s for s in R.ALL_SIZES if s[0] * s[1] <= R.RECORDED_PIXELS)
REFUSED = ("progressive", "422", "cmyk", "png")  # recorded Pillow files that jpeg_parse must refuse


def encode_cases():
    """(key, h, w, make) for every file that tests/jpeg_ref.py's encoder writes (4:2:0, the Annex K tables): jpeg_ref.cases() and the
    photograph at two qualities.  make() returns the file's bytes."""
    out = []
    for case in R.cases():
        h, w, name, quality, seed = case
        out.append(("enc_" + R.case_key(*case), h, w, functools.partial(_encode_pattern, case)))
    for q in PHOTO_QUALITIES:
        out.append((f"enc_photo{PHOTO_SIZE[0]}_q{q}", PHOTO_SIZE[0], PHOTO_SIZE[1], functools.partial(_encode_photo, q)))
    return out


@functools.lru_cache(maxsize=None)
def _encode_pattern(case):
    h, w, name, quality, seed = case
    return R.encode(R.pattern(name, h, w, seed), quality)


@functools.lru_cache(maxsize=None)
def _encode_photo(quality):
    return R.encode(R.photo(*PHOTO_SIZE), quality)


def pillow_cases():
    """(key, h, w, variant, pattern, seed) of the Pillow-made files of the fixture."""
    out = []
    for seed, (h, w) in enumerate(R.ALL_SIZES):
        if (h, w) in PILLOW_SIZES:
            out += [(f"pil_{v[0]}_{h}x{w}_{name}", h, w, v, name, seed) for v in PILLOW_VARIANTS for name in PILLOW_PATTERNS]
    return out


def pillow_input(mode, name, h, w, seed):
    x = R.pattern(name, h, w, seed)
    return np.ascontiguousarray(x[..., 1]) if mode == "L" else x


# ---- the parser ----

def parse(data):
    """The file -> dict(h, w, sampling, q: int64 [components, 64] natural order, dht: per component ((counts, symbols) DC, (counts,
    symbols) AC), scan: the entropy-coded segment with the byte stuffing removed).  Only files in scope; anything else is an
    AssertionError here (image_io.jpeg_parse is the one that words the refusals)."""
    assert data[:2] == b"\xff\xd8"
    at, q, huff, frame = 2, {}, {}, None
    while True:
        assert data[at] == 0xFF
        marker = data[at + 1]
        size = int.from_bytes(data[at + 2:at + 4], "big")
        body = data[at + 4:at + 2 + size]
        at += 2 + size
        if marker == 0xDB:
            while body:
                assert body[0] >> 4 == 0
                t = np.zeros(64, np.int64)
                t[R.ZIGZAG] = np.frombuffer(body[1:65], np.uint8)
                q[body[0] & 15] = t
                body = body[65:]
        elif marker == 0xC4:
            while body:
                counts = tuple(body[1:17])
                huff[body[0]] = (counts, bytes(body[17:17 + sum(counts)]))
                body = body[17 + sum(counts):]
        elif marker == 0xC0:
            assert body[0] == 8
            h, w, n = int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big"), body[5]
            frame = [(body[6 + 3 * i], body[7 + 3 * i], body[8 + 3 * i]) for i in range(n)]
        elif marker == 0xDA:
            assert body[0] == len(frame) and tuple(body[-3:]) == (0, 63, 0)
            sel = [body[2 + 2 * i] for i in range(len(frame))]
            break
        else:
            assert 0xE0 <= marker <= 0xFE, hex(marker)
    factors = tuple(f[1] for f in frame)
    sampling = "grey" if len(frame) == 1 else {(0x22, 0x11, 0x11): "420", (0x11, 0x11, 0x11): "444"}[factors]
    end = at
    while not (data[end] == 0xFF and data[end + 1] != 0):
        end += 1
    assert data[end + 1] == 0xD9
    return {"h": h, "w": w, "sampling": sampling, "q": np.stack([q[f[2]] for f in frame]),
            "dht": tuple((huff[s >> 4], huff[0x10 | (s & 15)]) for s in sel), "scan": data[at:end].replace(b"\xff\x00", b"\xff")}


def geometry(h, w, sampling):
    """(MCUs across, MCUs down, blocks per image)."""
    m = 16 if sampling == "420" else 8
    mx, my = -(-w // m), -(-h // m)
    return mx, my, BLOCKS_PER_MCU[sampling] * mx * my


# ---- the Huffman decoder as a function of states ----

@functools.lru_cache(maxsize=None)
def _lookup(counts, symbols):
    """The table as a list over the next 16 bits: (length << 8) | symbol, 0 where the bits begin no code."""
    lut = np.zeros(1 << 16, np.int64)
    for s, (code, length) in R.huffman_codes(counts, symbols).items():
        lut[code << (16 - length):(code + 1) << (16 - length)] = (length << 8) | s
    return lut.tolist()


class Stream:
    """One image's scan, ready to be walked: the bits (followed by 1-bits without end: what a read past the end returns), the code
    tables of every block position of the MCU, the geometry."""

    def __init__(self, parsed):
        scan = parsed["scan"]
        self.bits = 8 * len(scan)
        b = np.frombuffer(scan + b"\xff" * 8, np.uint8).astype(np.int64)
        win = np.zeros(len(scan) + 1, np.int64)
        for k in range(5):
            win = (win << 8) | b[k:k + len(scan) + 1]
        self._win = win.tolist()  # _win[i]: bytes i .. i + 4, the first on top
        self.sampling = parsed["sampling"]
        self.per_mcu = BLOCKS_PER_MCU[self.sampling]
        self._dc = [_lookup(*parsed["dht"][c][0]) for c in SLOT_COMPONENT[self.sampling]]
        self._ac = [_lookup(*parsed["dht"][c][1]) for c in SLOT_COMPONENT[self.sampling]]
        self.blocks = geometry(parsed["h"], parsed["w"], self.sampling)[2]

    def subsequences(self, sub_bits):
        return max(1, -(-self.bits // sub_bits))

    def peek32(self, p):
        if p >= self.bits:
            return 0xFFFFFFFF
        return (self._win[p >> 3] >> (8 - (p & 7))) & 0xFFFFFFFF

    def walk(self, state, end, out=None, block=0):
        """Decode every symbol that starts before bit min(end, self.bits), from `state` = (p, slot, k): the bit position of the next
        symbol, the block's position in its MCU, the next zigzag index (0: the DC code is next).  Returns (the state it stops in,
        blocks completed, flags).  A state already at or past the end comes back unchanged.  Nonsense is defined: bits that begin no
        code advance p by one and change nothing else; a run that carries k past 63 ends the block.  out: int64 [blocks, 64] that
        takes every coefficient passed (the DC as its difference), the first block completed or continued being `block`; blocks at
        or past len(out) are decoded and not stored."""
        p, slot, k = state
        end = min(end, self.bits)
        done = flags = 0
        while p < end:
            v = self.peek32(p)
            e = (self._dc if k == 0 else self._ac)[slot][v >> 16]
            if e == 0:
                p += 1
                continue
            length, sym = e >> 8, e & 255
            size = sym & 15
            value = (v >> (32 - length - size)) & ((1 << size) - 1) if size else 0
            if size and value < (1 << (size - 1)):
                value -= (1 << size) - 1
            store = out is not None and block + done < len(out)
            finished = False
            if k == 0:
                flags |= STATUS_CATEGORY if size > 11 else 0
                if store:
                    out[block + done, 0] = value
                k, p = 1, p + length + size
            elif size == 0 and sym != 0xF0:  # end of block
                if store:
                    out[block + done, k:] = 0
                p, finished = p + length, True
            else:
                flags |= STATUS_CATEGORY if size > 10 else 0
                run = 16 if size == 0 else sym >> 4
                if store:
                    out[block + done, k:k + run] = 0
                k += run
                if size and k <= 63:
                    if store:
                        out[block + done, k] = value
                    k += 1
                p, finished = p + length + size, k > 63
            if finished:
                done, k, slot = done + 1, 0, (slot + 1) % self.per_mcu
        return (p, slot, k), done, flags

    def f(self, i, state, sub_bits, out=None, block=0):
        """f_i: subsequence i's step."""
        return self.walk(state, (i + 1) * sub_bits, out, block)


def sequential_states(stream, sub_bits):
    """The entry state of every subsequence, as the sequential decoder passes them: int64 [n, 3]."""
    n = stream.subsequences(sub_bits)
    entry = [(0, 0, 0)]
    for i in range(n - 1):
        entry.append(stream.f(i, entry[i], sub_bits)[0])
    return np.array(entry, np.int64)


def relax(stream, sub_bits):
    """The relaxation, one level: every subsequence but the first starts from the guess (i sub_bits, 0, 0); a round sets
    entry[i + 1] = f_i(entry[i]) wherever entry[i] changed in the round before.  Returns (entries int64 [n, 3], rounds run, the one
    that found nothing to change included)."""
    n = stream.subsequences(sub_bits)
    entry = [(i * sub_bits, 0, 0) for i in range(n)]
    changed, rounds = [True] * n, 0
    while True:
        new = {i + 1: stream.f(i, entry[i], sub_bits)[0] for i in range(n - 1) if changed[i]}
        rounds += 1
        changed = [False] * n
        for j, s in new.items():
            if s != entry[j]:
                entry[j], changed[j] = s, True
        if not any(changed):
            return np.array(entry, np.int64), rounds


def relax_two_level(stream, sub_bits, group=GROUP):
    """The form the kernels run.  A workgroup owns `group` consecutive subsequences and relaxes them among themselves until nothing
    changes (at most `group` rounds, after which they are the chain from the workgroup's first entry); what it hands to the next
    workgroup is seen by that one in the NEXT launch.  The host launches until no workgroup handed over anything new.  Returns
    (entries int64 [n, 3], launches)."""
    n = stream.subsequences(sub_bits)
    groups = -(-n // group)
    entry = [(i * sub_bits, 0, 0) for i in range(n)]
    first = [(g * group * sub_bits, 0, 0) for g in range(groups)]  # what each workgroup is handed
    seen = [None] * groups
    launches = 0
    while True:
        handed, changed = list(first), False
        for g in range(groups):
            lo, hi = g * group, min(n, (g + 1) * group)
            if first[g] != seen[g]:
                entry[lo] = seen[g] = first[g]
                for i in range(lo, hi - 1):
                    entry[i + 1] = stream.f(i, entry[i], sub_bits)[0]
                tail = stream.f(hi - 1, entry[hi - 1], sub_bits)[0]
                if g + 1 < groups and tail != first[g + 1]:
                    handed[g + 1], changed = tail, True
        first = handed
        launches += 1
        if not changed:
            return np.array(entry, np.int64), launches


def coefficients(parsed, sub_bits=None):
    """(int16 [blocks, 64] in zigzag order and scan order, DC values not differences; status).  sub_bits None: one walk over the whole
    scan.  Otherwise the three passes of the kernels: every subsequence counts its blocks from its entry state, a prefix sum gives it
    its first block, it decodes again and stores; then the DC differences are summed per component."""
    stream = Stream(parsed)
    out = np.zeros((stream.blocks, 64), np.int64)
    if sub_bits is None:
        state, done, flags = stream.walk((0, 0, 0), stream.bits, out)
    else:
        entry = [tuple(s) for s in sequential_states(stream, sub_bits).tolist()]
        walks = [stream.f(i, s, sub_bits) for i, s in enumerate(entry)]
        first = np.cumsum([0] + [wk[1] for wk in walks])
        for i, s in enumerate(entry):
            stream.f(i, s, sub_bits, out, int(first[i]))
        state, done, flags = walks[-1][0], int(first[-1]), functools.reduce(lambda a, b: a | b, (wk[2] for wk in walks))
    status = flags | (STATUS_COUNT if done != stream.blocks else 0) | (STATUS_INSIDE if state[2] != 0 or state[0] > stream.bits else 0)
    comp = np.array(SLOT_COMPONENT[stream.sampling])[np.arange(stream.blocks) % stream.per_mcu]
    for c in range(comp.max() + 1):
        out[comp == c, 0] = np.cumsum(out[comp == c, 0])
    return out.astype(np.int16), status


# ---- the pixel rules ----

def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _idct_pass(d, shift):
    """One pass of jidctint (jpeg_idct_islow) over the last axis of int64 [..., 8]."""
    z2, z3 = d[..., 2], d[..., 6]
    z1 = (z2 + z3) * 4433
    t2, t3 = z1 - z3 * 15137, z1 + z2 * 6270
    t0, t1 = (d[..., 0] + d[..., 4]) << 13, (d[..., 0] - d[..., 4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = d[..., 7], d[..., 5], d[..., 3], d[..., 1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, -z3 * 16069 + z5, -z4 * 3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    return np.stack([_descale(o, shift) for o in out], -1)


def samples(coef, q):
    """int16 [n, 64] zigzag coefficients and int64 [64] natural-order table -> int64 [n, 8, 8] samples 0..255."""
    nat = np.zeros((coef.shape[0], 64), np.int64)
    nat[:, R.ZIGZAG] = coef.astype(np.int64)
    d = (nat * q[None, :]).reshape(-1, 8, 8)
    d = _idct_pass(d.transpose(0, 2, 1), 11).transpose(0, 2, 1)  # columns
    return np.clip(_idct_pass(d, 18) + 128, 0, 255)              # rows


def _upsample(c):
    """libjpeg's h2v2_fancy_upsample of the real chroma plane int64 [ch, cw] -> [2 ch, 2 cw]; beyond the plane the edge repeats."""
    ch, cw = c.shape
    y = np.arange(2 * ch)
    far = np.clip((y >> 1) + np.where(y & 1, 1, -1), 0, ch - 1)
    s = 3 * c[y >> 1] + c[far]
    i = np.arange(cw)
    out = np.zeros((2 * ch, 2 * cw), np.int64)
    out[:, 0::2] = (3 * s + s[:, np.clip(i - 1, 0, cw - 1)] + 8) >> 4
    out[:, 1::2] = (3 * s + s[:, np.clip(i + 1, 0, cw - 1)] + 7) >> 4
    return out


def _fix(x):
    return int(x * 65536 + 0.5)


def pixels(coef, q, h, w, sampling):
    """int16 [blocks, 64] and int64 [components, 64] -> uint8 [h, w, 3], what Image.open(...).convert("RGB") returns."""
    mx, my, blocks = geometry(h, w, sampling)
    per = BLOCKS_PER_MCU[sampling]
    c = coef.reshape(my, mx, per, 64)
    comp = SLOT_COMPONENT[sampling]

    def plane(slots, rows, cols):  # the blocks of the given MCU slots, laid out rows x cols inside each MCU
        s = np.stack([samples(c[:, :, j].reshape(-1, 64), q[comp[j]]).reshape(my, mx, 8, 8) for j in slots], 2)
        return s.reshape(my, mx, rows, cols, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(my * rows * 8, mx * cols * 8)

    if sampling == "grey":
        y = plane((0,), 1, 1)[:h, :w]
        return np.repeat(y[..., None], 3, -1).astype(np.uint8)
    if sampling == "444":
        y, cb, cr = (plane((j,), 1, 1)[:h, :w] for j in range(3))
    else:
        y = plane((0, 1, 2, 3), 2, 2)[:h, :w]
        ch, cw = -(-h // 2), -(-w // 2)
        cb, cr = (_upsample(plane((j,), 1, 1)[:ch, :cw])[:h, :w] for j in (4, 5))
    cb, cr = cb - 128, cr - 128
    r = y + ((_fix(1.402) * cr + 32768) >> 16)
    g = y + ((-_fix(0.34414) * cb - _fix(0.71414) * cr + 32768) >> 16)
    b = y + ((_fix(1.772) * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode(data):
    """The file -> uint8 [h, w, 3]."""
    p = parse(data)
    coef, status = coefficients(p)
    assert status == 0, status
    return pixels(coef, p["q"], p["h"], p["w"], p["sampling"])
