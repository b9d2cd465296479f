"""Test-side tools of the PNG decoder (where2edit_amd/csrc/png.hip): a PNG writer on zlib.compressobj + struct that can choose the
filter of every row, the IDAT split and every compressobj knob; a deflate bit writer for hand-built blocks; a pure-Python inflate with a
census of what a stream exercises, an unfilter and the colour step; the list of valid streams and the list of corrupt ones that the host
program (tests/png_core_host.cpp) and the GPU tests both run.  numpy and the standard library only."""
import functools
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
BAND = 64  # W2E_PNG_BAND (tests/test_png_host.py checks it against the header)
STATUS = {"TYPE": 1, "STORED": 2, "LENGTHS": 4, "CODE": 8, "DISTANCE": 16, "INPUT": 32, "SHORT": 64, "LONG": 128, "ADLER": 256, "FILTER": 512}


# ---- writer ----
def chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def pack_rows(pixels, colour, depth=8):
    """pixels uint8 [H,W] or [H,W,C] -> uint8 [H, row bytes]: the rows before filtering (a palette below 8 bits packed, first pixel in
    the high bits)."""
    pixels = np.asarray(pixels, np.uint8)
    h, w = pixels.shape[:2]
    if depth == 8:
        return pixels.reshape(h, w * CHANNELS[colour])
    per = 8 // depth
    padded = np.zeros((h, -(-w // per) * per), np.uint8)
    padded[:, :w] = pixels
    out = np.zeros((h, padded.shape[1] // per), np.uint8)
    for k in range(per):
        out |= padded[:, k::per] << (8 - depth * (k + 1))
    return out


def _paeth(a, b, c):
    a, b, c = a.astype(np.int32), b.astype(np.int32), c.astype(np.int32)
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(rows, bpp, filters):
    """rows uint8 [H, n] -> the filtered bytes with a filter byte in front of each row.  filters: one of 0..4, or one per row."""
    h, n = rows.shape
    filters = [filters] * h if isinstance(filters, int) else list(filters)
    out = bytearray()
    zero = np.zeros(n, np.uint8)
    for y in range(h):
        x, b = rows[y], rows[y - 1] if y else zero
        a, c = np.concatenate((zero[:bpp], x[:-bpp] if n > bpp else x[:0]))[:n], np.concatenate((zero[:bpp], b[:-bpp] if n > bpp else b[:0]))[:n]
        f = filters[y]
        pred = (zero, a, b, ((a.astype(np.int32) + b) >> 1), _paeth(a, b, c))[f if f <= 4 else 0]
        out += bytes([f]) + ((x.astype(np.int32) - pred) & 255).astype(np.uint8).tobytes()
    return bytes(out)


def filter_bpp(colour, depth=8):
    return max(1, CHANNELS[colour] * depth // 8)


def write_png(pixels, colour, depth=8, palette=None, filters=0, idat=None, interlace=0, extra=(), **knobs):
    """pixels -> the bytes of a PNG file.  palette: uint8 [n, 3] for colour 3.  filters: 0..4 or one per row.  idat: the largest IDAT
    payload (None: one chunk).  extra: chunks (kind, body) to put in front of IDAT.  knobs: zlib.compressobj's arguments."""
    pixels = np.asarray(pixels, np.uint8)
    h, w = pixels.shape[:2]
    data = filter_rows(pack_rows(pixels, colour, depth), filter_bpp(colour, depth), filters)
    co = zlib.compressobj(**knobs)
    z = co.compress(data) + co.flush()
    out = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour, 0, 0, interlace))
    if palette is not None:
        out += chunk(b"PLTE", np.asarray(palette, np.uint8).tobytes())
    for kind, body in extra:
        out += chunk(kind, body)
    step = len(z) if idat is None else idat
    for at in range(0, len(z), max(step, 1)):
        out += chunk(b"IDAT", z[at:at + step])
    return out + chunk(b"IEND", b"")


# ---- bit writer ----
class Bits:
    """A deflate bit writer: values go in from the low bit on, Huffman codes from their high bit on."""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, bits):
        self.acc |= (value & ((1 << bits) - 1)) << self.n
        self.n += bits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, bits):
        self.put(int(format(code, f"0{bits}b")[::-1], 2), bits)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def raw(self, data):
        self.align()
        self.out += data

    def stored(self, data, last=False, nlen=None):
        self.put(1 if last else 0, 1), self.put(0, 2), self.align()
        self.out += struct.pack("<HH", len(data), (len(data) ^ 0xffff) if nlen is None else nlen) + data

    def done(self):
        self.align()
        return bytes(self.out)


def canonical(lengths):
    """{symbol: length} -> {symbol: (code, length)} by the rule of RFC 1951, 3.2.2."""
    code, out = 0, {}
    for length in range(1, 16):
        for s in sorted(s for s, l in lengths.items() if l == length):
            out[s] = (code, length)
            code += 1
        code <<= 1
    return out


_CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def dynamic_header(bits, lit, dist, last=True, nlit=None, ndist=None):
    """Write a dynamic block's header for the code lengths lit {symbol: length} and dist {symbol: length}: every length goes out as a
    4-bit code of a code-length code that has 0..15 at length 4 (no repeats).  Returns the two canonical codes."""
    nlit = max(257, max(lit) + 1) if nlit is None else nlit
    ndist = max(1, max(dist) + 1) if ndist is None else ndist
    bits.put(1 if last else 0, 1), bits.put(2, 2)
    bits.put(nlit - 257, 5), bits.put(ndist - 1, 5), bits.put(15, 4)
    for s in _CL_ORDER:
        bits.put(0 if s > 15 else 4, 3)
    for s in range(nlit):
        bits.code(lit.get(s, 0), 4)
    for s in range(ndist):
        bits.code(dist.get(s, 0), 4)
    return canonical(lit), canonical(dist)


def zlib_wrap(deflate, data):
    return b"\x78\x9c" + deflate + struct.pack(">I", zlib.adler32(data))


# ---- the restatement: inflate with a census, unfilter, colour ----
_LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
_LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
_DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
_DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


class Corrupt(ValueError):
    pass


class _Reader:
    def __init__(self, data):
        self.data, self.n, self.at = bytes(data), 8 * len(data), 0

    def take(self, bits):  # at most 32
        if self.at + bits > self.n:
            raise Corrupt("input")
        i = self.at >> 3
        v = (int.from_bytes(self.data[i:i + 5], "little") >> (self.at & 7)) & ((1 << bits) - 1)
        self.at += bits
        return v

    def symbol(self, table, census=None):
        code = 0
        for length in range(1, 16):
            code = (code << 1) | self.take(1)
            s = table.get((length, code))
            if s is not None:
                if census is not None:
                    census["longest_code"] = max(census["longest_code"], length)
                return s
        raise Corrupt("code")


def _table(lengths):
    lengths = {s: l for s, l in enumerate(lengths) if l}
    left = 1
    for length in range(1, 16):
        left = 2 * left - sum(1 for l in lengths.values() if l == length)
        if left < 0:
            raise Corrupt("lengths")
    return {(l, c): s for s, (c, l) in canonical(lengths).items()}


def inflate(stream):
    """A zlib stream -> (the inflated bytes, the census).  Raises Corrupt(reason) on a bad stream."""
    census = {"blocks": {0: 0, 1: 0, 2: 0}, "empty_stored": 0, "longest_code": 0, "largest_distance": 0, "longest_match": 0, "overlaps": set(),
              "run258": 0, "wraps": 0, "huffman_only": True, "wbits": (stream[0] >> 4) + 8}
    r, out = _Reader(stream), bytearray()
    if stream[0] & 15 != 8 or ((stream[0] << 8) | stream[1]) % 31 or stream[1] & 32:
        raise Corrupt("header")
    r.take(16)
    last = 0
    while not last:
        last, kind = r.take(1), r.take(2)
        if kind == 3:
            raise Corrupt("type")
        census["blocks"][kind] += 1
        if kind == 0:
            r.take(-r.at % 8)
            n, nn = r.take(16), r.take(16)
            if n != nn ^ 0xffff:
                raise Corrupt("stored")
            census["empty_stored"] += n == 0
            for _ in range(n):
                out.append(r.take(8))
            continue
        if kind == 1:
            lit, dist = _table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _table([5] * 30)
        else:
            nlit, ndist, ncode = r.take(5) + 257, r.take(5) + 1, r.take(4) + 4
            if nlit > 286 or ndist > 30:
                raise Corrupt("lengths")
            cl = [0] * 19
            for i in range(ncode):
                cl[_CL_ORDER[i]] = r.take(3)
            cl, lens = _table(cl), []
            while len(lens) < nlit + ndist:
                try:
                    s = r.symbol(cl)
                except Corrupt as e:
                    raise Corrupt("lengths" if str(e) == "code" else "input")
                if s < 16:
                    lens.append(s)
                    continue
                if s == 16 and not lens:
                    raise Corrupt("lengths")
                value, repeat = (lens[-1], 3 + r.take(2)) if s == 16 else (0, 3 + r.take(3)) if s == 17 else (0, 11 + r.take(7))
                lens += [value] * repeat
            if len(lens) > nlit + ndist or lens[256] == 0:
                raise Corrupt("lengths")
            lit, dist = _table(lens[:nlit]), _table(lens[nlit:])
        while True:
            s = r.symbol(lit, census)
            if s < 256:
                out.append(s)
            elif s == 256:
                break
            else:
                if s > 285:
                    raise Corrupt("code")
                n = _LEN_BASE[s - 257] + r.take(_LEN_EXTRA[s - 257])
                d = r.symbol(dist, census)
                if d > 29:
                    raise Corrupt("code")
                d = _DIST_BASE[d] + r.take(_DIST_EXTRA[d])
                if d > len(out):
                    raise Corrupt("distance")
                census["huffman_only"] = False
                census["largest_distance"], census["longest_match"] = max(census["largest_distance"], d), max(census["longest_match"], n)
                census["run258"] += n == 258 and d == 1
                if d < n:
                    census["overlaps"].add(d)
                at = len(out)
                if (at - d) // 32768 != (at - d + n - 1) // 32768 or at // 32768 != (at + n - 1) // 32768:
                    census["wraps"] += 1
                for _ in range(n):
                    out.append(out[-d])
    r.take(-r.at % 8)
    if r.take(32) != int.from_bytes(struct.pack("<I", zlib.adler32(bytes(out))), "big"):
        raise Corrupt("adler")
    return bytes(out), census


def unfilter(data, h, row_bytes, bpp):
    """The filtered bytes of h rows (a filter byte + row_bytes each) -> uint8 [h, row_bytes].  Raises Corrupt on a filter above 4."""
    out = np.zeros((h, row_bytes), np.uint8)
    prev = [0] * row_bytes
    for y in range(h):
        f, line = data[y * (row_bytes + 1)], list(data[y * (row_bytes + 1) + 1:(y + 1) * (row_bytes + 1)])
        if f > 4:
            raise Corrupt("filter")
        for x in range(row_bytes):
            a, c = (line[x - bpp], prev[x - bpp]) if x >= bpp else (0, 0)
            b = prev[x]
            if f == 1:
                p = a
            elif f == 2:
                p = b
            elif f == 3:
                p = (a + b) >> 1
            elif f == 4:
                q = a + b - c
                pa, pb, pc = abs(q - a), abs(q - b), abs(q - c)
                p = a if pa <= pb and pa <= pc else b if pb <= pc else c
            else:
                p = 0
            line[x] = (line[x] + p) & 255
        out[y], prev = line, line
    return out


def colour_step(rows, w, colour, depth, palette, mode):
    """Reconstructed rows uint8 [h, row bytes] -> the pixels of mode "RGB" ([h,w,3]) or "raw" ([h,w] grey / palette index, [h,w,C])."""
    h = rows.shape[0]
    if depth < 8:
        per = 8 // depth
        px = np.stack([(rows >> (8 - depth * (k + 1))) & ((1 << depth) - 1) for k in range(per)], axis=2).reshape(h, -1)[:, :w]
    else:
        px = rows.reshape(h, w, CHANNELS[colour])
        px = px[:, :, 0] if CHANNELS[colour] == 1 else px
    if mode == "raw":
        return np.ascontiguousarray(px)
    if colour == 3:
        table = np.zeros((256, 3), np.uint8)
        table[:len(palette)] = palette
        return table[px]
    if colour in (0, 4):
        grey = px if colour == 0 else px[:, :, 0]
        return np.repeat(grey[:, :, None], 3, axis=2)
    return np.ascontiguousarray(px[:, :, :3])


def chunks(data):
    at = 8
    while at + 12 <= len(data):
        n = struct.unpack(">I", data[at:at + 4])[0]
        yield data[at + 4:at + 8], data[at + 8:at + 8 + n]
        at += 12 + n


def decode(data, mode="RGB"):
    """The restatement's decoder: file bytes -> pixels (its own chunk walk, inflate, unfilter and colour step)."""
    palette, z = None, b""
    for kind, body in chunks(data):
        if kind == b"IHDR":
            w, h, depth, colour = struct.unpack(">IIBB", body[:10])
        elif kind == b"PLTE":
            palette = np.frombuffer(body, np.uint8).reshape(-1, 3)
        elif kind == b"IDAT":
            z += body
    bits = CHANNELS[colour] * depth
    row_bytes = (w * bits + 7) // 8
    raw, _ = inflate(z)
    assert len(raw) == h * (row_bytes + 1)
    return colour_step(unfilter(raw, h, row_bytes, max(1, bits // 8)), w, colour, depth, palette, mode)


# ---- the case lists ----
def _rng(seed):
    return np.random.default_rng(seed)


def _z(data, flush_at=None, **knobs):
    co = zlib.compressobj(**knobs)
    if flush_at is None:
        return co.compress(data) + co.flush()
    return co.compress(data[:flush_at]) + co.flush(zlib.Z_SYNC_FLUSH) + co.compress(data[flush_at:]) + co.flush()


def hand_built():
    """One dynamic block that zlib never emits: literal/length code lengths 1..15 (symbols 0..13 at 1..14 bits, end-of-block and length
    symbol 285 at 15), the distance code one symbol (29) of one bit; after 32768 stored bytes it codes the literals 0..13, one match of
    258 bytes (symbol 285) at distance 32768 (24577 + 13 extra bits of ones) and the end of the block."""
    head = _rng(7).integers(0, 256, 32768, dtype=np.uint8).tobytes()
    bits = Bits()
    bits.stored(head)
    lit = {s: s + 1 for s in range(14)}
    lit[256], lit[285] = 15, 15
    lc, dc = dynamic_header(bits, lit, {29: 1})
    for s in range(14):
        bits.code(*lc[s])
    bits.code(*lc[285])
    bits.code(*dc[29]), bits.put(8191, 13)
    bits.code(*lc[256])
    data = head + bytes(range(14))
    data += data[len(data) - 32768:len(data) - 32768 + 258]
    return zlib_wrap(bits.done(), data), data


@functools.lru_cache(maxsize=None)
def valid_cases():
    """{name: (zlib stream, the bytes it inflates to)}: what an inflate can get wrong (tests/test_png_host.py asserts from the census
    that each case shows what it is here for)."""
    r = _rng(1)
    noise = lambda n: r.integers(0, 256, n, dtype=np.uint8).tobytes()
    geo = lambda n: np.minimum(_rng(2).geometric(0.08, n) - 1, 255).astype(np.uint8).tobytes()
    four = r.integers(0, 4, 6000, dtype=np.uint8).tobytes()
    block = noise(5000)
    far = noise(100)
    cases = {
        "stored_two": (noise(70000), dict(level=0)),
        "stored_empty": (four, dict(level=6, flush_at=3000)),
        "fixed": (four[:2000], dict(level=6, strategy=zlib.Z_FIXED)),
        "dynamic_many": (four, dict(level=6, memLevel=1)),
        "huffman_only": (geo(3000), dict(level=6, strategy=zlib.Z_HUFFMAN_ONLY)),
        "run258": (bytes([7]) * 30000, dict(level=6)),
        "period2_3": (b"ab" * 300 + noise(20) + b"xyz" * 300, dict(level=9)),
        "long_codes": (geo(40000), dict(level=9)),
        "far": (far + noise(32100) + far, dict(level=9)),
        "wbits9": (four[:300] + geo(400), dict(level=6, wbits=9)),
        "ring_wrap": (block * 16, dict(level=6)),
    }
    out = {}
    for name, (data, knobs) in cases.items():
        out[name] = (_z(data, **knobs), data)
    for n in range(1, 17):
        data = noise(n)
        out[f"tiny{n}"] = (_z(data, level=6), data)
    out["hand_built"] = hand_built()
    return out


def _fixed(symbols, last=True):
    """A fixed block from ('lit', v) / ('match', length symbol, extra bits, extra, distance symbol, extra bits, extra) / ('end',)."""
    lit = canonical({s: (8 if s < 144 else 9 if s < 256 else 7 if s < 280 else 8) for s in range(288)})
    bits = Bits()
    bits.put(1 if last else 0, 1), bits.put(1, 2)
    for item in symbols:
        if item[0] == "lit":
            bits.code(*lit[item[1]])
        elif item[0] == "end":
            bits.code(*lit[256])
        else:
            _, ls, lb, lv, ds, db, dv = item
            bits.code(*lit[ls]), bits.put(lv, lb), bits.code(ds, 5), bits.put(dv, db)
    return bits.done()


@functools.lru_cache(maxsize=None)
def corrupt_cases():
    """[(name, zlib stream, expected size, the status name or None for "any")]: one entry per way a stream can be bad.  The filter
    entry is separate (corrupt_filter): its stream is fine."""
    valid = valid_cases()
    z, data = valid["dynamic_many"]
    out = [("cut_half", z[:len(z) // 2], len(data), "INPUT"), ("cut_last_byte", z[:-1], len(data), "INPUT")]
    b = Bits()
    b.put(1, 1), b.put(3, 2), b.put(0, 13)
    out.append(("block_type_3", zlib_wrap(b.done(), b""), 16, "TYPE"))
    b = Bits()
    b.stored(b"abcdefgh", last=True, nlen=0x1234)
    out.append(("nlen_wrong", zlib_wrap(b.done(), b"abcdefgh"), 8, "STORED"))
    b = Bits()  # every code-length code of length 1: over-subscribed
    b.put(1, 1), b.put(2, 2), b.put(0, 5), b.put(0, 5), b.put(15, 4)
    for _ in range(19):
        b.put(1, 3)
    b.put(0, 64)
    out.append(("oversubscribed", zlib_wrap(b.done(), b""), 16, "LENGTHS"))
    b = Bits()  # three codes of two bits: 11 is missing, and is then used
    lc, dc = dynamic_header(b, {0: 2, 1: 2, 256: 2}, {0: 1})
    b.code(*lc[0]), b.code(*lc[1]), b.code(3, 2), b.code(*lc[256])
    out.append(("missing_code_used", zlib_wrap(b.done(), b"\0\1"), 16, "CODE"))
    b = Bits()  # the first code-length symbol is the repeat 16
    b.put(1, 1), b.put(2, 2), b.put(0, 5), b.put(0, 5), b.put(15, 4)
    for s in _CL_ORDER:
        b.put(5 if s >= 8 else 4 if s in (0, 1, 2, 3, 4, 5) else 0, 3)
    cl = canonical({**{s: 4 for s in range(6)}, **{s: 5 for s in range(8, 19)}})
    b.code(*cl[16]), b.put(0, 2), b.put(0, 64)
    out.append(("repeat_first", zlib_wrap(b.done(), b""), 16, "LENGTHS"))
    out.append(("distance_before_start", zlib_wrap(_fixed([("lit", 65), ("lit", 66), ("match", 257, 0, 0, 4, 1, 0), ("end",)]), b"AB"), 16, "DISTANCE"))
    out.append(("one_byte_too_many", z, len(data) - 1, "LONG"))
    out.append(("one_byte_too_few", z, len(data) + 1, "SHORT"))
    out.append(("adler_flipped", z[:-2] + bytes([z[-2] ^ 0x10]) + z[-1:], len(data), "ADLER"))
    out.append(("random_4k", b"\x78\x9c" + _rng(3).integers(0, 256, 4096, dtype=np.uint8).tobytes(), 6000, None))
    return out


def corrupt_filter():
    """(zlib stream, h, w) of a 4 x 5 grey image whose third row has filter byte 5."""
    rows = _rng(4).integers(0, 256, (4, 5), dtype=np.uint8)
    data = bytearray(filter_rows(rows, 1, [1, 2, 0, 4]))
    data[2 * 6] = 5
    return zlib.compress(bytes(data)), 4, 5


def wrap_idat(z, h, w, colour=0, depth=8):
    """A PNG file around a given zlib stream."""
    return SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour, 0, 0, 0)) + chunk(b"IDAT", z) + chunk(b"IEND", b"")


def write_corpus(path):
    """The corpus file of tests/png_core_host.cpp (its header comment has the format): the valid list, the corrupt list, the filter
    entry and a few filtered images.  Returns (valid entries, corrupt entries)."""
    entries = []
    for name, (z, data) in valid_cases().items():
        entries.append((name, z, len(data), 0, data, 0, 0, 0, 0, b""))
    for name, z, size, status in corrupt_cases():
        entries.append((name, z, size, -1 if status is None else STATUS[status], b"", 0, 0, 0, 0, b""))
    z, h, w = corrupt_filter()
    entries.append(("filter_byte_5", z, h * (w + 1), 0, b"", h, w, 1, STATUS["FILTER"], b""))
    rng = _rng(5)
    for bpp in (1, 2, 3, 4):
        rows = rng.integers(0, 256, (7, 5 * bpp), dtype=np.uint8)
        data = filter_rows(rows, bpp, [4, 3, 2, 1, 0, 3, 4])
        entries.append((f"filters_bpp{bpp}", zlib.compress(data), len(data), 0, data, 7, 5 * bpp, bpp, 0, rows.tobytes()))
    with open(path, "wb") as f:
        f.write(b"PNGC" + struct.pack("<i", len(entries)))
        for name, z, size, status, out, h, row_bytes, bpp, fstatus, rows in entries:
            f.write(struct.pack("<i", len(name)) + name.encode() + struct.pack("<q", len(z)) + z + struct.pack("<qiq", size, status, len(out)) + out)
            f.write(struct.pack("<iiiiq", h, row_bytes, bpp, fstatus, len(rows)) + rows)
    return sum(e[3] == 0 for e in entries), sum(e[3] != 0 for e in entries)
