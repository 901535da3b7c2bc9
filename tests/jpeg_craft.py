"""TEST INFRASTRUCTURE: baseline JPEGs written from explicit pieces - quantiser tables, per-block zig-zag coefficients,
the component layout, an optional restart interval - with fixed Huffman tables and no encoder in between, so a test
chooses the exact integers the decoders see (coefficients at the limits of the format, inverse-DCT outputs on either
side of the range limit, saturated chroma), plus the exact-arithmetic description of where each such file sits
(``domain``) and the deterministic list of files (``crafted_cases``) the CPU and GPU parity tests share."""
import struct
from functools import lru_cache

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48,
                   41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])   # zig-zag k -> natural

LAYOUTS = {"grey": (1, 1, 1), "444": (3, 1, 1), "422": (3, 2, 1), "420": (3, 2, 2)}   # components, luma h, luma v

# Fixed tables, none of them what an encoder would pick: DC = the twelve categories 0..11 as 4-bit codes 0000..1011;
# AC = EOB, ZRL and every (run, size 1..10) as 8-bit codes 0x00..0xA1.  Neither uses an all-ones code.
DC_SYMS = list(range(12))
AC_SYMS = [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]
_DC_CODE = {s: (i, 4) for i, s in enumerate(DC_SYMS)}
_AC_CODE = {s: (i, 8) for i, s in enumerate(AC_SYMS)}


def _seg(marker, body):
    return b"\xff" + bytes([marker]) + struct.pack(">H", len(body) + 2) + body


def _dht(tc, th, length, syms):
    counts = [0] * 16
    counts[length - 1] = len(syms)
    return _seg(0xC4, bytes([(tc << 4) | th] + counts + list(syms)))


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, nbits):
        self.acc = (self.acc << nbits) | (value & ((1 << nbits) - 1))
        self.n += nbits
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0x00)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def align(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)

    def marker(self, m):
        self.align()
        self.out += bytes([0xFF, m])


def _magnitude(v):
    """(category, the category's extra bits) of ITU T.81 F.1.2.1."""
    s = int(abs(v)).bit_length()
    return s, (v if v >= 0 else v + (1 << s) - 1)


def _put_block(bits, zz, pred):
    diff = int(zz[0]) - pred
    s, extra = _magnitude(diff)
    assert s <= 11, f"DC difference {diff} needs category {s}: not a baseline stream"
    bits.put(*_DC_CODE[s])
    bits.put(extra, s)
    run = 0
    last = max([k for k in range(1, 64) if zz[k]], default=0)
    for k in range(1, last + 1):
        v = int(zz[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            bits.put(*_AC_CODE[0xF0])
            run -= 16
        s, extra = _magnitude(v)
        assert s <= 10, f"AC coefficient {v} needs category {s}: not a baseline stream"
        bits.put(*_AC_CODE[(run << 4) | s])
        bits.put(extra, s)
        run = 0
    if last < 63:
        bits.put(*_AC_CODE[0x00])
    return int(zz[0])


def geometry(width, height, layout):
    """Blocks per column / row of every component plane (whole MCUs), as the decoders lay them out."""
    ncomp, h, v = LAYOUTS[layout]
    mx, my = -(-width // (8 * h)), -(-height // (8 * v))
    return [(my * v, mx * h)] + [(my, mx)] * (ncomp - 1)


def build(width, height, layout, blocks, qts, restart=0):
    """blocks: one int array [bh, bw, 64] per component (zig-zag order, quantised; shapes from ``geometry``);
    qts: one [64] table in zig-zag order (values 1..255) for luma and, with three components, one for both chroma
    planes; restart: MCUs per restart interval, 0 = none.  Returns the file's bytes."""
    ncomp, h, v = LAYOUTS[layout]
    geo = geometry(width, height, layout)
    assert len(blocks) == ncomp and len(qts) == (1 if ncomp == 1 else 2)
    for b, g in zip(blocks, geo):
        assert tuple(np.shape(b)) == (*g, 64), (np.shape(b), g)
    out = b"\xff\xd8" + _seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, q in enumerate(qts):
        q = [int(x) for x in q]
        assert len(q) == 64 and all(1 <= x <= 255 for x in q)
        out += _seg(0xDB, bytes([i] + q))
    comps = b"".join(bytes([c + 1, ((h << 4) | v) if c == 0 else 0x11, min(c, 1)]) for c in range(ncomp))
    out += _seg(0xC0, bytes([8]) + struct.pack(">HH", height, width) + bytes([ncomp]) + comps)
    out += _dht(0, 0, 4, DC_SYMS) + _dht(1, 0, 8, AC_SYMS)          # one table per DHT segment
    if restart:
        out += _seg(0xDD, struct.pack(">H", restart))
    out += _seg(0xDA, bytes([ncomp]) + b"".join(bytes([c + 1, 0x00]) for c in range(ncomp)) + bytes([0, 63, 0]))
    bits, pred, done, rst = _Bits(), [0] * ncomp, 0, 0
    samp = [(h, v)] + [(1, 1)] * (ncomp - 1)
    for my in range(geo[0][0] // v):
        for mx in range(geo[0][1] // h):
            if restart and done and done % restart == 0:
                bits.marker(0xD0 + rst)
                rst, pred = (rst + 1) & 7, [0] * ncomp
            for c in range(ncomp):
                ch, cv = samp[c]
                for y in range(cv):
                    for x in range(ch):
                        pred[c] = _put_block(bits, blocks[c][my * cv + y][mx * ch + x], pred[c])
            done += 1
    bits.align()
    return out + bytes(bits.out) + b"\xff\xd9"


def zigzag_of(natural):
    """[..., 64] natural (row-major) order -> zig-zag order."""
    return np.asarray(natural)[..., ZIGZAG]


# ---------------------------------------------------------------------------------------------------------- domains
class Case:
    """One crafted file and what went into it (coefficients in NATURAL order per component, tables per component)."""

    def __init__(self, name, width, height, layout, blocks, qts, restart):
        self.name, self.width, self.height, self.layout, self.restart = name, width, height, layout, restart
        self.data = build(width, height, layout, blocks, qts, restart)
        inv = np.argsort(ZIGZAG)                                   # natural index -> zig-zag k
        self.coeffs = [np.asarray(b, dtype=np.int64).reshape(-1, 64)[:, inv] for b in blocks]
        self.qts = [np.asarray(qts[min(c, len(qts) - 1)], dtype=np.int64)[inv] for c in range(len(blocks))]

    def domain(self):
        """Where the file sits, in exact int64 arithmetic: does every dequantised coefficient fit int16, does every
        output of the inverse DCT's column pass fit int16, does every output of its row pass (the sample before +128)
        lie in [-512, 511] - the interval inside which every libjpeg range limit agrees - and the extremes."""
        from oracle import jpeg_ref as R
        deq16 = col16 = inr = True
        lo = hi = 0
        for c, q in zip(self.coeffs, self.qts):
            deq = c.reshape(-1, 8, 8) * q.reshape(8, 8)
            ws = R._idct_1d(deq.transpose(0, 2, 1), R.CONST_BITS - R.PASS1_BITS).transpose(0, 2, 1)
            px = R._idct_1d(ws, R.CONST_BITS + R.PASS1_BITS + 3)
            deq16 &= bool(deq.min() >= -32768 and deq.max() <= 32767)
            col16 &= bool(ws.min() >= -32768 and ws.max() <= 32767)
            inr &= bool(px.min() >= -512 and px.max() <= 511)
            lo, hi = min(lo, int(px.min())), max(hi, int(px.max()))
        return {"deq_int16": deq16, "col_int16": col16, "in_range": inr, "min": lo, "max": hi}


def _case(name, width, height, layout, blocks, qts, restart=0):
    return Case(name, width, height, layout, blocks, qts, restart)


# ------------------------------------------------------------------------------------------------------------ cases
SIZES = [(8, 8), (16, 16), (17, 9), (1, 1), (33, 17)]            # (width, height)


def _flat_q(q):
    return [q] * 64


def _zeros(width, height, layout):
    return [np.zeros((*g, 64), dtype=np.int64) for g in geometry(width, height, layout)]


def _dc_for_level(level):
    """With quantiser 8 a DC-only block decodes to descale(8 dc, 3) = dc everywhere: the DC that lands on ``level``."""
    return level


@lru_cache(maxsize=1)
def crafted_cases():
    """[Case] - deterministic (seeded numpy), a few hundred bytes each."""
    rng = np.random.default_rng(20240)
    out = []
    # DC-only blocks at +-2047 x q
    for q in (1, 4, 16):
        for sign in (1, -1):
            b = _zeros(8, 8, "grey")
            b[0][0, 0, 0] = sign * 2047
            out.append(_case(f"dc {sign * 2047} q{q} grey 8x8", 8, 8, "grey", b, [_flat_q(q)]))
    # flat blocks just inside and just outside each limit the range-limit rules care about
    for level in (-512, -129, -128, 127, 128, 511, 512):
        for step in (-1, 0, 1):
            for (w, h) in ((8, 8), (17, 9)):
                b = _zeros(w, h, "grey")
                b[0][..., 0] = _dc_for_level(level + step)
                out.append(_case(f"flat {level + step} grey {w}x{h}", w, h, "grey", b, [_flat_q(8)]))
    # the same limits reached by DC + one AC term (a ramp across the limit inside one block)
    for level in (-512, -129, -128, 127, 128, 511, 512):
        for k in (1, 2, 5):
            b = _zeros(16, 16, "grey")
            b[0][..., 0] = _dc_for_level(level)
            b[0][..., k] = rng.integers(-6, 7, b[0].shape[:2])
            out.append(_case(f"ramp {level} zz{k} grey 16x16", 16, 16, "grey", b, [_flat_q(8)], restart=1))
    # sparse blocks with large AC: a few coefficients at the format's limits, small and large quantisers
    for i in range(60):
        layout = ("grey", "444", "422", "420")[i % 4]
        w, h = SIZES[i % len(SIZES)]
        q = (1, 2, 4, 8, 16, 40)[i % 6]
        b = _zeros(w, h, layout)
        for comp in b:
            for by in range(comp.shape[0]):
                for bx in range(comp.shape[1]):
                    ks = rng.choice(64, size=int(rng.integers(1, 5)), replace=False)
                    mag = int(rng.choice([40, 200, 600, 1023]))
                    comp[by, bx, ks] = rng.integers(-mag, mag + 1, len(ks))
            comp[..., 0] = np.clip(comp[..., 0], -1023, 1023)    # DC differences stay within category 11
        out.append(_case(f"sparse {i} {layout} {w}x{h} q{q}", w, h, layout, b, [_flat_q(q)] * (1 if layout == "grey" else 2),
                         restart=(0, 1, 3)[i % 3]))
    # extreme chroma: Cb / Cr planes saturated in every combination, luma dark / mid / bright, each subsampling
    for layout in ("444", "422", "420"):
        for (w, h) in SIZES:
            for cb, cr in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
                b = _zeros(w, h, layout)
                b[0][..., 0] = rng.choice([-1020, -500, 0, 500, 1016], b[0].shape[:2])
                b[1][..., 0] = cb * rng.choice([1016, 1023, 2040], b[1].shape[:2])
                b[2][..., 0] = cr * rng.choice([1016, 1023, 2040], b[2].shape[:2])
                b[1][..., 1] = rng.integers(-30, 31, b[1].shape[:2])          # edges inside the planes: the upsampling
                b[2][..., 2] = rng.integers(-30, 31, b[2].shape[:2])          # filter sees different neighbours
                for comp in b[1:]:
                    comp[..., 0] = np.clip(comp[..., 0], -1023, 1023) if comp.shape[0] * comp.shape[1] > 1 else comp[..., 0]
                out.append(_case(f"chroma {cb:+d}{cr:+d} {layout} {w}x{h}", w, h, layout, b, [_flat_q(1), _flat_q(1)]))
    return out
