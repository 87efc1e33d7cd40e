"""BC6H (BPTC float, include/ic_amd.h ICAMD_BC6H_UF16 / ICAMD_BC6H_SF16): the decoder of all fourteen modes restated in numpy, the
8-bit map an independent decoder (Pillow) applies to the halves, and the one-subset encoder's DEFINITION (include/ic_amd.h,
steps 1-6) restated in numpy.  The kernels (csrc/bc6h_block.h) and their host twin are bit-exact against this file.  The mode
layouts below are written out on their own (csrc/bc6h_mode_tables.inc holds the kernels' copy; tests/test_bc6h_host.py compares
the two through the decoders); the partition / anchor tables are the first 32 two-subset entries of BC7's (bc7_oracle)."""
import hashlib

import numpy as np

import bc7_oracle as B7

BC6H_UF16, BC6H_SF16 = 34, 35
W3 = np.array(B7.WEIGHTS[3], np.int64)
W4 = np.array(B7.WEIGHTS[4], np.int64)
P2, A2 = B7.P2[:32], B7.A2[:32]

# Per mode: (mode field, its width, endpoint bits, (R, G, B) delta bits, transformed, subsets, the block's bits after the mode
# field in stream order).  A token names a field (r / g / b, then w = endpoint 0, x = endpoint 1, y, z = the second subset's
# two; d = the partition) and the field's bits that the next stream bits hold, first-last (descending where the stream holds
# them so).
MODES = (
    (0b00, 2, 10, (5, 5, 5), True, 2,
     "gy4 by4 bz4 rw0-9 gw0-9 bw0-9 rx0-4 gz4 gy0-3 gx0-4 bz0 gz0-3 bx0-4 bz1 by0-3 ry0-4 bz2 rz0-4 bz3 d0-4"),
    (0b01, 2, 7, (6, 6, 6), True, 2,
     "gy5 gz4 gz5 rw0-6 bz0 bz1 by4 gw0-6 by5 bz2 gy4 bw0-6 bz3 bz5 bz4 rx0-5 gy0-3 gx0-5 gz0-3 bx0-5 by0-3 ry0-5 rz0-5 d0-4"),
    (0b00010, 5, 11, (5, 4, 4), True, 2,
     "rw0-9 gw0-9 bw0-9 rx0-4 rw10 gy0-3 gx0-3 gw10 bz0 gz0-3 bx0-3 bw10 bz1 by0-3 ry0-4 bz2 rz0-4 bz3 d0-4"),
    (0b00110, 5, 11, (4, 5, 4), True, 2,
     "rw0-9 gw0-9 bw0-9 rx0-3 rw10 gz4 gy0-3 gx0-4 gw10 gz0-3 bx0-3 bw10 bz1 by0-3 ry0-3 bz0 bz2 rz0-3 gy4 bz3 d0-4"),
    (0b01010, 5, 11, (4, 4, 5), True, 2,
     "rw0-9 gw0-9 bw0-9 rx0-3 rw10 by4 gy0-3 gx0-3 gw10 bz0 gz0-3 bx0-4 bw10 by0-3 ry0-3 bz1 bz2 rz0-3 bz4 bz3 d0-4"),
    (0b01110, 5, 9, (5, 5, 5), True, 2,
     "rw0-8 by4 gw0-8 gy4 bw0-8 bz4 rx0-4 gz4 gy0-3 gx0-4 bz0 gz0-3 bx0-4 bz1 by0-3 ry0-4 bz2 rz0-4 bz3 d0-4"),
    (0b10010, 5, 8, (6, 5, 5), True, 2,
     "rw0-7 gz4 by4 gw0-7 bz2 gy4 bw0-7 bz3 bz4 rx0-5 gy0-3 gx0-4 bz0 gz0-3 bx0-4 bz1 by0-3 ry0-5 rz0-5 d0-4"),
    (0b10110, 5, 8, (5, 6, 5), True, 2,
     "rw0-7 bz0 by4 gw0-7 gy5 gy4 bw0-7 gz5 bz4 rx0-4 gz4 gy0-3 gx0-5 gz0-3 bx0-4 bz1 by0-3 ry0-4 bz2 rz0-4 bz3 d0-4"),
    (0b11010, 5, 8, (5, 5, 6), True, 2,
     "rw0-7 bz1 by4 gw0-7 by5 gy4 bw0-7 bz5 bz4 rx0-4 gz4 gy0-3 gx0-4 bz0 gz0-3 bx0-5 by0-3 ry0-4 bz2 rz0-4 bz3 d0-4"),
    (0b11110, 5, 6, (6, 6, 6), False, 2,
     "rw0-5 gz4 bz0 bz1 by4 gw0-5 gy5 by5 bz2 gy4 bw0-5 gz5 bz3 bz5 bz4 rx0-5 gy0-3 gx0-5 gz0-3 bx0-5 by0-3 ry0-5 rz0-5 d0-4"),
    (0b00011, 5, 10, (10, 10, 10), False, 1, "rw0-9 gw0-9 bw0-9 rx0-9 gx0-9 bx0-9"),
    (0b00111, 5, 11, (9, 9, 9), True, 1, "rw0-9 gw0-9 bw0-9 rx0-8 rw10 gx0-8 gw10 bx0-8 bw10"),
    (0b01011, 5, 12, (8, 8, 8), True, 1, "rw0-9 gw0-9 bw0-9 rx0-7 rw11-10 gx0-7 gw11-10 bx0-7 bw11-10"),
    (0b01111, 5, 16, (4, 4, 4), True, 1, "rw0-9 gw0-9 bw0-9 rx0-3 rw15-10 gx0-3 gw15-10 bx0-3 bw15-10"),
)
RESERVED = (0b10011, 0b10111, 0b11011, 0b11111)
FIELDS = ("rw", "rx", "ry", "rz", "gw", "gx", "gy", "gz", "bw", "bx", "by", "bz", "d")


def layout(mode):
    """[(field index into FIELDS, field bit)] for the stream bits after the mode field, in order."""
    out = []
    for tok in MODES[mode][6].split():
        name, rng = (tok[:1], tok[1:]) if tok[0] == "d" else (tok[:2], tok[2:])
        a, _, b = rng.partition("-")
        a, b = int(a), int(b or a)
        out += [(FIELDS.index(name), k) for k in (range(a, b + 1) if b >= a else range(a, b - 1, -1))]
    return out


def header_bits(mode):
    """Bits in front of the indices: 82 in the two-subset modes, 65 in the one-subset modes."""
    return MODES[mode][1] + len(layout(mode))


def mode_of(first_byte):
    """Index into MODES of a block whose byte 0 is given; -1 for the four reserved mode fields."""
    f = first_byte & 3
    if f < 2:
        return f
    f = first_byte & 31
    for m, spec in enumerate(MODES):
        if spec[1] == 5 and spec[0] == f:
            return m
    return -1


def _sext(v, bits):
    bits = np.asarray(bits, np.int64)
    return ((v & ((1 << bits) - 1)) ^ (1 << (bits - 1))) - (1 << (bits - 1))


def unquantise(c, bits, signed):
    c = np.asarray(c, np.int64)
    if not signed:
        if bits >= 15:
            return c
        return np.where(c == 0, 0, np.where(c == (1 << bits) - 1, 0xFFFF, ((c << 16) + 0x8000) >> bits))
    if bits >= 16:
        return c
    a = np.abs(c)
    u = np.where(a == 0, 0, np.where(a >= (1 << (bits - 1)) - 1, 0x7FFF, ((a << 15) + 0x4000) >> (bits - 1)))
    return np.where(c < 0, -u, u)


def finish(x, signed):
    """The interpolated value -> the half's bit pattern."""
    x = np.asarray(x, np.int64)
    if not signed:
        return (x * 31) >> 6
    return np.where(x < 0, (((-x) * 31) >> 5) | 0x8000, (x * 31) >> 5)


def interpolate(a, b, w):
    return (a * (64 - w) + b * w) >> 6  # (arithmetic shift: floor; NO rounding term -- the independent decoder has none)


def _bits(lo, hi, start, width):
    """`width` bits of the 128-bit values (lo, hi: uint64 arrays) from bit `start` (arrays; start + width <= 128)."""
    out = np.zeros(len(lo), np.int64)
    for k in range(4):
        pos = start + k
        word = np.where(pos < 64, lo, hi)
        bit = (word >> (pos & 63).astype(np.uint64)) & np.uint64(1)
        out |= np.where(k < width, bit.astype(np.int64) << k, 0)
    return out


def decode_blocks(blocks, signed):
    """n blocks (bytes or [n, 16] uint8) -> [n, 16, 3] uint16: the half bit patterns of R, G, B, texel i = 4 y + x."""
    b = np.frombuffer(bytes(blocks), np.uint8).reshape(-1, 16) if not isinstance(blocks, np.ndarray) else blocks.reshape(-1, 16)
    n = len(b)
    out = np.zeros((n, 16, 3), np.uint16)
    if n == 0:
        return out
    words = np.ascontiguousarray(b).view("<u8")
    lo, hi = words[:, 0].copy(), words[:, 1].copy()
    modes = np.array([mode_of(int(x)) for x in b[:, 0]])
    for m, (_, mbits, ep, delta, transformed, ns, _) in enumerate(MODES):
        sel = np.flatnonzero(modes == m)
        if len(sel) == 0:
            continue
        l, h = lo[sel], hi[sel]
        f = np.zeros((13, len(sel)), np.int64)
        for pos, (fi, fb) in enumerate(layout(m), start=mbits):
            word = l if pos < 64 else h
            f[fi] |= ((word >> np.uint64(pos & 63)) & np.uint64(1)).astype(np.int64) << fb
        e = f[:12].reshape(3, 4, -1)  # [channel, endpoint w x y z, block]
        if transformed:
            for c in range(3):
                if signed:
                    e[c, 0] = _sext(e[c, 0], ep)
                for k in range(1, 4):
                    e[c, k] = (e[c, 0] + _sext(e[c, k], delta[c])) & ((1 << ep) - 1)
                    if signed:  # read as a 16-bit two's-complement number, NOT sign-extended at ep (only ep = 16 differs)
                        e[c, k] = _sext(e[c, k], 16)
        elif signed:
            e[...] = _sext(e, ep)
        u = unquantise(e, ep, signed)
        if ns == 2:
            part = f[12]
            subset = P2[part]  # [block, 16]
            anchor = A2[part]
            ib, w = 3, W3
        else:
            subset = np.zeros((len(sel), 16), np.int64)
            anchor = np.zeros(len(sel), np.int64)
            ib, w = 4, W4
        pos = np.full(len(sel), header_bits(m), np.int64)
        for i in range(16):
            width = ib - ((i == 0) | ((anchor == i) & (ns == 2))).astype(np.int64)
            k = _bits(l, h, pos, width)
            pos += width
            s = subset[:, i]
            for c in range(3):
                a = np.where(s == 0, u[c, 0], u[c, 2])
                bb = np.where(s == 0, u[c, 1], u[c, 3])
                out[sel, i, c] = finish(interpolate(a, bb, w[k]), signed).astype(np.uint16)
        assert (pos == 128).all()
    return out


def decode(blocks, h, w, signed, pad=0):
    """Block stream of an h x w image -> [h, (w * 8 + pad) // 2] uint16: RGBA16F rows, A = 0x3C00; padding samples are zero.
    pad in bytes, even."""
    rows, cols = (h + 3) // 4, (w + 3) // 4
    t = decode_blocks(blocks, signed).reshape(rows, cols, 4, 4, 3).transpose(0, 2, 1, 3, 4).reshape(rows * 4, cols * 4, 3)[:h, :w]
    out = np.zeros((h, w * 4 + pad // 2), np.uint16)
    px = out[:, :w * 4].reshape(h, w, 4)
    px[..., :3] = t
    px[..., 3] = 0x3C00
    return out


def half_to_byte(bits):
    """What Pillow's reader makes of a decoded half: 0 for f < 0, 255 for f > 1, else trunc(255 f) (f as float32)."""
    f = np.asarray(bits, np.uint16).view(np.float16).astype(np.float32)
    with np.errstate(invalid="ignore"):
        v = np.where(f < 0, np.float32(0), np.where(f > 1, np.float32(255), f * np.float32(255)))
    return np.nan_to_num(v, nan=0.0).astype(np.uint8)


def digest(bytes48):
    return hashlib.sha256(bytes(bytes48)).digest()[:8]


def encoded_size(h, w):
    return ((h + 3) // 4) * ((w + 3) // 4) * 16


# ---- the encoder's definition

T_MAX = 0x7BFF


def target(h, signed):
    """The texel target t of half bit patterns h (any integer array): an integer monotone in the float's value."""
    h = np.asarray(h).astype(np.int64) & 0xFFFF
    m = h & 0x7FFF
    neg = (h & 0x8000) != 0
    t = np.minimum(m, T_MAX)
    t = np.where(m > 0x7C00, 0, t)
    return np.where(neg, -t if signed else 0, t)


def block_texels(img, signed, gh=None, gw=None):
    """[h, w, 3 or 4] uint16 half bits -> [rows * cols, 16, 3] int64 targets of the grid max(h, gh) x max(w, gw)."""
    h, w, _ = img.shape
    rows, cols = (max(h, gh or h) + 3) // 4, (max(w, gw or w) + 3) // 4
    ys = np.minimum(np.arange(rows * 4), h - 1)
    xs = np.minimum(np.arange(cols * 4), w - 1)
    t = target(img[ys][:, xs][..., :3], signed)
    return t.reshape(rows, 4, cols, 4, 3).transpose(0, 2, 1, 3, 4).reshape(rows * cols, 16, 3)


def q_range(signed):
    return (-511, 511) if signed else (0, 1023)


def _signed_value(bits):
    """Sign-magnitude half bits -> the signed integer of the t domain."""
    bits = np.asarray(bits, np.int64)
    return np.where(bits & 0x8000, -(bits & 0x7FFF), bits)


def D(q, signed):
    """The t-domain value a 10-bit endpoint q decodes to at weight 0."""
    d = finish(unquantise(q, 10, signed), signed)
    return _signed_value(d) if signed else d


def targets(t):
    """Step 1 over three channels."""
    lo, hi = t.min(axis=1), t.max(axis=1)
    cs = np.argmax(hi - lo, axis=1)
    n = np.arange(len(t))
    star = t[n, :, cs]
    cov = 16 * (star[:, :, None] * t).sum(axis=1) - star.sum(axis=1)[:, None] * t.sum(axis=1)
    flip = cov < 0
    flip[n, cs] = False
    return np.where(flip, hi, lo), np.where(flip, lo, hi)


def quantise(T, signed):
    """Step 2, by the definition: the smallest q minimising |D(q) - T|."""
    qlo, qhi = q_range(signed)
    q = np.arange(qlo, qhi + 1)
    d = D(q, signed)
    err = np.abs(d[None, :] - np.asarray(T, np.int64).reshape(-1, 1))
    return (q[err.argmin(axis=1)]).reshape(np.shape(T))


def palette(e0, e1, signed):
    """[N, 3] endpoints q -> [N, 16, 3] palette in the t domain."""
    u0, u1 = unquantise(e0, 10, signed), unquantise(e1, 10, signed)
    x = interpolate(u0[:, None, :], u1[:, None, :], W4[None, :, None])
    p = finish(x, signed)
    return _signed_value(p) if signed else p


def indices(t, e0, e1, signed):
    pal = palette(e0, e1, signed)
    d = ((pal[:, None, :, :] - t[:, :, None, :]) ** 2).sum(axis=3)
    return d.argmin(axis=2), d.min(axis=2).sum(axis=1)


def rdiv(n, d):
    return (2 * n + d) // (2 * d)


def refit_targets(t, k, signed):
    w = W4[k]
    a, b, c = ((64 - w) ** 2).sum(axis=1), ((64 - w) * w).sum(axis=1), (w * w).sum(axis=1)
    x, y = ((64 - w)[:, :, None] * t).sum(axis=1), (w[:, :, None] * t).sum(axis=1)
    det = a * c - b * b
    ok = det != 0
    d = np.where(ok, det, 1)[:, None]
    lo = -T_MAX if signed else 0
    t0 = np.clip(rdiv(64 * (c[:, None] * x - b[:, None] * y), d), lo, T_MAX)
    t1 = np.clip(rdiv(64 * (a[:, None] * y - b[:, None] * x), d), lo, T_MAX)
    return t0, t1, ok


def encode_texels(t, signed, stages=False):
    """[N, 16, 3] int64 targets -> [N, 16] uint8 blocks (steps 1-6)."""
    t = np.asarray(t, np.int64)
    t0, t1 = targets(t)
    e0, e1 = quantise(t0, signed), quantise(t1, signed)
    k, sse = indices(t, e0, e1, signed)
    r0, r1, ok = refit_targets(t, k, signed)
    f0, f1 = quantise(r0, signed), quantise(r1, signed)
    k2, sse2 = indices(t, f0, f1, signed)
    take = ok & (sse2 < sse)
    e0, e1 = np.where(take[:, None], f0, e0), np.where(take[:, None], f1, e1)
    k = np.where(take[:, None], k2, k)
    final = np.where(take, sse2, sse)
    pre = (e0.copy(), e1.copy(), k.copy())
    flip = k[:, 0] >= 8
    e0, e1 = np.where(flip[:, None], e1, e0), np.where(flip[:, None], e0, e1)
    k = np.where(flip[:, None], 15 - k, k)
    blocks = pack(e0, e1, k)
    return (blocks, sse, final, take, pre) if stages else blocks


def pack(e0, e1, k):
    """Step 6: mode field 00011, rw gw bw rx gx bx (10 bits each, two's complement), k_0 in 3 bits, k_1.. in 4."""
    out = []
    for n in range(len(k)):
        bits, pos = 0b00011, 5
        for e in (e0, e1):
            for c in range(3):
                bits |= (int(e[n, c]) & 1023) << pos
                pos += 10
        bits |= int(k[n, 0]) << pos
        pos += 3
        for p in range(1, 16):
            bits |= int(k[n, p]) << pos
            pos += 4
        assert pos == 128 and int(k[n, 0]) < 8
        out.append(np.frombuffer(bits.to_bytes(16, "little"), np.uint8))
    return np.stack(out) if out else np.zeros((0, 16), np.uint8)


def oracle_encode(img, signed, gh=None, gw=None):
    return encode_texels(block_texels(img, signed, gh, gw), signed).tobytes()


def metric(img, blocks, signed, gw=None):
    """(sse [3], max_abs [3]) of t(decoded) - t(source) over the image; blocks lie in a grid max(w, gw) wide."""
    h, w, _ = img.shape
    cols, gcols = (w + 3) // 4, (max(w, gw or w) + 3) // 4
    rows = (h + 3) // 4
    b = np.frombuffer(bytes(blocks), np.uint8).reshape(-1, gcols, 16)[:rows, :cols]
    dec = decode(np.ascontiguousarray(b).tobytes(), h, w, signed).reshape(h, w, 4)[..., :3]
    d = target(dec, signed) - target(img[..., :3], signed)
    return (d * d).sum(axis=(0, 1)), np.abs(d).max(axis=(0, 1))


# ---- test content (integer-only generators)

def half_bits(x):
    return np.asarray(x, np.float32).astype(np.float16).view(np.uint16)


CONTENTS = ("noise", "flat", "two_valued", "exponents", "specials", "gradient", "ldr")


def content(name, h, w, chans, seed=0):
    """[h, w, chans] uint16 half bit patterns."""
    g = np.random.Generator(np.random.PCG64(0xBC6000 + 977 * seed + 31 * h + w))
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    img = np.empty((h, w, 4), np.int64)
    if name == "noise":  # every bit pattern: both signs, NaN, Inf and denormals among them
        img[...] = g.integers(0, 65536, (h, w, 4))
    elif name == "flat":
        t = g.integers(0, 65536, ((h + 7) // 8, (w + 7) // 8, 4))
        img[...] = t.repeat(8, 0).repeat(8, 1)[:h, :w]
    elif name == "two_valued":
        t = g.integers(0, 65536, ((h + 7) // 8, (w + 7) // 8, 2, 4))
        pick = g.integers(0, 2, (h, w))
        both = t.repeat(8, 0).repeat(8, 1)[:h, :w]
        img[...] = np.where(pick[..., None] == 0, both[:, :, 0], both[:, :, 1])
    elif name == "exponents":  # every whole block spans 20 exponents: 5 at its first texel, 25 at its last, random mantissas and signs
        i = 4 * (y % 4) + x % 4
        e = 5 + np.where(i == 0, 0, np.where(i == 15, 20, g.integers(0, 21, (h, w))))
        img[...] = (e[..., None] << 10) | g.integers(0, 1024, (h, w, 4)) | (g.integers(0, 8, (h, w, 4)) == 0) << 15
    elif name == "specials":  # NaN, +-Inf, -0, denormals, 0x7BFF, 0xFBFF dealt among calm values
        table = np.array([0x7E00, 0xFE01, 0x7C00, 0xFC00, 0x8000, 0x0001, 0x83FF, 0x7BFF, 0xFBFF, 0x0000, 0x3C00, 0xBC00, 0x7C01])
        img[...] = 0x3800 + g.integers(0, 512, (h, w, 4))
        pick = g.integers(0, 3 * len(table), (h, w, 4))
        img[...] = np.where(pick < len(table), table[pick % len(table)], img)
    elif name == "gradient":  # smooth HDR: magnitudes from 2^-6 to 2^12 along the diagonal, a little noise
        t = (x * 18 * 1024 // max(w - 1, 1) + y * 1024 // max(h - 1, 1)) + g.integers(0, 16, (h, w))
        for c in range(4):
            img[..., c] = np.clip((9 << 10) + t + 300 * c, 0, T_MAX)
    elif name == "ldr":  # [0, 1] ramps
        v = np.stack([x / max(w - 1, 1), y / max(h - 1, 1), (x + y) / max(w + h - 2, 1), 1 - x / max(w - 1, 1)], axis=2)
        img[...] = half_bits(v)
    else:
        raise ValueError(name)
    return (img & 0xFFFF).astype(np.uint16)[..., :chans].copy()


# ---- random blocks for the decoder tests

def random_block(g, mode, partition=None, ones=False):
    """A block of MODES[mode] (mode 14..17: the reserved fields): the partition fixed where asked, other bits random / all ones."""
    v = (1 << 128) - 1 if ones else int.from_bytes(g.integers(0, 256, 16, dtype=np.uint8).tobytes(), "little")
    if mode >= 14:
        return ((v >> 5 << 5) | RESERVED[mode - 14]).to_bytes(16, "little")
    field, mbits = MODES[mode][0], MODES[mode][1]
    v = (v >> mbits << mbits) | field
    if partition is not None and MODES[mode][5] == 2:
        v = (v & ~(31 << 77)) | partition << 77
    return v.to_bytes(16, "little")


def stratified_blocks(n, seed):
    """n blocks cycling over the fourteen modes and the four reserved fields."""
    g = np.random.Generator(np.random.PCG64(seed))
    return b"".join(random_block(g, i % 18) for i in range(n))
