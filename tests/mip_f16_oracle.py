"""The half-float pixel pyramid (include/ic_amd.h, "half-float pixel pyramid") restated in numpy, twice.

average() is the INDEPENDENT oracle: the four halves, cleaned of NaN and infinities, summed in float64 (exact: four values of at
most 11 significant bits between 2^-24 and 2^16), divided by 4 (exact) and rounded to binary16 by numpy (nearest even), with -0
written as +0.  average_integer() writes the header's integer definition out, step by step.  The host tier holds the two
together and the kernel's routine (csrc/mip_f16.h) against them; the GPU tier holds the kernel against pyramid().
Test infrastructure only; the product has no CPU path."""
import numpy as np

import mips_oracle as M


def clean(h):
    """NaN -> 0, +-Inf -> the largest finite half of the sign; uint16 bit patterns in, uint16 out."""
    h = np.asarray(h, np.uint16)
    m = h & 0x7FFF
    return np.where(m > 0x7C00, 0, np.where(m == 0x7C00, (h & 0x8000) | 0x7BFF, h)).astype(np.uint16)


def average(p0, p1, p2, p3):
    """uint16 bit patterns of the half nearest to the mean of the four cleaned values, ties to even, never -0."""
    v = [clean(p).view(np.float16).astype(np.float64) for p in (p0, p1, p2, p3)]
    out = ((v[0] + v[1] + v[2] + v[3]) / 4).astype(np.float16).view(np.uint16)
    return np.where(out == 0x8000, 0, out).astype(np.uint16)


def fixed(h):
    """F(h): the cleaned half in units of 2^-24, int64."""
    h = clean(h).astype(np.int64)
    e, f = (h >> 10) & 31, h & 1023
    mag = np.where(e == 0, f, (1024 + f) << np.maximum(e - 1, 0))
    return np.where(h & 0x8000, -mag, mag)


def average_integer(p0, p1, p2, p3):
    """The header's definition, literally."""
    s_sum = fixed(p0) + fixed(p1) + fixed(p2) + fixed(p3)
    a = np.abs(s_sum)
    n = np.zeros(a.shape, np.int64)  # bit length
    for bit in range(43):
        n = np.where(a >> bit, bit + 1, n)
    s = np.maximum(2, n - 11)
    q = a >> s
    rem = a & ((np.int64(1) << s) - 1)
    half = np.int64(1) << (s - 1)
    q = q + ((rem > half) | ((rem == half) & (q & 1 == 1)))
    mag = ((s - 2) << 10) + q
    return np.where(mag == 0, 0, np.where(s_sum < 0, mag | 0x8000, mag)).astype(np.uint16)  # (S == 0: q == 0, so mag == 0)


def next_level(p, avg=average):
    """P_{l+1} from P_l, an (h, w, c) uint16 array of bit patterns: rows 2y, min(2y + 1, h - 1), columns alike (mips_oracle)."""
    h, w = p.shape[:2]
    nh, nw = max(1, h >> 1), max(1, w >> 1)
    y0 = 2 * np.arange(nh)
    y1 = np.minimum(y0 + 1, h - 1)
    x0 = 2 * np.arange(nw)
    x1 = np.minimum(x0 + 1, w - 1)
    return avg(p[y0][:, x0], p[y0][:, x1], p[y1][:, x0], p[y1][:, x1])


def pyramid(img, levels=None):
    """[P_0, P_1, ..., P_{levels-1}] of an (h, w, c) uint16 image, each level from the rounded level above."""
    img = np.ascontiguousarray(img).view(np.uint16)
    h, w = img.shape[:2]
    levels = M.max_levels(h, w) if levels is None else levels
    out = [img]
    for _ in range(1, levels):
        out.append(next_level(out[-1]))
    return out


def pyramid_bytes(img, levels=None):
    """What icamd_mip_pyramid_f16_device writes for one image: levels 1 .. levels-1, tight rows, back to back."""
    return b"".join(np.ascontiguousarray(p).tobytes() for p in pyramid(img, levels)[1:])


# ---- content
# The stated quads, as (p0, p1, p2, p3, expected): NaN -> 0, +-Inf -> +-65504, subnormals, cancelling pairs (0x0000, never
# 0x8000), four times the largest half, the two ties, carries into the next exponent.
SPECIAL_QUADS = [
    (0x7E00, 0x7E00, 0xFE00, 0x7C01, 0x0000),
    (0x7E00, 0x4400, 0x4400, 0x4400, 0x4200),  # (0 + 4 + 4 + 4) / 4 = 3
    (0x7C00, 0x7C00, 0x7C00, 0x7C00, 0x7BFF),
    (0xFC00, 0xFC00, 0xFC00, 0xFC00, 0xFBFF),
    (0x7C00, 0xFC00, 0x3C00, 0x3C00, 0x3800),  # the infinities cancel as +-65504: (1 + 1) / 4
    (0x0001, 0x0001, 0x0001, 0x0001, 0x0001),
    (0x0001, 0x0001, 0x0001, 0x0000, 0x0001),  # 0.75 of the smallest subnormal rounds up
    (0x0001, 0x0001, 0x0000, 0x0000, 0x0000),  # a tie of subnormals: to the even 0
    (0x0003, 0x0001, 0x0001, 0x0001, 0x0002),  # 1.5 -> 2 (even)
    (0x03FF, 0x03FF, 0x03FF, 0x03FF, 0x03FF),
    (0x3C00, 0xBC00, 0x0001, 0x8001, 0x0000),
    (0x7BFF, 0xFBFF, 0x8001, 0x0001, 0x0000),
    (0x8001, 0x8001, 0x0001, 0x0001, 0x0000),
    (0x8000, 0x8000, 0x8000, 0x8000, 0x0000),
    (0x8001, 0x8001, 0x8000, 0x8000, 0x0000),  # a negative sum that rounds to nothing (a tie, to the even 0): +0
    (0x8001, 0x8000, 0x8000, 0x8000, 0x0000),
    (0x7BFF, 0x7BFF, 0x7BFF, 0x7BFF, 0x7BFF),
    (0xFBFF, 0xFBFF, 0xFBFF, 0xFBFF, 0xFBFF),
    (0x3C00, 0x3C00, 0x3C01, 0x3C01, 0x3C00),
    (0x3C01, 0x3C01, 0x3C02, 0x3C02, 0x3C02),
    (0x3FFF, 0x3FFF, 0x4000, 0x4000, 0x4000),  # 1 + 1023.5 / 1024: the tie goes to the even 1024, a carry into the exponent
    (0x03FF, 0x03FF, 0x03FF, 0x0403, 0x0400),  # a carry from the subnormals into the first normal exponent
]


def random_quads(n, seed):
    """n quads over the whole bit-pattern range, a third of them confined to neighbouring values so that ties and cancellations
    occur; (n, 4) uint16."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 1 << 16, (n, 4), dtype=np.uint32)
    near = rng.integers(0, 3, n) == 0
    base = rng.integers(0, 1 << 16, n, dtype=np.uint32)
    q[near] = (base[near, None] + rng.integers(0, 4, (int(near.sum()), 4), dtype=np.uint32)) & 0xFFFF
    flip = rng.integers(0, 6, n) == 0  # cancelling pairs: p1 = -p0
    q[flip, 1] = q[flip, 0] ^ 0x8000
    return q.astype(np.uint16)


def image(h, w, chans, seed):
    """An (h, w, chans) uint16 image: noise over the full bit-pattern range with the special quads laid over it as 2 x 2 pixel
    groups at odd offsets (so that they straddle the tiles and 4 x 4 blocks of the kernel) and at even ones."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 1 << 16, (h, w, chans), dtype=np.uint32).astype(np.uint16)
    k = 0
    for y in range(0, h - 1, 3):
        for x in range(y % 2, w - 1, 5):
            p0, p1, p2, p3, _ = SPECIAL_QUADS[k % len(SPECIAL_QUADS)]
            img[y, x, :], img[y, x + 1, :], img[y + 1, x, :], img[y + 1, x + 1, :] = p0, p1, p2, p3
            k += 1
    return img
