"""ICAMD_MIP_FILTER_NORMAL (include/ic_amd.h, "normal-map mip filter") restated in numpy: P_{l+1} from P_l, the cascaded
pyramid and the per-level BC5 encode through tests/bc45_oracle.py; the literal per-pixel loop it is checked against; and the
images of the GPU tier with the cases of the definition planted in them.  Test infrastructure only; the product has no CPU path."""
import math

import numpy as np

import bc45_oracle as B
import mips_oracle as M

NORMAL = 4
UNIT2 = 255 * 255


def isqrt(n):
    """The floor square root, elementwise and exact (n < 2^52: the float root is settled by compare-and-step)."""
    n = np.asarray(n, np.int64)
    s = np.floor(np.sqrt(n.astype(np.float64))).astype(np.int64)
    s = np.where(s * s > n, s - 1, s)
    return np.where((s + 1) * (s + 1) <= n, s + 1, s)


def r_channel(comps, swap):
    return 2 if (swap and comps >= 3) else 0


def z_of(r, g):
    x, y = 2 * np.asarray(r, np.int64) - 255, 2 * np.asarray(g, np.int64) - 255
    return (isqrt(4 * np.maximum(0, UNIT2 - x * x - y * y)) + 1) >> 1


def unclamped_m(V, Ls):
    """(4080 |V| + (Ls >> 1)) // Ls before the clamp at 255 (Ls >= 1)."""
    return (4080 * np.abs(V) + (Ls >> 1)) // Ls


def filter_quads(p0, p1, p2, p3, swap=0, return_unclamped=False):
    """The rule on arrays of pixels (..., c) uint8, c = 2..4: the next level's pixels."""
    ps = [np.asarray(p, np.uint8).astype(np.int64) for p in (p0, p1, p2, p3)]
    c = ps[0].shape[-1]
    assert 2 <= c <= 4
    rc = r_channel(c, swap)
    out = (ps[0] + ps[1] + ps[2] + ps[3]) >> 2  # every byte: the truncating mean; R and G are replaced below
    xs = [2 * p[..., rc] - 255 for p in ps]
    ys = [2 * p[..., 1] - 255 for p in ps]
    zs = [(isqrt(4 * np.maximum(0, UNIT2 - x * x - y * y)) + 1) >> 1 for x, y in zip(xs, ys)]
    X, Y, Z = sum(xs), sum(ys), sum(zs)
    N2 = X * X + Y * Y + Z * Z
    Ls = np.maximum(isqrt(N2 << 8), 1)
    worst = 0
    for V, ch in ((X, rc), (Y, 1)):
        m = unclamped_m(V, Ls)
        worst = max(worst, int(np.where(N2 > 0, m, 0).max(initial=0)))
        v = np.sign(V) * np.minimum(255, m)
        out[..., ch] = np.where(N2 > 0, (v + 256) >> 1, out[..., ch])
    out = out.astype(np.uint8)
    return (out, worst) if return_unclamped else out


def _quad_views(p):
    h, w = p.shape[:2]
    nh, nw = max(1, h >> 1), max(1, w >> 1)
    y0 = 2 * np.arange(nh)
    y1 = np.minimum(y0 + 1, h - 1)
    x0 = 2 * np.arange(nw)
    x1 = np.minimum(x0 + 1, w - 1)
    return p[y0][:, x0], p[y0][:, x1], p[y1][:, x0], p[y1][:, x1]


def next_level(p, swap=0):
    """P_{l+1} from P_l (an (h, w, c) uint8 array): rows 2y and min(2y + 1, h - 1), columns alike."""
    return filter_quads(*_quad_views(p), swap=swap)


def _pixel_literal(quad, swap):
    """One output pixel from four pixels (lists of ints), in plain Python, word for word as the header states it."""
    c = len(quad[0])
    rc = 2 if (swap and c >= 3) else 0
    out = [sum(q[k] for q in quad) >> 2 for k in range(c)]
    X = Y = Z = 0
    for q in quad:
        x, y = 2 * q[rc] - 255, 2 * q[1] - 255
        rem = max(0, 65025 - x * x - y * y)
        X, Y, Z = X + x, Y + y, Z + ((math.isqrt(4 * rem) + 1) >> 1)
    N2 = X * X + Y * Y + Z * Z
    if N2 == 0:
        return out
    Ls = math.isqrt(N2 << 8)
    for V, ch in ((X, rc), (Y, 1)):
        m = min(255, (4080 * abs(V) + (Ls >> 1)) // Ls)
        v = -m if V < 0 else m
        out[ch] = (v + 256) >> 1
    return out


def next_level_literal(p, swap=0):
    h, w, c = p.shape
    nh, nw = max(1, h >> 1), max(1, w >> 1)
    out = np.zeros((nh, nw, c), np.uint8)
    for y in range(nh):
        for x in range(nw):
            ya, yb = 2 * y, min(2 * y + 1, h - 1)
            xa, xb = 2 * x, min(2 * x + 1, w - 1)
            quad = [[int(t) for t in p[yy, xx]] for yy, xx in ((ya, xa), (ya, xb), (yb, xa), (yb, xb))]
            out[y, x] = _pixel_literal(quad, swap)
    return out


def pyramid(img, swap=0, levels=None):
    """[P_0, P_1, ..., P_{levels-1}] of an (h, w, c) image under the normal filter."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    levels = M.max_levels(h, w) if levels is None else levels
    out = [img]
    for _ in range(1, levels):
        out.append(next_level(out[-1], swap))
    return out


def oracle_chain(img, comps, swap=0, levels=None):
    return b"".join(M.oracle_encode(B.BC5, p, comps, swap) for p in pyramid(img, swap, levels))


def pyramid_bytes(img, levels=None):
    return b"".join(p.tobytes() for p in pyramid(img, 0, levels)[1:])


def rg_quad(q):
    """A 2 x 2 x 2 image from four (r, g) pairs in the order p_0..p_3."""
    return np.array(q, np.uint8).reshape(2, 2, 2)


# ---- the images of the GPU tier

CASES = ("N2 == 0", "clamped rem", "flat unit", "general")
_N2_ZERO = np.array([[[255, 255], [0, 0]], [[255, 0], [0, 255]]], np.uint8)


def normal_image(h, w, comps, swap=0, index=0):
    """An (h, w, comps) image whose R (by the BC5 rules) and G hold, in cells of whole level-1 quads that rotate with `index`:
    quads with N2 == 0, texels longer than a unit vector (rem clamped at 0), flat quads of one unit-or-shorter texel, and
    unit normals with noise.  The other bytes are noise."""
    rng = np.random.default_rng(4000 + index)
    img = rng.integers(0, 256, (h, w, comps), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    cell = 8 if min(h, w) >= 32 else 2
    band = (yy // cell + xx // cell + index) % 4
    # unit normals with z > 0 and one code of noise
    ang = rng.uniform(0, 2 * np.pi, (h, w))
    tilt = rng.uniform(0, 1, (h, w))
    noise = rng.integers(-1, 2, (2, h, w))
    rg = np.stack([np.clip(np.rint(127.5 + 127.5 * tilt * np.cos(ang)) + noise[0], 0, 255),
                   np.clip(np.rint(127.5 + 127.5 * tilt * np.sin(ang)) + noise[1], 0, 255)], axis=-1).astype(np.uint8)
    # band 0: the quad (255,255) (0,0) (255,0) (0,255)
    zero = _N2_ZERO[yy % 2, xx % 2]
    # band 1: both components in the outer 20 codes: x^2 + y^2 > 255^2
    far = rng.integers(0, 21, (h, w, 2))
    far = np.where(rng.integers(0, 2, (h, w, 2)) == 1, 255 - far, far).astype(np.uint8)
    # band 2: one unit-or-shorter texel per quad
    flat = rg[(yy // 2) * 2, (xx // 2) * 2]
    x, y = 2 * flat[..., 0].astype(np.int64) - 255, 2 * flat[..., 1].astype(np.int64) - 255
    flat = np.where((x * x + y * y > UNIT2)[..., None], np.uint8(128), flat)
    planted = np.select([(band == 0)[..., None], (band == 1)[..., None], (band == 2)[..., None]], [zero, far, flat], rg)
    img[..., r_channel(comps, swap)] = planted[..., 0]
    img[..., 1] = planted[..., 1]
    return np.ascontiguousarray(img)


def quad_cases(img, swap=0):
    """How many level-1 quads of the image are of each kind of CASES (a quad may be of more than one: a flat quad of an
    over-long texel has a clamped rem)."""
    ps = [p.astype(np.int64) for p in _quad_views(np.asarray(img, np.uint8))]
    rc = r_channel(img.shape[-1], swap)
    xs = [2 * p[..., rc] - 255 for p in ps]
    ys = [2 * p[..., 1] - 255 for p in ps]
    over = [x * x + y * y > UNIT2 for x, y in zip(xs, ys)]
    zs = [(isqrt(4 * np.maximum(0, UNIT2 - x * x - y * y)) + 1) >> 1 for x, y in zip(xs, ys)]
    n2 = sum(xs) ** 2 + sum(ys) ** 2 + sum(zs) ** 2
    same = np.ones(n2.shape, bool)
    for k in range(1, 4):
        same &= (xs[k] == xs[0]) & (ys[k] == ys[0])
    clamped = over[0] | over[1] | over[2] | over[3]
    return (int((n2 == 0).sum()), int(clamped.sum()), int((same & ~clamped).sum()), int(((n2 > 0) & ~same).sum()))


# The GPU tier (tests/test_gpu_mip_normal.py): sizes, source layouts and the index of every image it asks gpu_image for; the
# CPU tier checks the planted cases on exactly these, and gpu_image refuses an image that is not listed.
SIZES = [(1, 1), (5, 3), (8, 8), (64, 64), (129, 65), (131, 257), (256, 256)]
LAYOUTS = [(2, 0), (3, 0), (3, 1), (4, 0), (4, 1)]  # (src_components, swap_rb)
BATCH_SHAPE = (61, 59)
GPU_TEST_IMAGES = ([(h, w, comps, swap, k) for h, w in SIZES for k, (comps, swap) in enumerate(LAYOUTS)] +
                   [(h, w, 2, 0, 10 + i) for i, (h, w) in enumerate(SIZES)] +
                   [BATCH_SHAPE + (comps, swap, 20 + i) for comps, swap in ((2, 0), (3, 1)) for i in range(3)] +
                   [(64, 64, comps, 0, 30) for comps in (2, 3, 4)] + [(129, 65, comps, 0, 31) for comps in (2, 3, 4)])


def gpu_image(h, w, comps, swap, index):
    assert (h, w, comps, swap, index) in GPU_TEST_IMAGES, "add %r to GPU_TEST_IMAGES" % ((h, w, comps, swap, index),)
    return normal_image(h, w, comps, swap, index)
