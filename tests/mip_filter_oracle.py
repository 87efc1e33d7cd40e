"""The mip filters (include/ic_amd.h, "mip filters") restated in numpy: P_{l+1} from P_l under ICAMD_MIP_FILTER_SRGB,
ICAMD_MIP_FILTER_ALPHA_WEIGHTED or both, the cascaded pyramid and the per-level encode through the existing oracles
(tests/mips_oracle.py).  The sRGB table is computed here from the transfer function, not read from the product's copy.
Test infrastructure only; the product has no CPU path."""
import hashlib

import numpy as np

import ic_testlib as T
import mips_oracle as M

BOX, SRGB, ALPHA_WEIGHTED = 0, 1, 2
TABLE_SHA256_PREFIX = "fdb7af3c01815a21"  # of the 256 little-endian uint16 values (the issue's figure)
# the shapes of the GPU tier's chains (tests/test_gpu_mip_filters.py)
SHAPES = [(1, 1), (5, 3), (61, 59), (129, 257), (300, 13), (1024, 1024)]
# (codec, source components, filters accepted besides 0)
LAYOUTS = [(T.DXT1, 3, (1,)), (T.DXT1, 4, (1, 2, 3)), (T.DXT5, 4, (1, 2, 3)), (T.ETC1, 3, (1,)), (T.ETC1, 4, (1, 2, 3))]


def _to_linear(c):
    return c / 12.92 if c <= 0.04045 else ((c + 0.055) / 1.055) ** 2.4


TABLE = np.array([int(65535.0 * _to_linear(s / 255.0) + 0.5) for s in range(256)], np.int64)      # T
MIDPOINTS = np.array([(int(TABLE[k - 1]) + int(TABLE[k]) + 1) >> 1 for k in range(1, 256)], np.int64)  # M[1..255]


def table_sha256(table=TABLE):
    return hashlib.sha256(np.asarray(table).astype("<u2").tobytes()).hexdigest()


def inv(v):
    """The number of k in 1..255 with M[k] <= v (elementwise): the code whose T is nearest."""
    return _INV[np.asarray(v, np.int64)]


_INV = np.searchsorted(MIDPOINTS, np.arange(65536), side="right")  # every v the rule can produce


def filter_quads(p0, p1, p2, p3, mip_filter):
    """The rule on arrays of pixels (..., c) uint8, c = 3 or 4 (1 / 2 only with filter 0): the next level's pixels."""
    ps = [np.asarray(p, np.uint8).astype(np.int64) for p in (p0, p1, p2, p3)]
    c = ps[0].shape[-1]
    if mip_filter == BOX:
        return ((ps[0] + ps[1] + ps[2] + ps[3]) >> 2).astype(np.uint8)
    assert c in (3, 4) and (c == 4 or not mip_filter & ALPHA_WEIGHTED)
    srgb = bool(mip_filter & SRGB)
    out = np.zeros(ps[0].shape, np.int64)
    xs = [TABLE[p[..., :3]] if srgb else p[..., :3] for p in ps]
    v = (xs[0] + xs[1] + xs[2] + xs[3] + (2 if srgb else 0)) >> 2
    if c == 4:
        al = [p[..., 3:4] for p in ps]
        A = al[0] + al[1] + al[2] + al[3]
        out[..., 3:4] = A >> 2
        if mip_filter & ALPHA_WEIGHTED:
            num = al[0] * xs[0] + al[1] * xs[1] + al[2] * xs[2] + al[3] * xs[3] + (A >> 1)
            v = np.where(A > 0, num // np.maximum(A, 1), v)
    out[..., :3] = inv(v) if srgb else v
    return out.astype(np.uint8)


def next_level(p, mip_filter):
    """P_{l+1} from P_l (an (h, w, c) uint8 array): rows 2y and min(2y + 1, h - 1), columns alike."""
    h, w = p.shape[:2]
    nh, nw = max(1, h >> 1), max(1, w >> 1)
    y0 = 2 * np.arange(nh)
    y1 = np.minimum(y0 + 1, h - 1)
    x0 = 2 * np.arange(nw)
    x1 = np.minimum(x0 + 1, w - 1)
    return filter_quads(p[y0][:, x0], p[y0][:, x1], p[y1][:, x0], p[y1][:, x1], mip_filter)


def _pixel_literal(quad, mip_filter):
    """One output pixel from four pixels (lists of ints), in plain Python, word for word as the header states it."""
    c = len(quad[0])
    table = [int(t) for t in TABLE]
    mids = [(table[k - 1] + table[k] + 1) >> 1 for k in range(1, 256)]
    out = []
    alphas = [q[3] for q in quad] if c == 4 else [0, 0, 0, 0]
    A = sum(alphas)
    for k in range(min(c, 3)):
        xs = [table[q[k]] if mip_filter & SRGB else q[k] for q in quad]
        v = (sum(xs) + 2) >> 2 if mip_filter & SRGB else sum(xs) >> 2
        if mip_filter & ALPHA_WEIGHTED and A > 0:
            v = (sum(a * x for a, x in zip(alphas, xs)) + (A >> 1)) // A
        out.append(sum(1 for m in mids if m <= v) if mip_filter & SRGB else v)
    if c == 4:
        out.append(A >> 2)
    return out


def next_level_literal(p, mip_filter):
    h, w, c = p.shape
    nh, nw = max(1, h >> 1), max(1, w >> 1)
    out = np.zeros((nh, nw, c), np.uint8)
    for y in range(nh):
        for x in range(nw):
            ya, yb = 2 * y, min(2 * y + 1, h - 1)
            xa, xb = 2 * x, min(2 * x + 1, w - 1)
            quad = [[int(t) for t in p[yy, xx]] for yy, xx in ((ya, xa), (ya, xb), (yb, xa), (yb, xb))]
            out[y, x] = _pixel_literal(quad, mip_filter)
    return out


def pyramid(img, mip_filter, levels=None):
    """[P_0, P_1, ..., P_{levels-1}] of an (h, w, c) image under the filter."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    levels = M.max_levels(h, w) if levels is None else levels
    out = [img]
    for _ in range(1, levels):
        out.append(next_level(out[-1], mip_filter))
    return out


def oracle_chain(codec, img, comps, mip_filter, levels=None, swap=0, strategy=T.SMALLER_ERROR):
    return b"".join(M.oracle_encode(codec, p, comps, swap, strategy) for p in pyramid(img, mip_filter, levels))


def pyramid_bytes(img, mip_filter, levels=None):
    return b"".join(p.tobytes() for p in pyramid(img, mip_filter, levels)[1:])


def alpha_runs(h, w, index=0):
    """An (h, w) alpha plane with runs of 0, runs of 255 and noise, so that quads with A == 0, A == 1020 and everything
    between occur (checked by alpha_cases)."""
    rng = np.random.default_rng(1000 + index)
    a = rng.integers(0, 256, (h, w), dtype=np.uint8)
    cell = 8 if min(h, w) >= 32 else 2  # whole quads of one kind even in thin images
    band = (np.arange(h)[:, None] // cell + np.arange(w)[None, :] // cell + index) % 3
    a[band == 0] = 0
    a[band == 1] = 255
    return a


def mixed_image(h, w, comps, index=0):
    """T.s_mixed colour with the alpha plane of alpha_runs."""
    img = np.ascontiguousarray(T.s_mixed(h, w, 4, index=index).reshape(h, w, 4))
    img[..., 3] = alpha_runs(h, w, index)
    return np.ascontiguousarray(img[..., :comps])


# Every (h, w, index) the GPU tier (tests/test_gpu_mip_filters.py) asks gpu_image for, by test; the CPU tier checks the alpha
# cases on exactly these (tests/test_mip_filters_host.py), and gpu_image refuses an image that is not listed.
ETC1_SHAPES = [(5, 3), (61, 59), (200, 300), (1, 77)]
PYRAMID_SHAPES = SHAPES + [(2048, 2048), (3000, 17)]
FILTER_ZERO_SHAPES = [(61, 59), (300, 200), (129, 257), (5, 3), (300, 13), (1, 1), (13, 300), (61, 59), (256, 256), (130, 257),
                      (1000, 13), (300, 200)]
HOST_FORM_SHAPES = [(61, 59, 5), (300, 200, 0), (1, 9, 3)]  # (h, w, padding bytes per row)
GPU_TEST_IMAGES = (
    [(h, w, i) for i, (h, w) in enumerate(SHAPES)] + [(300, 200, 4)] +
    [(h, w, 10 + i) for i, (h, w) in enumerate(ETC1_SHAPES)] +
    [(h, w, 20 + i) for i, (h, w) in enumerate(PYRAMID_SHAPES)] + [(300, 301, 40 + i) for i in range(5)] +
    [(h, w, h) for h, w in FILTER_ZERO_SHAPES] + [(61, 59, 2), (61, 59, 7), (4096, 4096, 5)] +
    [(256, 256, 100 + i) for i in range(64)] + [(61, 59, 3), (1024, 768, 9), (1024, 768, 10)] +
    [(h, w, h) for h, w, _ in HOST_FORM_SHAPES] + [(61, 130, 6), (200, 136, 8)])


def gpu_image(h, w, comps, index):
    assert (h, w, index) in GPU_TEST_IMAGES, "add (%d, %d, %d) to GPU_TEST_IMAGES" % (h, w, index)
    return mixed_image(h, w, comps, index=index)


def alpha_cases(img):
    """(quads with A == 0, with A == 1020, with 0 < A < 1020) at level 0 -> 1 of an RGBA image."""
    h, w = img.shape[:2]
    nh, nw = max(1, h >> 1), max(1, w >> 1)
    y0 = 2 * np.arange(nh)
    y1 = np.minimum(y0 + 1, h - 1)
    x0 = 2 * np.arange(nw)
    x1 = np.minimum(x0 + 1, w - 1)
    a = img[..., 3].astype(np.int64)
    A = a[y0][:, x0] + a[y0][:, x1] + a[y1][:, x0] + a[y1][:, x1]
    return int((A == 0).sum()), int((A == 1020).sum()), int(((A > 0) & (A < 1020)).sum())
