"""The mip-chain definition (include/ic_amd.h, mip-chain section) restated in numpy: the cascaded 2 x 2 truncating
pyramid and the per-level encode through the existing oracles (ic_testlib for DXT1 / DXT5 / ETC1, bc45_oracle for BC4 /
BC5).  Test infrastructure only; the product has no CPU path."""
import numpy as np

import bc45_oracle as B
import ic_testlib as T

CODECS = (T.DXT1, T.DXT5, T.ETC1, B.BC4, B.BC5)
# (codec, source components accepted) -- the rules of icamd_encode_device
LAYOUTS = [(T.DXT1, 3), (T.DXT1, 4), (T.DXT5, 4), (T.ETC1, 3), (T.ETC1, 4), (B.BC4, 1), (B.BC4, 2), (B.BC4, 3), (B.BC4, 4),
           (B.BC5, 2), (B.BC5, 3), (B.BC5, 4)]


def max_levels(h, w):
    return 0 if h == 0 or w == 0 else max(h, w).bit_length()


def level_shape(h, w, l):
    return max(1, h >> l), max(1, w >> l)


def block_bytes(codec):
    return 16 if codec in (T.DXT5, B.BC5) else 8


def level_bytes(codec, h, w, l):
    lh, lw = level_shape(h, w, l)
    return ((lh + 3) // 4) * ((lw + 3) // 4) * block_bytes(codec)


def chain_offsets(codec, h, w, levels):
    offs = [0]
    for l in range(levels):
        offs.append(offs[-1] + level_bytes(codec, h, w, l))
    return offs


def next_level(p):
    """P_{l+1} from P_l (an (h, w, c) uint8 array): (a + b + c + d) // 4 of rows 2y, min(2y + 1, h - 1) and columns alike."""
    h, w = p.shape[:2]
    nh, nw = max(1, h >> 1), max(1, w >> 1)
    y0 = 2 * np.arange(nh)
    y1 = np.minimum(y0 + 1, h - 1)
    x0 = 2 * np.arange(nw)
    x1 = np.minimum(x0 + 1, w - 1)
    q = p.astype(np.uint16)
    s = q[y0][:, x0] + q[y0][:, x1] + q[y1][:, x0] + q[y1][:, x1]
    return (s // 4).astype(np.uint8)


def next_level_literal(p):
    """The same rule as plain loops, one pixel and one channel at a time (the restatement next_level is checked against)."""
    h, w, c = p.shape
    nh, nw = max(1, h >> 1), max(1, w >> 1)
    out = np.zeros((nh, nw, c), np.uint8)
    for y in range(nh):
        for x in range(nw):
            ya, yb = 2 * y, min(2 * y + 1, h - 1)
            xa, xb = 2 * x, min(2 * x + 1, w - 1)
            for k in range(c):
                out[y, x, k] = (int(p[ya, xa, k]) + int(p[ya, xb, k]) + int(p[yb, xa, k]) + int(p[yb, xb, k])) // 4
    return out


def pyramid(img, levels=None):
    """[P_0, P_1, ..., P_{levels-1}] of an (h, w, c) image."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    levels = max_levels(h, w) if levels is None else levels
    out = [img]
    for _ in range(1, levels):
        out.append(next_level(out[-1]))
    return out


def oracle_encode(codec, img, comps, swap=0, strategy=T.SMALLER_ERROR):
    """Expected bytes of one level (an (h, w, comps) image): icamd_encode_device's definition for that codec."""
    h, w = img.shape[:2]
    if codec in (B.BC4, B.BC5):
        return B.oracle_encode(codec, img, h, w, comps, swap=swap)
    return T.oracle_encode(codec, np.ascontiguousarray(img), h, w, comps, swap=swap, strategy=strategy)


def oracle_chain(codec, img, comps, levels=None, swap=0, strategy=T.SMALLER_ERROR):
    return b"".join(oracle_encode(codec, p, comps, swap, strategy) for p in pyramid(img, levels))


def pyramid_bytes(img, levels=None):
    """What icamd_mip_pyramid_device writes for one image: levels 1 .. levels-1, tight rows, back to back."""
    return b"".join(p.tobytes() for p in pyramid(img, levels)[1:])
