"""BC4 / BC5 (RGTC) as DEFINED through the reference's DXT5 alpha path (include/ic_amd.h, ICAMD_BC4), computed with the oracle:

* BC4 of channel c = bytes 0..7 of every 16-byte DXT5 block of the RGBA8 image whose alpha is channel c (RGB zero);
* BC5 = BC4(R) then BC4(G) in each 16-byte block;
* decode: the BC4 words as the alpha half of DXT5 blocks, the A channel of the oracle's DXT5 decode.

Shared by tests/test_bc45_host.py (CPU tier) and tests/test_gpu_bc45.py (GPU tier), and scripts/bench_bc45.py."""
import numpy as np

import ic_testlib as T

BC4, BC5 = 5, 6
SHAPES = [(64, 64, 0), (61, 59, 3), (128, 260, 0), (5, 3, 0), (1, 1, 0), (4, 4, 1), (9, 2, 7), (257, 1023, 5)]
# (codec, src_components, swap_rb) of every source layout the C ABI accepts
LAYOUTS = [(BC4, 1, 0), (BC4, 2, 0), (BC4, 3, 0), (BC4, 3, 1), (BC4, 4, 0), (BC4, 4, 1),
           (BC5, 2, 0), (BC5, 3, 0), (BC5, 3, 1), (BC5, 4, 0), (BC5, 4, 1)]


def comps_out(codec):
    return 2 if codec == BC5 else 1


def block_bytes(codec):
    return 16 if codec == BC5 else 8


def encoded_size(codec, gh, gw):
    return ((gh + 3) // 4) * ((gw + 3) // 4) * block_bytes(codec)


def s_saturated(h, w, comps, index=0):
    """Blocks that reach every branch of ComputeBaseAlphas: 0 / 1 / >= 2 pixels at 0 and at 255, all-0 and all-255 blocks,
    narrow and wide ranges (both table modes at many |alpha0 - alpha1|), each channel drawn independently."""
    g = np.random.Generator(np.random.PCG64(T.SEED0 + 7000 + index))
    bh, bw = (h + 3) // 4, (w + 3) // 4
    img = np.empty((bh * 4, bw * 4, comps), np.uint8)
    for by in range(bh):
        for bx in range(bw):
            for c in range(comps):
                kind = int(g.integers(0, 8))
                if kind == 0:
                    v = np.full(16, 0 if g.integers(0, 2) else 255, np.int64)
                else:
                    lo = int(g.integers(1, 255))
                    hi = int(min(254, lo + g.integers(0, 256 if kind > 4 else 16)))
                    v = g.integers(lo, hi + 1, size=16)
                    n0, n255 = int(g.integers(0, 4)), int(g.integers(0, 4))
                    pos = g.permutation(16)
                    v[pos[:n0]] = 0
                    v[pos[n0:n0 + n255]] = 255
                img[by * 4:by * 4 + 4, bx * 4:bx * 4 + 4, c] = v.reshape(4, 4)
    return img[:h, :w].copy()


def every_range_strip():
    """4 x (4 * 2 * 254) one-channel strip: for every D = |alpha0 - alpha1| in 0..253 one block with values in [1, 254] only
    (8-value mode) and one with two zeros added (6-value mode); the rest of each block lies between the two endpoints."""
    g = np.random.Generator(np.random.PCG64(T.SEED0 + 7100))
    blocks = []
    for d in range(254):
        for six in (0, 1):
            lo = int(g.integers(1, 255 - d))
            v = g.integers(lo, lo + d + 1, size=16)
            v[0], v[5] = lo, lo + d
            if six:
                v[3] = v[10] = 0
            blocks.append(v.reshape(4, 4))
    return np.concatenate(blocks, axis=1).astype(np.uint8)


GENERATORS = dict(T.GENERATORS, saturated=s_saturated)


def image(gen, h, w, comps, index=0):
    """(h, w, comps) uint8 test image; 1- and 2-byte layouts are channels of the 4-byte one."""
    return np.ascontiguousarray(GENERATORS[gen](h, w, 4, index)[..., :comps])


def _bc4_blocks(chan, h, w, gh, gw):
    rgba = np.zeros((h, w, 4), np.uint8)
    rgba[..., 3] = chan
    d = T.oracle_encode(T.DXT5, rgba, h, w, 4, gh=gh, gw=gw)
    return np.frombuffer(d, np.uint8).reshape(-1, 16)[:, :8]


def oracle_encode(codec, img, h, w, comps, swap=0, gh=None, gw=None):
    """Expected bytes of one image (h, w, comps) -- or a flat buffer with row padding, given as an (h, w, comps) view."""
    gh = h if gh is None else max(gh, h)
    gw = w if gw is None else max(gw, w)
    img = np.asarray(img, np.uint8).reshape(h, w, comps)
    rch = 2 if (swap and comps >= 3) else 0
    r = _bc4_blocks(img[..., rch], h, w, gh, gw)
    if codec == BC4:
        return r.tobytes()
    return np.concatenate([r, _bc4_blocks(img[..., 1], h, w, gh, gw)], axis=1).tobytes()


def _bc4_decode(words, h, w):
    dxt5 = np.zeros((words.shape[0], 16), np.uint8)
    dxt5[:, :8] = words
    return T.oracle_decode(T.DXT5, dxt5.tobytes(), h, w).reshape(h, w, 4)[..., 3]


def oracle_decode(codec, blocks, h, w, pad=0):
    """Expected R8 / RG8 rows (h rows of w * comps + pad bytes, the pad bytes zero)."""
    b = np.frombuffer(bytes(blocks), np.uint8).reshape(-1, block_bytes(codec))
    chans = [_bc4_decode(b[:, :8], h, w)]
    if codec == BC5:
        chans.append(_bc4_decode(b[:, 8:], h, w))
    rows = np.stack(chans, axis=-1).reshape(h, w * len(chans))
    out = np.zeros((h, w * len(chans) + pad), np.uint8)
    out[:, :w * len(chans)] = rows
    return out.reshape(-1)


def random_words(codec, h, w, seed):
    """Arbitrary block bytes; every fourth BC4 word has alpha0 <= alpha1 forced, so both table modes are common."""
    g = np.random.Generator(np.random.PCG64(seed))
    b = g.integers(0, 256, size=(((h + 3) // 4) * ((w + 3) // 4) * block_bytes(codec) // 8, 8), dtype=np.uint8)
    lo = np.minimum(b[::4, 0], b[::4, 1])
    hi = np.maximum(b[::4, 0], b[::4, 1])
    b[::4, 0], b[::4, 1] = lo, hi
    return b.tobytes()
