"""ETC2 RGBA8 (include/ic_amd.h, ICAMD_ETC2_RGBA8) as DEFINED in DESIGN.md 3.11, restated in numpy:

* bytes 8..15 of a block = the oracle's ETC1 of the RGBA8 image (alpha ignored), same strategy, grid and edge replication;
* bytes 0..7 = the EAC alpha word of the block's sixteen alphas: 144 candidates (16 tables x 3 multipliers x 3 bases), the
  lexicographically smallest (sse, table, multiplier, base), every texel the smallest index that reaches its minimum;
* decode: the oracle's ETC1 decode of the colour word, alpha = clamp(base + M[table][index] * multiplier, 0, 255).

Vectorised over blocks (one pass per candidate over [n_blocks, 16, 8] arrays).  Shared by tests/test_etc2_host.py (CPU tier),
tests/test_gpu_etc2.py (GPU tier) and scripts/bench_etc2.py."""
import numpy as np

import ic_testlib as T

ETC2_RGBA8 = 16
STRATEGIES = (T.SPLIT_H, T.SPLIT_V, T.SMALLER_ERROR, T.HEURISTIC)

# the 16 x 8 modifier table of the Khronos ETC2 / EAC specification
M = np.array([
    [-3, -6, -9, -15, 2, 5, 8, 14], [-3, -7, -10, -13, 2, 6, 9, 12], [-2, -5, -8, -13, 1, 4, 7, 12], [-2, -4, -6, -13, 1, 3, 5, 12],
    [-3, -6, -8, -12, 2, 5, 7, 11], [-3, -7, -9, -11, 2, 6, 8, 10], [-4, -7, -8, -11, 3, 6, 7, 10], [-3, -5, -8, -11, 2, 4, 7, 10],
    [-2, -6, -8, -10, 1, 5, 7, 9], [-2, -5, -8, -10, 1, 4, 7, 9], [-2, -4, -8, -10, 1, 3, 7, 9], [-2, -5, -7, -10, 1, 4, 6, 9],
    [-3, -4, -7, -10, 2, 3, 6, 9], [-1, -2, -3, -10, 0, 1, 2, 9], [-4, -6, -8, -9, 3, 5, 7, 8], [-3, -5, -7, -9, 2, 4, 6, 8]],
    dtype=np.int64)
SPAN = M[:, 7] - M[:, 3]


def encoded_size(gh, gw):
    return ((gh + 3) // 4) * ((gw + 3) // 4) * 16


def block_alphas(alpha, h, w, gh, gw):
    """[n_blocks, 16] alphas of the block grid max(h, gh) x max(w, gw) over the h x w plane `alpha`, texel i = 4 x + y, fetched
    with the encoders' clamp-to-edge replication (also for the blocks of a padded grid that lie outside the image)."""
    rows, cols = (max(h, gh) + 3) // 4, (max(w, gw) + 3) // 4
    ys = np.minimum(np.arange(rows * 4), h - 1)
    xs = np.minimum(np.arange(cols * 4), w - 1)
    full = np.asarray(alpha, np.int64).reshape(h, w)[np.ix_(ys, xs)]
    b = full.reshape(rows, 4, cols, 4)            # [brow, y, bcol, x]
    return b.transpose(0, 2, 3, 1).reshape(rows * cols, 16)  # [.., x, y] -> i = 4 x + y


def eac_encode(a):
    """[n, 16] alphas (texel i = 4 x + y) -> [n, 8] uint8 EAC words."""
    a = np.asarray(a, np.int64)
    n = a.shape[0]
    lo, hi = a.min(axis=1), a.max(axis=1)
    R = hi - lo
    best_key = np.full(n, np.iinfo(np.int64).max, np.int64)
    best_idx = np.zeros((n, 16), np.int64)
    for t in range(16):
        span = int(SPAN[t])
        m0 = np.clip((2 * R + span) // (2 * span), 1, 15)
        for dm in (-1, 0, 1):
            m = np.clip(m0 + dm, 1, 15)
            b0 = (lo + hi + m + 1) >> 1
            for db in (-1, 0, 1):
                b = np.clip(b0 + db, 0, 255)
                vals = np.clip(b[:, None] + M[t][None, :] * m[:, None], 0, 255)   # [n, 8]
                err = np.abs(vals[:, None, :] - a[:, :, None])                    # [n, 16, 8]
                idx = err.argmin(axis=2)                                          # first (smallest) index of the minimum
                e = err.min(axis=2)
                key = ((e * e).sum(axis=1) << 16) | (t << 12) | (m << 8) | b      # (sse, t, m, b), lexicographic
                better = key < best_key
                best_key = np.where(better, key, best_key)
                best_idx[better] = idx[better]
    word = ((best_key & 0xffff) >> 0).astype(np.uint64)
    t, m, b = (word >> np.uint64(12)) & np.uint64(15), (word >> np.uint64(8)) & np.uint64(15), word & np.uint64(255)
    v = (b << np.uint64(56)) | (m << np.uint64(52)) | (t << np.uint64(48))
    for i in range(16):
        v |= best_idx[:, i].astype(np.uint64) << np.uint64(45 - 3 * i)
    return v.astype(">u8").view(np.uint8).reshape(n, 8)


def eac_decode(words):
    """[n, 8] uint8 EAC words -> [n, 16] alphas, texel i = 4 x + y."""
    v = np.ascontiguousarray(words, np.uint8).reshape(-1, 8).view(">u8").reshape(-1).astype(np.uint64)
    b = (v >> np.uint64(56)).astype(np.int64)
    m = ((v >> np.uint64(52)) & np.uint64(15)).astype(np.int64)
    t = ((v >> np.uint64(48)) & np.uint64(15)).astype(np.int64)
    out = np.empty((v.size, 16), np.int64)
    for i in range(16):
        idx = ((v >> np.uint64(45 - 3 * i)) & np.uint64(7)).astype(np.int64)
        out[:, i] = np.clip(b + M[t, idx] * m, 0, 255)
    return out


def oracle_encode(img, h, w, swap=0, strategy=T.SMALLER_ERROR, gh=None, gw=None, alpha_words=None):
    """Expected bytes for one RGBA8 image, given as an (h, w, 4) array.  alpha_words: the result of eac_encode for this image
    and grid, when the caller has it already (the alpha half does not depend on swap or strategy)."""
    gh = h if gh is None else max(gh, h)
    gw = w if gw is None else max(gw, w)
    img = np.ascontiguousarray(np.asarray(img, np.uint8).reshape(h, w, 4))
    colour = np.frombuffer(T.oracle_encode(T.ETC1, img, h, w, 4, swap, strategy, gh=gh, gw=gw), np.uint8).reshape(-1, 8)
    alpha = eac_encode(block_alphas(img[..., 3], h, w, gh, gw)) if alpha_words is None else alpha_words
    return np.concatenate([alpha, colour], axis=1).tobytes()


def oracle_decode(blocks, h, w, swap=0, pad=0):
    """Expected RGBA8 rows (h rows of 4 w + pad bytes, the pad bytes zero) of blocks whose colour words are ETC1-compatible."""
    b = np.frombuffer(bytes(blocks), np.uint8).reshape(-1, 16)
    rows, cols = (h + 3) // 4, (w + 3) // 4
    rgb = T.oracle_decode(T.ETC1, b[:, 8:].tobytes(), h, w).reshape(h, w, 3)
    a = eac_decode(b[:, :8]).reshape(rows, cols, 4, 4)               # [brow, bcol, x, y]
    plane = a.transpose(0, 3, 1, 2).reshape(rows * 4, cols * 4)[:h, :w]
    out = np.zeros((h, w * 4 + pad), np.uint8)
    px = out[:, :w * 4].reshape(h, w, 4)
    px[..., :3] = rgb[..., ::-1] if swap else rgb
    px[..., 3] = plane
    return out.reshape(-1)


def random_words(h, w, seed):
    """Arbitrary ETC2 RGBA8 blocks for an h x w image: any alpha word (multiplier 0 and clamping bases included -- every fourth
    word gets multiplier 0, the next one base 0 or 255 with a large multiplier); colour words from T.random_blocks restricted to
    the ETC1-compatible modes (individual, or differential whose 5-bit base + 3-bit delta stays in 0..31 on every channel)."""
    g = np.random.Generator(np.random.PCG64(seed))
    n = ((h + 3) // 4) * ((w + 3) // 4)
    col = np.frombuffer(T.random_blocks(T.ETC1, h, w, seed), np.uint8).reshape(n, 8).copy()
    diff = (col[:, 3] & 2) != 0
    for ch in range(3):
        b5 = (col[:, ch] >> 3).astype(np.int64)
        d3 = (col[:, ch] & 7).astype(np.int64)
        s = b5 + np.where(d3 >= 4, d3 - 8, d3)
        bad = diff & ((s < 0) | (s > 31))
        col[bad, ch] &= 0xf8  # delta 0
    al = g.integers(0, 256, size=(n, 8), dtype=np.uint8)
    al[::4, 1] &= 0x0f
    al[1::4, 0] = np.where(g.integers(0, 2, size=al[1::4, 0].shape) == 1, 255, 0)
    al[1::4, 1] |= 0xc0
    return np.concatenate([al, col], axis=1).tobytes()


def every_range_strip():
    """4 x (4 * 256 * 2) alpha plane: for every R = hi - lo in 0..255 two blocks whose extremes are R apart (one at the low end
    of the range, one anywhere), so every m0 of every table is reached, both multiplier clamps included."""
    g = np.random.Generator(np.random.PCG64(T.SEED0 + 9100))
    blocks = []
    for r in range(256):
        for lo in (0, int(g.integers(0, 256 - r))):
            v = g.integers(lo, lo + r + 1, size=16)
            v[3], v[9] = lo, lo + r
            blocks.append(v.reshape(4, 4))
    return np.concatenate(blocks, axis=1).astype(np.uint8)
