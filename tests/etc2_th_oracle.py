"""The T / H search of icamd_encode_etc2_device(ICAMD_ETC2_RGB8, ..., ICAMD_ETC2_MODES_TH) as DEFINED in include/ic_amd.h and
DESIGN.md 3.17, restated in numpy and vectorised over blocks, on top of etc2_colour_oracle (oracle_encode for W, block_texels,
decode_blocks, sse):

* two partitions of the sixteen texels (L: luminance R + 2 G + B against its mean; C: the widest channel against the middle
  of its range), cluster colours quantised to 4 bits per channel without a search;
* per partition the candidates T(a, b), T(b, a), H(a, b), each with the eight distances, every texel on its nearest paint;
* the first smallest error wins, and the block is that word only where it is STRICTLY closer than W.

Shared by tests/test_etc2_th_host.py (CPU tier), tests/test_gpu_etc2_th.py (GPU tier) and scripts/bench_etc2_th.py."""
import numpy as np

import etc2_colour_oracle as C
import ic_testlib as T

ETC2_RGB8 = C.ETC2_RGB8
MODES_DEFAULT, MODES_TH = 0, 1
PART_L, PART_C = 0, 1
KIND_T_AB, KIND_T_BA, KIND_H = 0, 1, 2
NO_ERROR = np.int64(1) << 40  # a dropped candidate


def partitions(tex):
    """[n, 4(y), 4(x), 3] texels -> [2, n, 4, 4] bool: texel in cluster B under partition L and partition C."""
    v = np.asarray(tex, np.int64)
    y = v[..., 0] + 2 * v[..., 1] + v[..., 2]
    in_b_l = 16 * y > y.sum(axis=(1, 2))[:, None, None]
    flat = v.reshape(-1, 16, 3)
    mx, mn = flat.max(axis=1), flat.min(axis=1)
    ch = np.argmax(mx - mn, axis=1)  # (the first largest: R before G before B)
    rows = np.arange(v.shape[0])
    in_b_c = 2 * flat[rows, :, ch] > (mx[rows, ch] + mn[rows, ch])[:, None]
    return np.stack([in_b_l, in_b_c.reshape(-1, 4, 4)])


def cluster_colours(tex, in_b):
    """-> a, b [n, 3] 4-bit codes of clusters A and B, and [n] bool: the partition survives."""
    v = np.asarray(tex, np.int64)
    nb = in_b.sum(axis=(1, 2))
    na = 16 - nb
    sb = (v * in_b[..., None]).sum(axis=(1, 2))
    sa = v.sum(axis=(1, 2)) - sb
    ok = (na > 0) & (nb > 0)
    qa = (30 * sa + 255 * na[:, None]) // (510 * np.maximum(na, 1)[:, None])
    qb = (30 * sb + 255 * nb[:, None]) // (510 * np.maximum(nb, 1)[:, None])
    ok &= (qa != qb).any(axis=1)
    return qa, qb, ok


def paints(kind, a, b, di):
    """[n, 4, 3] paint colours of candidate `kind` on the codes a, b [n, 3] at distance index di, as the decoder defines them."""
    ca, cb = a * 17, b * 17
    d = C.DIST[di]
    if kind == KIND_H:
        return np.stack([np.clip(ca + d, 0, 255), np.clip(ca - d, 0, 255), np.clip(cb + d, 0, 255), np.clip(cb - d, 0, 255)], axis=1)
    c1, c2 = (ca, cb) if kind == KIND_T_AB else (cb, ca)
    return np.stack([c1, np.clip(c2 + d, 0, 255), c2, np.clip(c2 - d, 0, 255)], axis=1)


def nearest(tex, pts):
    """-> [n, 4, 4] index of the nearest paint (ties to the smallest index) and [n] the summed squared distance."""
    v = np.asarray(tex, np.int64)
    dist = ((v[:, :, :, None, :] - pts[:, None, None, :, :]) ** 2).sum(axis=-1)
    k = dist.argmin(axis=-1)  # (numpy: the first minimum)
    return k, dist.min(axis=-1).sum(axis=(1, 2))


def _put(v, field, top, bottom):
    field = np.asarray(field, np.int64)
    assert ((field >> (top - bottom + 1)) == 0).all()
    return v | (field.astype(np.uint64) << np.uint64(bottom))


def _index_bits(v, k):
    for y in range(4):
        for x in range(4):
            p = 4 * x + y
            v = _put(v, k[:, y, x] & 1, p, p)
            v = _put(v, k[:, y, x] >> 1, p + 16, p + 16)
    return v


def pack_t(c1, c2, di, k):
    """[n, 3] codes, [n] distance indices, [n, 4(y), 4(x)] paint indices -> [n, 8] uint8 T words."""
    v = np.zeros(c1.shape[0], np.uint64)
    hi2, lo2 = c1[:, 0] >> 2, c1[:, 0] & 3
    over = hi2 + lo2 >= 4
    v = _put(v, np.where(over, 7, 0), 63, 61)
    v = _put(v, hi2, 60, 59)
    v = _put(v, np.where(over, 0, 1), 58, 58)
    v = _put(v, lo2, 57, 56)
    for field, top in ((c1[:, 1], 55), (c1[:, 2], 51), (c2[:, 0], 47), (c2[:, 1], 43), (c2[:, 2], 39)):
        v = _put(v, field, top, top - 3)
    v = _put(v, di >> 1, 35, 34)
    v = _put(v, np.ones_like(di), 33, 33)
    v = _put(v, di & 1, 32, 32)
    return _index_bits(v, k).astype(">u8").view(np.uint8).reshape(-1, 8)


def pack_h(a, b, di, k):
    """H words of (C1, C2) = (a, b): stored swapped, every index flipped by 2, where the order of the colours must carry the
    other value of di's lowest bit."""
    va = a[:, 0] << 16 | a[:, 1] << 8 | a[:, 2]  # (codes order as the expanded colours do)
    vb = b[:, 0] << 16 | b[:, 1] << 8 | b[:, 2]
    swap = (va >= vb).astype(np.int64) != (di & 1)
    c1 = np.where(swap[:, None], b, a)
    c2 = np.where(swap[:, None], a, b)
    k = np.where(swap[:, None, None], k ^ 2, k)
    v = np.zeros(a.shape[0], np.uint64)
    g1, b1 = c1[:, 1], c1[:, 2]
    v = _put(v, g1 >> 3, 63, 63)
    v = _put(v, c1[:, 0], 62, 59)
    v = _put(v, g1 >> 1, 58, 56)
    over = ((g1 & 1) << 1 | b1 >> 3) + ((b1 >> 1) & 3) >= 4
    v = _put(v, np.where(over, 7, 0), 55, 53)
    v = _put(v, g1 & 1, 52, 52)
    v = _put(v, b1 >> 3, 51, 51)
    v = _put(v, np.where(over, 0, 1), 50, 50)
    v = _put(v, b1 & 7, 49, 47)
    v = _put(v, c2[:, 0], 46, 43)
    v = _put(v, c2[:, 1], 42, 39)
    v = _put(v, c2[:, 2], 38, 35)
    v = _put(v, di >> 2, 34, 34)
    v = _put(v, np.ones_like(di), 33, 33)
    v = _put(v, (di >> 1) & 1, 32, 32)
    return _index_bits(v, k).astype(">u8").view(np.uint8).reshape(-1, 8)


def search(tex):
    """[n, 4, 4, 3] texels -> (words [n, 8] uint8, err [n], choice [n, 3]): the best T / H candidate of every block, its claimed
    error (NO_ERROR: no surviving partition) and its (partition, kind, di), -1 where there is none."""
    v = np.asarray(tex, np.int64)
    n = v.shape[0]
    best_err = np.full(n, NO_ERROR, np.int64)
    best_word = np.zeros((n, 8), np.uint8)
    choice = np.full((n, 3), -1, np.int64)
    parts = partitions(v)
    for part in (PART_L, PART_C):
        a, b, ok = cluster_colours(v, parts[part])
        for kind in (KIND_T_AB, KIND_T_BA, KIND_H):
            for di in range(8):
                k, err = nearest(v, paints(kind, a, b, di))
                better = ok & (err < best_err)  # strictly: a tie stays with the earlier candidate
                if not better.any():
                    continue
                dis = np.full(int(better.sum()), di, np.int64)
                if kind == KIND_H:
                    w = pack_h(a[better], b[better], dis, k[better])
                else:
                    c1, c2 = (a, b) if kind == KIND_T_AB else (b, a)
                    w = pack_t(c1[better], c2[better], dis, k[better])
                best_err[better] = err[better]
                best_word[better] = w
                choice[better] = (part, kind, di)
    return best_word, best_err, choice


def oracle_encode(img, h, w, comps, swap=0, strategy=T.SMALLER_ERROR, gh=None, gw=None, modes=MODES_TH, return_choice=False):
    """Expected bytes of icamd_encode_etc2_device(ICAMD_ETC2_RGB8, strategy, modes, ...) for one (h, w, comps) image.
    return_choice: also [n_blocks, 3] (partition, kind, di) of the blocks that became T / H, -1 in the others."""
    gh = h if gh is None else max(gh, h)
    gw = w if gw is None else max(gw, w)
    img = np.ascontiguousarray(np.asarray(img, np.uint8).reshape(h, w, comps))
    base = np.frombuffer(C.oracle_encode(img, h, w, comps, swap, strategy, gh=gh, gw=gw), np.uint8).reshape(-1, 8)
    if modes == MODES_DEFAULT:
        none = np.full((base.shape[0], 3), -1, np.int64)
        return (base.tobytes(), none) if return_choice else base.tobytes()
    tex = C.block_texels(img, h, w, gh, gw)
    err_w = C.sse(tex, C.decode_blocks(base))
    words, err, choice = search(tex)
    wins = err < err_w
    out = np.where(wins[:, None], words, base)
    choice[~wins] = -1
    return (out.tobytes(), choice) if return_choice else out.tobytes()


def changed(choice):
    return choice[:, 0] >= 0


# ---- inputs

def edges(noise, h=64, w=64, comps=3, seed=0):
    """Two colours of nearly equal luminance meeting along a circle and diagonal bands, plus uniform noise in [-noise, noise]."""
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    m = ((x - 32) ** 2 + (y - 32) ** 2 < 22.4 ** 2) ^ ((x + 2 * y) % 23 < 5)
    img = np.where(m[..., None], np.array([200, 40, 30]), np.array([30, 60, 200])).astype(np.int64)
    if noise:
        g = np.random.Generator(np.random.PCG64(T.SEED0 + 9700 + seed))
        img = img + g.integers(-noise, noise + 1, img.shape)
    out = np.full((h, w, comps), 255, np.uint8)
    out[..., :3] = np.clip(img, 0, 255)
    return out


def equiluminant(h=64, w=64, comps=3):
    """Stripes of (200, 50, 100) and (100, 100, 100): equal R + 2 G + B, so partition L is dropped in every block."""
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    m = (3 * x + 5 * y) % 17 < 6
    out = np.full((h, w, comps), 255, np.uint8)
    out[..., :3] = np.where(m[..., None], np.array([200, 50, 100]), np.array([100, 100, 100]))
    return out


def mixed(comps=3):
    """64 x 64: columns 0..15 of the gradient, 16..31 flat, 32..63 edges(6) -- every wave of 16 x 4 blocks holds lanes that
    skip (W is exact), lanes that keep W and lanes that take T / H."""
    out = edges(6, comps=comps, seed=1)
    out[:, :16, :3] = C.gradient(64, 64)[:, :16]
    out[:, 16:32, :3] = (90, 160, 40)
    return out


def wave_kinds(img, comps=3, strategy=T.SMALLER_ERROR):
    """Per wave of the 64 x 64 tile (16 x 4 blocks each): the numbers of blocks that skip the search (err(W) == 0, or no
    surviving partition), that search and keep W, and that take T / H."""
    base = np.frombuffer(C.oracle_encode(img, 64, 64, comps, 0, strategy), np.uint8).reshape(-1, 8)
    tex = C.block_texels(img, 64, 64, 64, 64)
    skip = (C.sse(tex, C.decode_blocks(base)) == 0) | (search(tex)[1] == NO_ERROR)
    _, choice = oracle_encode(img, 64, 64, comps, 0, strategy, return_choice=True)
    th = changed(choice)
    keep = ~skip & ~th
    assert not (skip & th).any()
    return [(int(skip[r].sum()), int(keep[r].sum()), int(th[r].sum())) for r in (slice(64 * i, 64 * i + 64) for i in range(4))]
