"""ETC2 RGB8 with punch-through alpha (include/ic_amd.h, ICAMD_ETC2_RGB8A1) as STATED there, restated in plain numpy and
vectorised over blocks: the decoder (four modes under both values of the opaque bit) and the encoder (all-transparent word, ETC1
word or masked differential search D, planar choice).  E comes from the ETC1 oracle, the planar word and the T / H / planar
texels from etc2_colour_oracle.

Shared by tests/test_etc2_a1_host.py (CPU tier), tests/test_gpu_etc2_a1.py (GPU tier) and scripts/bench_etc2_a1.py."""
import numpy as np

import etc2_colour_oracle as C
import ic_testlib as T

ETC2_RGB8A1 = 21
STRATEGIES = C.STRATEGIES
MOD_A = np.array([2, 5, 9, 13, 18, 24, 33, 47], np.int64)
MOD_B = np.array([8, 17, 29, 42, 60, 80, 106, 183], np.int64)
ALL_TRANSPARENT = bytes.fromhex("00000000ffff0000")
DIFFERENTIAL, T_MODE, H_MODE, PLANAR = C.DIFFERENTIAL, C.T_MODE, C.H_MODE, C.PLANAR
# the classes of a block, by the definition
CLEAR, E_KEPT, D_OPAQUE, PLANAR_CHOSEN, D_MASKED = range(5)


def encoded_size(gh, gw):
    return ((gh + 3) // 4) * ((gw + 3) // 4) * 8


def _as_words(blocks):
    if isinstance(blocks, np.ndarray):
        return np.ascontiguousarray(blocks, np.uint8).reshape(-1, 8)
    return np.frombuffer(bytes(blocks), np.uint8).reshape(-1, 8)


def opaque_bit(blocks):
    return (_as_words(blocks)[:, 3] >> 1) & 1


def modes(blocks):
    """[n] DIFFERENTIAL, T_MODE, H_MODE or PLANAR: the overflow rule applies whatever Op, and there is no individual mode."""
    b = _as_words(blocks).copy()
    b[:, 3] |= 2
    return C.modes(b)


def _index_planes(lo):
    """[n] low words -> [n, 4(y), 4(x)] texel indices k = bit(p) | bit(p + 16) << 1, p = 4 x + y."""
    k = np.empty((lo.shape[0], 4, 4), np.int64)
    for y in range(4):
        for x in range(4):
            p = 4 * x + y
            k[:, y, x] = ((lo >> p) & 1) | (((lo >> (p + 16)) & 1) << 1)
    return k


def _sub_block(flip):
    """[4(y), 4(x)] sub-block number of every texel: flip 0 splits by columns, flip 1 by rows."""
    y, x = np.mgrid[0:4, 0:4]
    return (y >= 2).astype(np.int64) if flip else (x >= 2).astype(np.int64)


def _expand5(v):
    return v << 3 | v >> 2


def _decode_differential_punch(b):
    """Op = 0 differential words -> [n, 4, 4, 4]: modifiers {0, +b, transparent, -b}."""
    hi, lo = C._words(b)
    n = hi.shape[0]
    base = np.empty((n, 2, 3), np.int64)
    for ch in range(3):
        b5 = (hi >> (27 - 8 * ch)) & 31
        d3 = (hi >> (24 - 8 * ch)) & 7
        base[:, 0, ch] = _expand5(b5)
        base[:, 1, ch] = _expand5(b5 + np.where(d3 >= 4, d3 - 8, d3))
    table = np.stack([(hi >> 5) & 7, (hi >> 2) & 7], axis=1)
    flip = hi & 1
    sub = np.where(flip[:, None, None] == 1, _sub_block(1)[None], _sub_block(0)[None])      # [n, 4, 4]
    k = _index_planes(lo)
    rows = np.arange(n)[:, None, None]
    bmag = MOD_B[table[rows, sub]]
    mod = np.where(k == 0, 0, np.where(k == 1, bmag, -bmag))
    rgb = np.clip(base[rows, sub] + mod[..., None], 0, 255)
    out = np.concatenate([rgb, np.full((n, 4, 4, 1), 255, np.int64)], axis=-1)
    out[k == 2] = 0
    return out


def decode_blocks(blocks):
    """Any 8-byte words -> [n, 4(y), 4(x), 4] uint8 RGBA texels."""
    b = _as_words(blocks)
    n = b.shape[0]
    m, op = modes(b), opaque_bit(b)
    as_rgb8 = b.copy()
    as_rgb8[:, 3] |= 2  # Op = 1 (and planar): the ICAMD_ETC2_RGB8 word with the same bits, alpha 255
    out = np.concatenate([C.decode_blocks(as_rgb8).astype(np.int64), np.full((n, 4, 4, 1), 255, np.int64)], axis=-1)
    sel = (op == 0) & (m == DIFFERENTIAL)
    if sel.any():
        out[sel] = _decode_differential_punch(b[sel])
    sel = (op == 0) & ((m == T_MODE) | (m == H_MODE))
    if sel.any():  # paint 2 is the transparent texel
        k = _index_planes(C._words(b[sel])[1])
        part = out[sel]
        part[k == 2] = 0
        out[sel] = part
    return out.astype(np.uint8)


def oracle_decode(blocks, h, w, swap=0, pad=0):
    """Expected RGBA8 rows (h rows of 4 w + pad bytes, the pad bytes zero); swap: stored R goes to the third byte."""
    rows, cols = (h + 3) // 4, (w + 3) // 4
    tex = decode_blocks(blocks).reshape(rows, cols, 4, 4, 4)
    img = tex.transpose(0, 2, 1, 3, 4).reshape(rows * 4, cols * 4, 4)[:h, :w]
    if swap:
        img = img[..., [2, 1, 0, 3]]
    out = np.zeros((h, w * 4 + pad), np.uint8)
    out[:, :w * 4] = img.reshape(h, w * 4)
    return out.reshape(-1)


# ---- encoder

def block_texels(img, h, w, gh, gw):
    """[n_blocks, 4(y), 4(x), 4] RGBA texels of the block grid max(h, gh) x max(w, gw), clamp-to-edge replication."""
    rows, cols = (max(h, gh) + 3) // 4, (max(w, gw) + 3) // 4
    ys = np.minimum(np.arange(rows * 4), h - 1)
    xs = np.minimum(np.arange(cols * 4), w - 1)
    full = np.asarray(img).reshape(h, w, 4).astype(np.int64)[np.ix_(ys, xs)]
    return full.reshape(rows, 4, cols, 4, 4).transpose(0, 2, 1, 3, 4).reshape(rows * cols, 4, 4, 4)


def search_bases(rgb, opq, flip):
    """The bases step of D: [m, 2, 3] q5 per sub-block and channel, and [m, 2] the opaque counts n."""
    sub = _sub_block(flip)
    q5 = np.zeros((rgb.shape[0], 2, 3), np.int64)
    cnt = np.zeros((rgb.shape[0], 2), np.int64)
    for s in range(2):
        sel = opq & (sub == s)[None]
        cnt[:, s] = sel.sum(axis=(1, 2))
        sums = (rgb * sel[..., None]).sum(axis=(1, 2))
        q5[:, s] = sums // (8 * np.maximum(cnt[:, s], 1))[:, None]
    q5[cnt[:, 0] == 0, 0] = q5[cnt[:, 0] == 0, 1]
    q5[cnt[:, 1] == 0, 1] = q5[cnt[:, 1] == 0, 0]
    return q5, cnt


def search(rgb, opq, op, flip):
    """D on one partition.  rgb [m, 4, 4, 3] int, opq [m, 4, 4] bool, op and flip scalars -> ([m, 8] uint8 words, [m] error)."""
    rgb = np.asarray(rgb, np.int64)
    m = rgb.shape[0]
    sub = _sub_block(flip)
    q5, _ = search_bases(rgb, opq, flip)
    d = q5[:, 1] - q5[:, 0]
    c = np.clip(d, -4, 3)
    e = d - c
    a = q5[:, 0] + np.sign(e) * (np.abs(e) // 2)  # C division: toward zero
    base = np.stack([_expand5(a), _expand5(a + c)], axis=1)  # [m, 2, 3]
    assert (a >= 0).all() and (a <= 31).all() and (a + c >= 0).all() and (a + c <= 31).all()
    index = np.full((m, 4, 4), 2, np.int64)  # transparent texels: index 2
    table = np.zeros((m, 2), np.int64)
    total = np.zeros(m, np.int64)
    for s in range(2):
        sel = opq & (sub == s)[None]
        best = None
        for t in range(8):
            mods = np.array([MOD_A[t] if op else 0, MOD_B[t], -MOD_A[t], -MOD_B[t]], np.int64)
            cand = np.clip(base[:, s, None, :] + mods[None, :, None], 0, 255)               # [m, 4(k), 3]
            dist = ((rgb[:, :, :, None, :] - cand[:, None, None, :, :]) ** 2).sum(axis=-1)  # [m, 4, 4, 4(k)]
            if not op:
                dist[..., 2] = 1 << 40
            k = dist.argmin(axis=-1)  # (the first minimum: the smallest index)
            err = (dist.min(axis=-1) * sel).sum(axis=(1, 2))
            if best is None:
                best, best_k = err.copy(), k.copy()
            else:
                better = err < best
                best[better], best_k[better], table[better, s] = err[better], k[better], t
        index[sel] = best_k[sel]
        total += best
    hi = np.full(m, (2 if op else 0) | (1 if flip else 0), np.int64) | table[:, 0] << 5 | table[:, 1] << 2
    for ch in range(3):
        hi |= a[:, ch] << (27 - 8 * ch) | (c[:, ch] & 7) << (24 - 8 * ch)
    lo = np.zeros(m, np.int64)
    for y in range(4):
        for x in range(4):
            p = 4 * x + y
            lo |= (index[:, y, x] & 1) << p | (index[:, y, x] >> 1) << (p + 16)
    words = ((hi << 32) | lo).astype(np.uint64).astype(">u8").view(np.uint8).reshape(-1, 8)
    return words, total


def oracle_encode(img, h, w, swap=0, strategy=T.SMALLER_ERROR, gh=None, gw=None, return_classes=False):
    """Expected ICAMD_ETC2_RGB8A1 bytes of one (h, w, 4) image.  return_classes: also a dict with the [n_blocks] class of every
    block (CLEAR, E_KEPT, D_OPAQUE, PLANAR_CHOSEN, D_MASKED; PLANAR_CHOSEN overrides the class of C), "c_words" (C of the opaque
    blocks, zero elsewhere) and "opaque" ([n, 4, 4] bool)."""
    gh = h if gh is None else max(gh, h)
    gw = w if gw is None else max(gw, w)
    img = np.ascontiguousarray(np.asarray(img, np.uint8).reshape(h, w, 4))
    tex = block_texels(img, h, w, gh, gw)
    rgb, opq = tex[..., :3], tex[..., 3] >= 128
    n = tex.shape[0]
    n_opq = opq.sum(axis=(1, 2))
    out = np.zeros((n, 8), np.uint8)
    cls = np.full(n, CLEAR, np.int64)
    out[n_opq == 0] = np.frombuffer(ALL_TRANSPARENT, np.uint8)

    full = n_opq == 16
    c_words = np.zeros((n, 8), np.uint8)
    if full.any():
        e = np.frombuffer(T.oracle_encode(T.ETC1, img, h, w, 4, swap, strategy, gh=gh, gw=gw), np.uint8).reshape(-1, 8)
        c = e[full].copy()
        kind = np.full(c.shape[0], E_KEPT, np.int64)
        individual = (c[:, 3] & 2) == 0
        for flip in (0, 1):
            sel = individual & ((c[:, 3] & 1) == flip)
            if sel.any():
                c[sel] = search(rgb[full][sel], opq[full][sel], 1, flip)[0]
                kind[sel] = D_OPAQUE
        sse_c = C.sse(rgb[full], C.decode_blocks(c))
        codes = C.planar_fit(rgb[full])
        planar = C.sse(rgb[full], C.planar_texels(codes)) < sse_c
        out[full] = np.where(planar[:, None], C.planar_pack(codes), c)
        cls[full] = np.where(planar, PLANAR_CHOSEN, kind)
        c_words[full] = c

    mixed = (n_opq > 0) & (n_opq < 16)
    if mixed.any():
        flips = {T.SPLIT_H: (1,), T.SPLIT_V: (0,)}.get(strategy, (0, 1))
        best_w, best_e = None, None
        for flip in flips:
            wd, err = search(rgb[mixed], opq[mixed], 0, flip)
            if best_w is None:
                best_w, best_e = wd, err
            else:
                better = err < best_e  # (a tie keeps flip 0)
                best_w[better], best_e[better] = wd[better], err[better]
        out[mixed] = best_w
        cls[mixed] = D_MASKED
    if return_classes:
        return out.tobytes(), {"class": cls, "c_words": c_words, "opaque": opq, "rgb": rgb}
    return out.tobytes()


# ---- inputs

def random_words(h, w, seed, only=None, op=None):
    """Arbitrary 8-byte words for an h x w image: the four modes interleaved block by block (block i takes mode 1 + i % 4 of
    etc2_colour_oracle, or every block `only`), the opaque bit alternating every four blocks (or every block `op`)."""
    n = ((h + 3) // 4) * ((w + 3) // 4)
    b = np.empty((n, 8), np.uint8)
    for mode in (DIFFERENTIAL, T_MODE, H_MODE, PLANAR):
        sel = (np.arange(n) % 4 == mode - 1) if only is None else np.full(n, only == mode)
        k = int(sel.sum())
        if k:
            b[sel] = np.frombuffer(C.random_colour_words(4, 4 * k, seed + mode, only=mode), np.uint8).reshape(-1, 8)
    bit = ((np.arange(n) // 4) % 2) if op is None else np.full(n, op)
    b[:, 3] = (b[:, 3] & 0xfd) | (bit.astype(np.uint8) << 1)
    return b.tobytes()


def alpha_blobs(h, w, index=0):
    """A blobby cut-out mask: alpha 255 inside discs of radius 2..9 that cover about a third of the image, 0 outside, a band
    of in-between values along the rims."""
    g = np.random.Generator(np.random.PCG64(T.SEED0 + 9700 + index))
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    a = np.zeros((h, w), np.int64)
    for _ in range(max(3, h * w // 250)):
        cy, cx, r = g.integers(0, h), g.integers(0, w), g.integers(2, min(10, max(3, min(h, w) // 3 + 3)))
        d2 = (y - cy) ** 2 + (x - cx) ** 2
        a = np.maximum(a, np.clip(255 - 40 * (d2 - r * r) // max(r, 1), 0, 255))
    return a.astype(np.uint8)


def masked_image(gen, mask, h, w, index=0):
    """(h, w, 4) image: colour of generator `gen`, alpha by mask kind: "none" (255), "blobs", or "noise" (per texel)."""
    import bc45_oracle as B
    img = B.image(gen, h, w, 4, index=index).copy()
    if mask == "none":
        img[..., 3] = 255
    elif mask == "blobs":
        img[..., 3] = alpha_blobs(h, w, index)
    else:
        g = np.random.Generator(np.random.PCG64(T.SEED0 + 9800 + index))
        a = g.integers(0, 256, (h, w), dtype=np.uint8)
        rare = g.integers(0, 8, ((h + 3) // 4, (w + 3) // 4))  # some blocks nearly all transparent or nearly all opaque
        big = np.repeat(np.repeat(rare, 4, axis=0), 4, axis=1)[:h, :w]
        a = np.where(big == 0, np.minimum(a, 140), np.where(big == 1, np.maximum(a, 120), a))
        img[..., 3] = a
    return img
