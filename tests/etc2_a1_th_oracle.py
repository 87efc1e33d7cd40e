"""icamd_encode_etc2_colour_device (include/ic_amd.h) as DEFINED there, restated in numpy and vectorised over
blocks, on top of etc2_a1_oracle (W, the RGB8A1 decoder), etc2_th_oracle (the T / H search of ETC2 RGB8, the packing) and
etc2_colour_oracle (texels, planar choice, decoder):

* ETC2 RGB8A1 with ETC2_COLOUR_PLANAR_TH: by the block's class -- all transparent: W; none transparent: the T / H search of ETC2
  RGB8 against W; 1..15 transparent: the masked search (two partitions of the opaque texels, T(a, b), T(b, a), H(a, b) with the
  paints {0, 1, 3} of the decoder under Op = 0, the H order forced by di's lowest bit, the first smallest error, strictly
  closer than W over the opaque texels);
* ETC2 RGBA8: the EAC alpha word of etc2_oracle, then the ETC2 RGB8 word of the same pixels (planar choice, or planar + T / H).

Holds the fixtures.  Shared by tests/test_etc2_colour_modes_host.py (CPU tier), tests/test_gpu_etc2_colour_modes.py (GPU tier) and
scripts/bench_etc2_colour_modes.py."""
import numpy as np

import etc2_a1_oracle as A
import etc2_colour_oracle as C
import etc2_oracle as E2
import etc2_th_oracle as H
import ic_testlib as T

ETC2_RGBA8, ETC2_RGB8, ETC2_RGB8A1 = E2.ETC2_RGBA8, C.ETC2_RGB8, A.ETC2_RGB8A1
COLOUR_DEFAULT, COLOUR_PLANAR, COLOUR_PLANAR_TH = 0, 1, 2
CLASS_CLEAR, CLASS_OPAQUE, CLASS_MIXED = 1, 2, 3  # the numbering of the definition
PART_L, PART_C = H.PART_L, H.PART_C
KIND_T_AB, KIND_T_BA, KIND_H = H.KIND_T_AB, H.KIND_T_BA, H.KIND_H
NO_ERROR = H.NO_ERROR
# columns of `choice`: the block's class; partition, kind, di of the word that replaced W (-1: the block is W); for an H word 1
# where (C1, C2) = (b, a), 0 where (a, b) (-1 otherwise)
COL_CLASS, COL_PART, COL_KIND, COL_DI, COL_SWAPPED = range(5)


def masked_partitions(rgb, opq):
    """[n, 4, 4, 3] texels, [n, 4, 4] bool opaque -> [2, n, 4, 4] bool: opaque texel in cluster B under partition L and C."""
    v = np.asarray(rgb, np.int64)
    n_o = opq.sum(axis=(1, 2))
    y = v[..., 0] + 2 * v[..., 1] + v[..., 2]
    in_b_l = opq & (n_o[:, None, None] * y > (y * opq).sum(axis=(1, 2))[:, None, None])
    flat, of = v.reshape(-1, 16, 3), opq.reshape(-1, 16)
    mx = np.where(of[..., None], flat, -1).max(axis=1)
    mn = np.where(of[..., None], flat, 256).min(axis=1)
    ch = np.argmax(mx - mn, axis=1)  # (the first largest: R before G before B)
    rows = np.arange(v.shape[0])
    in_b_c = of & (2 * flat[rows, :, ch] > (mx[rows, ch] + mn[rows, ch])[:, None])
    return np.stack([in_b_l, in_b_c.reshape(-1, 4, 4)])


def masked_cluster_colours(rgb, opq, in_b):
    """-> a, b [n, 3] 4-bit codes of clusters A (opaque, outside in_b) and B, and [n] bool: the partition survives."""
    v = np.asarray(rgb, np.int64)
    in_a = opq & ~in_b
    na, nb = in_a.sum(axis=(1, 2)), in_b.sum(axis=(1, 2))
    sa, sb = (v * in_a[..., None]).sum(axis=(1, 2)), (v * in_b[..., None]).sum(axis=(1, 2))
    ok = (na > 0) & (nb > 0)
    qa = (30 * sa + 255 * na[:, None]) // (510 * np.maximum(na, 1)[:, None])
    qb = (30 * sb + 255 * nb[:, None]) // (510 * np.maximum(nb, 1)[:, None])
    ok &= (qa != qb).any(axis=1)
    return qa, qb, ok


def _order_value(c):
    return c[:, 0] << 16 | c[:, 1] << 8 | c[:, 2]


def masked_candidate(kind, a, b, di):
    """The stored colours (c1, c2 [n, 3] codes), [n] bool "stored as (b, a)" and the paints [n, 4, 3] (index 2 unused) of
    candidate `kind` on the codes a, b at distance index di, as the decoder reads them under Op = 0."""
    d = C.DIST[di]
    if kind == KIND_H:
        swapped = (_order_value(a) >= _order_value(b)).astype(np.int64) != (di & 1)
        c1, c2 = np.where(swapped[:, None], b, a), np.where(swapped[:, None], a, b)
        e1, e2 = c1 * 17, c2 * 17
        pts = np.stack([np.clip(e1 + d, 0, 255), np.clip(e1 - d, 0, 255), np.zeros_like(e1), np.clip(e2 - d, 0, 255)], axis=1)
        return c1, c2, swapped, pts
    c1, c2 = (a, b) if kind == KIND_T_AB else (b, a)
    e1, e2 = c1 * 17, c2 * 17
    pts = np.stack([e1, np.clip(e2 + d, 0, 255), np.zeros_like(e1), np.clip(e2 - d, 0, 255)], axis=1)
    return c1, c2, np.zeros(a.shape[0], bool), pts


def masked_nearest(rgb, opq, pts):
    """-> [n, 4, 4] index: the nearest of paints 0, 1, 3 for an opaque texel (ties to the smallest index), 2 for a transparent
    one; and [n] the squared distance summed over the opaque texels."""
    v = np.asarray(rgb, np.int64)
    dist = ((v[:, :, :, None, :] - pts[:, None, None, :, :]) ** 2).sum(axis=-1)
    dist[..., 2] = NO_ERROR
    k = np.where(opq, dist.argmin(axis=-1), 2)
    return k, (dist.min(axis=-1) * opq).sum(axis=(1, 2))


def _clear_bit33(words):
    words = words.copy()
    words[:, 3] &= 0xfd
    return words


def masked_search(rgb, opq):
    """[n, 4, 4, 3] texels and [n, 4, 4] bool opaque of blocks with 1..15 transparent texels -> (words [n, 8] uint8, err [n],
    choice [n, 4]): the best candidate of every block, its error over the opaque texels (NO_ERROR: no surviving partition) and
    its (partition, kind, di, swapped), -1 where there is none."""
    v = np.asarray(rgb, np.int64)
    n = v.shape[0]
    best_err = np.full(n, NO_ERROR, np.int64)
    best_word = np.zeros((n, 8), np.uint8)
    choice = np.full((n, 4), -1, np.int64)
    parts = masked_partitions(v, opq)
    for part in (PART_L, PART_C):
        a, b, ok = masked_cluster_colours(v, opq, parts[part])
        for kind in (KIND_T_AB, KIND_T_BA, KIND_H):
            for di in range(8):
                c1, c2, swapped, pts = masked_candidate(kind, a, b, di)
                k, err = masked_nearest(v, opq, pts)
                better = ok & (err < best_err)  # strictly: a tie stays with the earlier candidate
                if not better.any():
                    continue
                dis = np.full(int(better.sum()), di, np.int64)
                # (pack_h stores the colours as handed where their order already says di & 1: no swap, no index flipped)
                pack = H.pack_h if kind == KIND_H else H.pack_t
                best_word[better] = _clear_bit33(pack(c1[better], c2[better], dis, k[better]))
                best_err[better] = err[better]
                choice[better, 0], choice[better, 1], choice[better, 2] = part, kind, di
                choice[better, 3] = swapped[better] if kind == KIND_H else -1
    return best_word, best_err, choice


def sse_opaque(rgb, opq, words):
    """[n] squared RGB error of the RGB8A1 words over the opaque texels, the words read by the RGB8A1 decoder."""
    dec = A.decode_blocks(words)[..., :3].astype(np.int64)
    return (((np.asarray(rgb, np.int64) - dec) ** 2).sum(axis=-1) * opq).sum(axis=(1, 2))


def block_classes(opq):
    n_o = opq.sum(axis=(1, 2))
    return np.where(n_o == 0, CLASS_CLEAR, np.where(n_o == 16, CLASS_OPAQUE, CLASS_MIXED))


def oracle_encode(img, h, w, swap=0, strategy=T.SMALLER_ERROR, gh=None, gw=None, modes=COLOUR_PLANAR_TH, return_choice=False):
    """Expected bytes of icamd_encode_etc2_colour_device(ICAMD_ETC2_RGB8A1, strategy, modes, 4, ...) for one (h, w, 4) image.
    return_choice: also [n_blocks, 5] (class, partition, kind, di, swapped), the last four -1 where the block is W."""
    gh = h if gh is None else max(gh, h)
    gw = w if gw is None else max(gw, w)
    img = np.ascontiguousarray(np.asarray(img, np.uint8).reshape(h, w, 4))
    base = np.frombuffer(A.oracle_encode(img, h, w, swap, strategy, gh=gh, gw=gw), np.uint8).reshape(-1, 8)
    tex = A.block_texels(img, h, w, gh, gw)
    rgb, opq = tex[..., :3], tex[..., 3] >= 128
    choice = np.full((base.shape[0], 5), -1, np.int64)
    choice[:, COL_CLASS] = block_classes(opq)
    out = base.copy()
    if modes == COLOUR_PLANAR_TH:
        full = choice[:, COL_CLASS] == CLASS_OPAQUE
        if full.any():  # the search of ETC2 RGB8, against this W
            words, err, ch = H.search(rgb[full])
            wins = err < C.sse(rgb[full], C.decode_blocks(base[full]))
            out[full] = np.where(wins[:, None], words, base[full])
            ch[~wins] = -1
            choice[full, COL_PART:COL_SWAPPED] = ch
        mixed = choice[:, COL_CLASS] == CLASS_MIXED
        if mixed.any():
            words, err, ch = masked_search(rgb[mixed], opq[mixed])
            wins = err < sse_opaque(rgb[mixed], opq[mixed], base[mixed])
            out[mixed] = np.where(wins[:, None], words, base[mixed])
            ch[~wins] = -1
            choice[mixed, COL_PART:] = ch
    else:
        assert modes in (COLOUR_DEFAULT, COLOUR_PLANAR)  # both are icamd_encode_device
    return (out.tobytes(), choice) if return_choice else out.tobytes()


def changed(choice):
    return choice[:, COL_PART] >= 0


def oracle_encode_rgba8(img, h, w, swap=0, strategy=T.SMALLER_ERROR, gh=None, gw=None, modes=COLOUR_PLANAR_TH, alpha_words=None):
    """Expected bytes of icamd_encode_etc2_colour_device(ICAMD_ETC2_RGBA8, strategy, modes, 4, ...): etc2_oracle's alpha word,
    then the ETC1 word (DEFAULT), the ETC2 RGB8 word (PLANAR) or the ETC2 RGB8 word with T / H (PLANAR_TH) of the same pixels."""
    gh = h if gh is None else max(gh, h)
    gw = w if gw is None else max(gw, w)
    img = np.ascontiguousarray(np.asarray(img, np.uint8).reshape(h, w, 4))
    if modes == COLOUR_DEFAULT:
        return E2.oracle_encode(img, h, w, swap, strategy, gh=gh, gw=gw, alpha_words=alpha_words)
    if modes == COLOUR_PLANAR:
        colour = C.oracle_encode(img, h, w, 4, swap, strategy, gh=gh, gw=gw)
    else:
        colour = H.oracle_encode(img, h, w, 4, swap, strategy, gh=gh, gw=gw)
    alpha = E2.eac_encode(E2.block_alphas(img[..., 3], h, w, gh, gw)) if alpha_words is None else alpha_words
    return np.concatenate([alpha, np.frombuffer(colour, np.uint8).reshape(-1, 8)], axis=1).tobytes()


def oracle_decode_rgba8(blocks, h, w, swap=0):
    """Expected RGBA8 rows of ETC2 RGBA8 blocks whose colour words may be of any mode."""
    b = np.frombuffer(bytes(blocks), np.uint8).reshape(-1, 16)
    rows, cols = (h + 3) // 4, (w + 3) // 4
    rgb = C.oracle_decode(b[:, 8:].tobytes(), h, w).reshape(h, w, 3)
    a = E2.eac_decode(b[:, :8]).reshape(rows, cols, 4, 4)  # [brow, bcol, x, y]
    out = np.empty((h, w, 4), np.uint8)
    out[..., :3] = rgb[..., ::-1] if swap else rgb
    out[..., 3] = a.transpose(0, 3, 1, 2).reshape(rows * 4, cols * 4)[:h, :w]
    return out.reshape(-1)


# ---- inputs: colour from etc2_th_oracle.edges / mixed, alpha from the masks below

def alpha_edge(h, w, offset=22):
    """A straight vertical cut: transparent left of column `offset` (not a multiple of 4: it runs through a block column)."""
    assert offset % 4
    a = np.full((h, w), 255, np.uint8)
    a[:, :offset] = 0
    return a


def alpha_noise(h, w, seed=0):
    g = np.random.Generator(np.random.PCG64(T.SEED0 + 9900 + seed))
    return g.integers(0, 256, (h, w), dtype=np.uint8)


def with_alpha(rgb, alpha):
    out = np.empty(rgb.shape[:2] + (4,), np.uint8)
    out[..., :3] = rgb[..., :3]
    out[..., 3] = alpha
    return out


def edges_cut(noise=6, h=64, w=64, offset=22):
    return with_alpha(H.edges(noise, h, w), alpha_edge(h, w, offset))


def edges_blobs(noise=6, h=64, w=64, index=0):
    return with_alpha(H.edges(noise, h, w), A.alpha_blobs(h, w, index))


def edges_noise(noise=6, h=64, w=64, seed=0):
    return with_alpha(H.edges(noise, h, w), alpha_noise(h, w, seed))


def mixed():
    """64 x 64: the colours of etc2_th_oracle.mixed (columns 0..15 gradient, 16..31 flat, 32..63 edges) under per-texel noise
    alpha that is forced by column band -- 0..7 opaque, 8..23 noise, 24..31 transparent, 32..47 opaque, 48..63 noise -- so that
    every wave of 16 x 4 blocks holds blocks of every class, changed and kept."""
    a = alpha_noise(64, 64, 1)
    a[:, 0:8] = 255
    a[:, 24:32] = 0
    a[:, 32:48] = 255
    return with_alpha(H.mixed(), a)


WAVE_KINDS = ("clear", "opaque_changed", "opaque_kept", "mixed_changed", "mixed_kept")


def wave_kinds(img, strategy=T.SMALLER_ERROR):
    """Per wave of the 64 x 64 tile (16 x 4 blocks each, the block-to-lane mapping of etc2_th_oracle.wave_kinds): the numbers of
    blocks of class 1, class 2 changed / kept, class 3 changed / kept."""
    _, choice = oracle_encode(img, 64, 64, 0, strategy, return_choice=True)
    cls, ch = choice[:, COL_CLASS], changed(choice)
    kinds = [cls == CLASS_CLEAR, (cls == CLASS_OPAQUE) & ch, (cls == CLASS_OPAQUE) & ~ch, (cls == CLASS_MIXED) & ch,
             (cls == CLASS_MIXED) & ~ch]
    return [tuple(int(k[64 * i:64 * i + 64].sum()) for k in kinds) for i in range(4)]
