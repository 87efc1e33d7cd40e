"""BC1 with punch-through alpha and BC2 (include/ic_amd.h, ICAMD_BC1A / ICAMD_BC2) as STATED there, restated in plain numpy and
vectorised over blocks: both decoders as the formats define them, the BC1A encoder (all-transparent word, the DXT1 bytes, the
masked three-colour search), the BC2 encoder (sixteen roundings + the DXT5 colour block) and the four-channel metric.  The opaque
BC1A path and BC2's colour half come from the DXT oracle (ic_testlib.oracle_encode).

Shared by tests/test_bc1a_bc2_host.py (CPU tier), tests/test_gpu_bc1a_bc2.py (GPU tier), tests/golden/make_bc1a_bc2_golden.py and
scripts/bench_bc1a_bc2.py."""
import os

import numpy as np

import etc2_a1_oracle as A  # alpha_blobs, masked_image: the cut-out inputs of ICAMD_ETC2_RGB8A1
import ic_testlib as T

BC1A, BC2 = 36, 37
BLOCK_BYTES = {BC1A: 8, BC2: 16}
ALL_TRANSPARENT = bytes.fromhex("00000000ffffffff")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bc1a_bc2_decode_kat.bin")
MASKS = ("none", "blobs", "noise", "one")


def example_images():
    """The two worked examples of the header as (4, 4, 4) images; their blocks and decoded texels are literals in the tests."""
    a = np.zeros((4, 4, 4), np.uint8)
    a[..., :3] = (100, 150, 200)
    a[:, :2, 3] = 255
    b = np.zeros((4, 4, 4), np.uint8)
    b[...] = (200, 100, 50, 255)
    b[0, 0] = (10, 20, 30, 255)
    b[1, 1] = (105, 60, 40, 200)
    b[3, 3, 3] = 127
    return a, b


def encoded_size(codec, gh, gw):
    return ((gh + 3) // 4) * ((gw + 3) // 4) * BLOCK_BYTES[codec]


def _as_blocks(blocks, size):
    if isinstance(blocks, np.ndarray):
        return np.ascontiguousarray(blocks, np.uint8).reshape(-1, size)
    return np.frombuffer(bytes(blocks), np.uint8).reshape(-1, size)


def quantize8(v, maximum):
    i = np.asarray(v, np.int64) * maximum + 128
    return (i + (i >> 8)) >> 8


def quantize565(rgb):
    """[..., 3] canonical R, G, B -> packed 565."""
    rgb = np.asarray(rgb, np.int64)
    return quantize8(rgb[..., 0], 31) << 11 | quantize8(rgb[..., 1], 63) << 5 | quantize8(rgb[..., 2], 31)


def expand565(c):
    """[n] packed 565 -> [n, 3] R, G, B by bit replication."""
    c = np.asarray(c, np.int64)
    r, g, b = c >> 11, (c >> 5) & 63, c & 31
    return np.stack([r << 3 | r >> 2, g << 2 | g >> 4, b << 3 | b >> 2], axis=-1)


def colour_words(b8):
    """[n, 8] colour-block bytes -> (c0, c1, [n, 16] indices, texel p = 4 y + x)."""
    b8 = b8.astype(np.int64)
    c0, c1 = b8[:, 0] | b8[:, 1] << 8, b8[:, 2] | b8[:, 3] << 8
    bits = b8[:, 4] | b8[:, 5] << 8 | b8[:, 6] << 16 | b8[:, 7] << 24
    idx = (bits[:, None] >> (2 * np.arange(16))[None]) & 3
    return c0, c1, idx


def _palette(c0, c1, four):
    """[n, 4, 4] RGBA palettes: `four` [n] bool picks the four-colour rule, the others get (E0 + E1) / 2 and a clear index 3."""
    e0, e1 = expand565(c0), expand565(c1)
    n = e0.shape[0]
    pal = np.zeros((n, 4, 4), np.int64)
    pal[:, 0, :3], pal[:, 1, :3] = e0, e1
    pal[:, 2, :3] = np.where(four[:, None], (2 * e0 + e1) // 3, (e0 + e1) // 2)
    pal[:, 3, :3] = np.where(four[:, None], (e0 + 2 * e1) // 3, 0)
    pal[:, :3, 3] = 255
    pal[:, 3, 3] = np.where(four, 255, 0)
    return pal


def decode_bc1a_blocks(blocks):
    """Any 8-byte BC1 blocks -> [n, 4(y), 4(x), 4] uint8 RGBA texels, as the format defines them."""
    c0, c1, idx = colour_words(_as_blocks(blocks, 8))
    pal = _palette(c0, c1, c0 > c1)
    return pal[np.arange(pal.shape[0])[:, None], idx].reshape(-1, 4, 4, 4).astype(np.uint8)


def decode_bc2_blocks(blocks):
    """Any 16-byte BC2 blocks -> [n, 4, 4, 4] uint8 RGBA texels: always four colours, alpha = nibble x 17."""
    b = _as_blocks(blocks, 16)
    c0, c1, idx = colour_words(b[:, 8:])
    pal = _palette(c0, c1, np.ones(c0.shape[0], bool))
    out = pal[np.arange(pal.shape[0])[:, None], idx]
    a = b[:, :8].astype(np.int64)
    nib = np.stack([a[:, p >> 1] >> (4 * (p & 1)) & 15 for p in range(16)], axis=1)
    out[..., 3] = nib * 17
    return out.reshape(-1, 4, 4, 4).astype(np.uint8)


def decode_blocks(codec, blocks):
    return decode_bc1a_blocks(blocks) if codec == BC1A else decode_bc2_blocks(blocks)


def oracle_decode(codec, blocks, h, w, swap=0, pad=0):
    """Expected RGBA8 rows (h rows of 4 w + pad bytes, the pad bytes zero); swap: stored R goes to the third byte."""
    rows, cols = (h + 3) // 4, (w + 3) // 4
    tex = decode_blocks(codec, blocks).reshape(rows, cols, 4, 4, 4)
    img = tex.transpose(0, 2, 1, 3, 4).reshape(rows * 4, cols * 4, 4)[:h, :w]
    if swap:
        img = img[..., [2, 1, 0, 3]]
    out = np.zeros((h, w * 4 + pad), np.uint8)
    out[:, :w * 4] = img.reshape(h, w * 4)
    return out.reshape(-1)


# ---- encoders

def block_texels(img, h, w, gh, gw, swap=0):
    """[n_blocks, 16, 4] canonical RGBA texels (p = 4 y + x) of the block grid max(h, gh) x max(w, gw), clamp-to-edge."""
    tex = A.block_texels(img, h, w, gh, gw).reshape(-1, 16, 4)
    return tex[..., [2, 1, 0, 3]] if swap else tex


def encode_masked(tex):
    """Case 3 of the definition on [m, 16, 4] canonical texels with 1..15 transparent ones -> [m, 8] uint8."""
    tex = np.asarray(tex, np.int64)
    m = tex.shape[0]
    opq = tex[:, :, 3] >= 128
    lum = 4 * tex[:, :, 0] + 8 * tex[:, :, 1] + tex[:, :, 2]
    lo = np.argmin(np.where(opq, lum, 1 << 30), axis=1)   # (argmin / argmax: the first in raster order)
    hi = np.argmax(np.where(opq, lum, -1), axis=1)
    a, b = quantize565(tex[np.arange(m), lo, :3]), quantize565(tex[np.arange(m), hi, :3])
    c0, c1 = np.minimum(a, b), np.maximum(a, b)
    e0, e1 = expand565(c0), expand565(c1)
    pal = np.stack([e0, e1, (e0 + e1) >> 1], axis=1)
    dist = ((tex[:, :, None, :3] - pal[:, None]) ** 2).sum(axis=-1)
    idx = np.where(opq, dist.argmin(axis=2), 3)
    bits = (idx << (2 * np.arange(16))[None]).sum(axis=1)
    out = np.zeros((m, 8), np.uint8)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = c0 & 255, c0 >> 8, c1 & 255, c1 >> 8
    for k in range(4):
        out[:, 4 + k] = (bits >> (8 * k)) & 255
    return out


def research_error(tex, blocks):
    """Per block: (error of the stored indices, error after re-searching the indices over the decoded palette), both the squared
    RGB distance summed over the opaque texels; transparent texels stay index 3."""
    tex = np.asarray(tex, np.int64)
    c0, c1, idx = colour_words(_as_blocks(blocks, 8))
    pal = _palette(c0, c1, c0 > c1)[..., :3]
    opq = tex[:, :, 3] >= 128
    dist = ((tex[:, :, None, :3] - pal[:, None]) ** 2).sum(axis=-1)        # [n, 16, 4]
    stored = np.take_along_axis(dist, idx[..., None], axis=2)[..., 0]
    allowed = np.where((c0 > c1)[:, None, None], dist, np.where(np.arange(4)[None, None] < 3, dist, 1 << 40))
    return (stored * opq).sum(axis=1), (allowed.min(axis=2) * opq).sum(axis=1)


def bc2_alpha_words(tex):
    """[n, 16, 4] texels -> [n, 8] uint8: nibble p = Quantize8(alpha_p, 15)."""
    nib = quantize8(tex[:, :, 3], 15)
    return (nib[:, 0::2] | nib[:, 1::2] << 4).astype(np.uint8)


def oracle_encode(codec, img, h, w, swap=0, gh=None, gw=None, return_classes=False):
    """Expected bytes of one (h, w, 4) image.  return_classes (BC1A): also [n_blocks] 0 all-transparent, 1 mixed, 2 opaque."""
    gh = h if gh is None else max(gh, h)
    gw = w if gw is None else max(gw, w)
    img = np.ascontiguousarray(np.asarray(img, np.uint8).reshape(h, w, 4))
    tex = block_texels(img, h, w, gh, gw, swap)
    if codec == BC2:
        dxt5 = np.frombuffer(T.oracle_encode(T.DXT5, img, h, w, 4, swap, gh=gh, gw=gw), np.uint8).reshape(-1, 16)
        return np.concatenate([bc2_alpha_words(tex), dxt5[:, 8:]], axis=1).tobytes()
    n_opq = (tex[:, :, 3] >= 128).sum(axis=1)
    out = np.zeros((tex.shape[0], 8), np.uint8)
    out[n_opq == 0] = np.frombuffer(ALL_TRANSPARENT, np.uint8)
    full = n_opq == 16
    if full.any():
        dxt1 = np.frombuffer(T.oracle_encode(T.DXT1, img, h, w, 4, swap, gh=gh, gw=gw), np.uint8).reshape(-1, 8)
        out[full] = dxt1[full]
    mixed = (n_opq > 0) & (n_opq < 16)
    if mixed.any():
        out[mixed] = encode_masked(tex[mixed])
    if return_classes:
        return out.tobytes(), np.where(full, 2, np.where(mixed, 1, 0))
    return out.tobytes()


def class_shares(img, h, w):
    """(all-transparent, mixed, opaque) shares of the image's own blocks."""
    n_opq = (block_texels(img, h, w, h, w)[:, :, 3] >= 128).sum(axis=1)
    n = float(n_opq.size)
    return (n_opq == 0).sum() / n, ((n_opq > 0) & (n_opq < 16)).sum() / n, (n_opq == 16).sum() / n


# ---- metric

def metric(codec, img, blocks, h, w, swap=0, gw=None):
    """(sse[4], max_abs[4]) of the blocks (laid out for a grid gw wide) against the image's own pixels, channels in memory order."""
    gw = w if gw is None else max(gw, w)
    rows, cols, gcols = (h + 3) // 4, (w + 3) // 4, (gw + 3) // 4
    b = _as_blocks(blocks, BLOCK_BYTES[codec]).reshape(-1, gcols, BLOCK_BYTES[codec])[:rows, :cols]
    dec = oracle_decode(codec, np.ascontiguousarray(b), h, w, swap).reshape(h, w, 4).astype(np.int64)
    d = np.asarray(img, np.uint8).reshape(h, w, 4).astype(np.int64) - dec
    return (d * d).sum(axis=(0, 1)), np.abs(d).max(axis=(0, 1))


# ---- inputs

def masked_image(gen, mask, h, w, index=0):
    """(h, w, 4) image: colour of generator `gen`, alpha by mask kind: "none" (255), "blobs", "noise" (etc2_a1_oracle), or "one":
    exactly one transparent texel in the image."""
    if mask != "one":
        return A.masked_image(gen, mask, h, w, index)
    img = A.masked_image(gen, "none", h, w, index)
    g = np.random.Generator(np.random.PCG64(T.SEED0 + 9900 + index))
    img[g.integers(0, h), g.integers(0, w), 3] = g.integers(0, 128)
    return img


def blob_fixture():
    """The 64 x 64 cut-out image whose blocks hold all three classes (class_shares: each at least 5 %)."""
    return masked_image("mixed", "blobs", 64, 64, index=1)


def random_masked_blocks(n, seed):
    """[n, 16, 4] canonical texels around a base colour, alpha uniform with texel 0 transparent and texel 1 opaque."""
    g = np.random.default_rng(seed)
    base = g.integers(0, 256, (n, 1, 3))
    spread = g.integers(0, 41, (n, 1, 1))
    rgb = np.clip(base + g.integers(-40, 41, (n, 16, 3)) * spread // 40, 0, 255)
    al = g.integers(0, 256, (n, 16, 1))
    al[:, 0], al[:, 1] = 0, 255
    return np.concatenate([rgb, al], axis=2).astype(np.int64)


def random_bc1_blocks(n, seed):
    """[n, 8] uint8: random blocks, a quarter each left as drawn, forced to c0 == c1, to c0 < c1 and to c0 > c1; the forced
    c0 < c1 blocks start with the sixteen-texel index pattern 0, 1, 2, 3, ... so every index occurs."""
    g = np.random.default_rng(seed)
    b = g.integers(0, 256, (n, 8), dtype=np.uint8)
    c = b[:, :4].astype(np.int64)
    c0, c1 = c[:, 0] | c[:, 1] << 8, c[:, 2] | c[:, 3] << 8
    kind = np.arange(n) % 4
    lo, hi = np.minimum(c0, c1), np.maximum(c0, c1)
    hi = np.where(hi == lo, np.where(lo == 0xffff, lo, lo + 1), hi)
    lo = np.where(hi == lo, lo - 1, lo)
    n0 = np.where(kind == 1, c0, np.where(kind == 2, lo, np.where(kind == 3, hi, c0)))
    n1 = np.where(kind == 1, c0, np.where(kind == 2, hi, np.where(kind == 3, lo, c1)))
    b[:, 0], b[:, 1], b[:, 2], b[:, 3] = n0 & 255, n0 >> 8, n1 & 255, n1 >> 8
    b[kind == 2, 4] = 0xe4
    return b


def random_bc2_blocks(n, seed):
    """[n, 16] uint8: random alpha words, random colour words (half of them with c0 <= c1)."""
    g = np.random.default_rng(seed)
    return np.concatenate([g.integers(0, 256, (n, 8), dtype=np.uint8), random_bc1_blocks(n, seed + 1)], axis=1)


def load_golden():
    """The committed fixture: (bc1 blocks [n, 8], their 64 decoded bytes [n, 64], bc2 blocks [m, 16], their decoded [m, 64])."""
    raw = np.fromfile(GOLDEN, np.uint8)
    assert bytes(raw[:8]) == b"BC1A2KAT"
    n, m = int(raw[8:12].view("<u4")[0]), int(raw[12:16].view("<u4")[0])
    p = 16
    bc1 = raw[p:p + 8 * n].reshape(n, 8); p += 8 * n
    dec1 = raw[p:p + 64 * n].reshape(n, 64); p += 64 * n
    bc2 = raw[p:p + 16 * m].reshape(m, 16); p += 16 * m
    dec2 = raw[p:p + 64 * m].reshape(m, 64); p += 64 * m
    assert p == raw.size
    return bc1, dec1, bc2, dec2
