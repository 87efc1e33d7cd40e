"""BC7 (BPTC, include/ic_amd.h ICAMD_BC7): the decoder of all eight modes restated from the BPTC specification in plain Python,
and the mode-6 encoder's DEFINITION (include/ic_amd.h, steps 1-6) restated in numpy.  The kernels (csrc/bc7_block.h) and their
host twin are bit-exact against this file.  The partition / anchor tables are read from csrc/bc7_partition_tables.inc (data only);
tests/test_bc7_host.py checks every entry of them against an independent decoder."""
import os
import re

import numpy as np

BC7 = 32
HERE = os.path.dirname(os.path.abspath(__file__))
TABLES_INC = os.path.join(os.path.dirname(HERE), "image-compression_amd", "csrc", "bc7_partition_tables.inc")

WEIGHTS = {2: (0, 21, 43, 64), 3: (0, 9, 18, 27, 37, 46, 55, 64),
           4: (0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64)}
# per mode: subsets, partition bits, rotation bits, index-selection bits, colour bits, alpha bits, unique p-bits (per endpoint),
# shared p-bits (per subset), index bits, secondary index bits
MODES = ((3, 4, 0, 0, 4, 0, 1, 0, 3, 0), (2, 6, 0, 0, 6, 0, 0, 1, 3, 0), (3, 6, 0, 0, 5, 0, 0, 0, 2, 0),
         (2, 6, 0, 0, 7, 0, 1, 0, 2, 0), (1, 0, 2, 1, 5, 6, 0, 0, 2, 3), (1, 0, 2, 0, 7, 8, 0, 0, 2, 2),
         (1, 0, 0, 0, 7, 7, 1, 0, 4, 0), (2, 6, 0, 0, 5, 5, 1, 0, 2, 0))


def _tables():
    text = open(TABLES_INC).read()
    out = {}
    for name in ("P2", "P3", "A2", "A3A", "A3B"):
        body = re.search(r"#ifdef ICAMD_BC7_TABLE_%s\n(.*?)#endif" % name, text, re.S).group(1)
        vals = [int(v) for v in re.findall(r"\d+", body)]
        out[name] = np.array(vals).reshape(64, 16) if name[0] == "P" else np.array(vals)
        assert out[name].shape[0] == 64
    return out


TABLES = _tables()
P2, P3, A2, A3A, A3B = (TABLES[k] for k in ("P2", "P3", "A2", "A3A", "A3B"))


def subset_of(ns, part, i):
    return 0 if ns == 1 else int(P2[part][i]) if ns == 2 else int(P3[part][i])


def anchors(ns, part):
    return (0,) if ns == 1 else (0, int(A2[part])) if ns == 2 else (0, int(A3A[part]), int(A3B[part]))


def decode_block(block):
    """16 bytes -> [16, 4] uint8 (texel i = 4 y + x; R, G, B, A)."""
    v = int.from_bytes(bytes(block), "little")
    out = np.zeros((16, 4), np.uint8)
    if v & 0xff == 0:
        return out  # reserved: sixteen (0, 0, 0, 0) texels
    mode = (v & 0xff & -(v & 0xff)).bit_length() - 1
    pos = [mode + 1]

    def take(n):
        r = (v >> pos[0]) & ((1 << n) - 1)
        pos[0] += n
        return r

    ns, pb, rb, isb, cb, ab, epb, spb, ib, ib2 = MODES[mode]
    part, rot, sel = take(pb), take(rb), take(isb)
    ne = 2 * ns
    ep = [[0, 0, 0, 255] for _ in range(ne)]
    for c in range(3):
        for e in range(ne):
            ep[e][c] = take(cb)
    if ab:
        for e in range(ne):
            ep[e][3] = take(ab)
    if epb:
        pbits = [take(1) for _ in range(ne)]
    elif spb:
        shared = [take(1) for _ in range(ns)]
        pbits = [shared[e // 2] for e in range(ne)]
    else:
        pbits = None
    for e in range(ne):
        for c in range(4 if ab else 3):
            bits = ab if c == 3 else cb
            x = ep[e][c]
            if pbits is not None:
                x, bits = x << 1 | pbits[e], bits + 1
            x <<= 8 - bits
            ep[e][c] = x | x >> bits
    anc = anchors(ns, part)
    idx1 = [take(ib - 1 if i in anc else ib) for i in range(16)]
    idx2 = [take(ib2 - 1 if i == 0 else ib2) for i in range(16)] if ib2 else idx1
    for i in range(16):
        s = subset_of(ns, part, i)
        e0, e1 = ep[2 * s], ep[2 * s + 1]
        ci, cbits, ai, abits = idx1[i], ib, idx2[i], ib2 or ib
        if sel:
            ci, cbits, ai, abits = ai, abits, ci, cbits
        wc, wa = WEIGHTS[cbits][ci], WEIGHTS[abits][ai]
        px = [((64 - wc) * e0[c] + wc * e1[c] + 32) >> 6 for c in range(3)] + [((64 - wa) * e0[3] + wa * e1[3] + 32) >> 6]
        if rot:
            px[rot - 1], px[3] = px[3], px[rot - 1]
        out[i] = px
    return out


def decode_blocks(blocks):
    b = np.frombuffer(bytes(blocks), np.uint8).reshape(-1, 16)
    return np.stack([decode_block(r) for r in b]) if len(b) else np.zeros((0, 16, 4), np.uint8)


def decode(blocks, h, w, pad=0, swap=False):
    """Block stream of an h x w image (raster block order) -> [h, w * 4 + pad] uint8 rows of RGBA8; padding bytes are zero."""
    rows, cols = (h + 3) // 4, (w + 3) // 4
    t = decode_blocks(blocks).reshape(rows, cols, 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(rows * 4, cols * 4, 4)[:h, :w]
    if swap:
        t = t[..., [2, 1, 0, 3]]
    out = np.zeros((h, w * 4 + pad), np.uint8)
    out[:, :w * 4] = t.reshape(h, w * 4)
    return out


def encoded_size(h, w):
    return ((h + 3) // 4) * ((w + 3) // 4) * 16


# ---- the encoder's definition

def block_texels(img, gh=None, gw=None, swap=False):
    """[h, w, 3 or 4] uint8 -> [rows * cols, 16, 4] int64 texels (R, G, B, A) of the grid max(h, gh) x max(w, gw): clamp-to-edge
    replication, A = 255 for 3-component sources, R and B exchanged with swap."""
    h, w, comps = img.shape
    rows, cols = (max(h, gh or h) + 3) // 4, (max(w, gw or w) + 3) // 4
    ys = np.minimum(np.arange(rows * 4), h - 1)
    xs = np.minimum(np.arange(cols * 4), w - 1)
    px = img[ys][:, xs].astype(np.int64)
    if comps == 3:
        px = np.concatenate([px, np.full(px.shape[:2] + (1,), 255, np.int64)], axis=2)
    if swap:
        px = px[..., [2, 1, 0, 3]]
    return px.reshape(rows, 4, cols, 4, 4).transpose(0, 2, 1, 3, 4).reshape(rows * cols, 16, 4)


def targets(v):
    """Step 1: (T0, T1), [N, 4] each."""
    lo, hi = v.min(axis=1), v.max(axis=1)
    cs = np.argmax(hi - lo, axis=1)  # the first maximum: ties R before G before B before A
    n = np.arange(len(v))
    star = v[n, :, cs]
    cov = 16 * (star[:, :, None] * v).sum(axis=1) - star.sum(axis=1)[:, None] * v.sum(axis=1)
    flip = cov < 0
    flip[n, cs] = False
    return np.where(flip, hi, lo), np.where(flip, lo, hi)


def quantise(t):
    """Step 2: [N, 4] targets -> [N, 4] endpoint values 2 q + p, p shared by the four channels."""
    cand, err = [], []
    for p in (0, 1):
        q = np.clip((t - p + 1) >> 1, 0, 127)
        e = 2 * q + p
        cand.append(e)
        err.append(((e - t) ** 2).sum(axis=1))
    return np.where((err[1] < err[0])[:, None], cand[1], cand[0])


W4 = np.array(WEIGHTS[4], np.int64)


def indices(v, e0, e1):
    """Step 3: (k [N, 16], sse [N])."""
    pal = ((64 - W4)[None, :, None] * e0[:, None, :] + W4[None, :, None] * e1[:, None, :] + 32) >> 6  # [N, 16 k, 4]
    d = ((pal[:, None, :, :] - v[:, :, None, :]) ** 2).sum(axis=3)  # [N, 16 p, 16 k]
    k = d.argmin(axis=2)
    return k, d.min(axis=2).sum(axis=1)


def rdiv(n, d):
    return (2 * n + d) // (2 * d)


def refit_targets(v, k):
    """Step 4: (T0', T1', has_refit) from the indices k."""
    w = W4[k]  # [N, 16]
    a, b, c = ((64 - w) ** 2).sum(axis=1), ((64 - w) * w).sum(axis=1), (w * w).sum(axis=1)
    x, y = ((64 - w)[:, :, None] * v).sum(axis=1), (w[:, :, None] * v).sum(axis=1)
    det = a * c - b * b
    ok = det != 0
    d = np.where(ok, det, 1)[:, None]
    t0 = np.clip(rdiv(64 * (c[:, None] * x - b[:, None] * y), d), 0, 255)
    t1 = np.clip(rdiv(64 * (a[:, None] * y - b[:, None] * x), d), 0, 255)
    return t0, t1, ok


def encode_texels(v, stages=False):
    """[N, 16, 4] int64 texels -> [N, 16] uint8 blocks (steps 1-6).  stages: also (sse of the first pass, final sse, refit taken)."""
    t0, t1 = targets(v)
    e0, e1 = quantise(t0), quantise(t1)
    k, sse = indices(v, e0, e1)
    r0, r1, ok = refit_targets(v, k)
    f0, f1 = quantise(r0), quantise(r1)
    k2, sse2 = indices(v, f0, f1)
    take = ok & (sse2 < sse)
    e0, e1 = np.where(take[:, None], f0, e0), np.where(take[:, None], f1, e1)
    k = np.where(take[:, None], k2, k)
    final = np.where(take, sse2, sse)
    flip = k[:, 0] >= 8  # step 5
    e0, e1 = np.where(flip[:, None], e1, e0), np.where(flip[:, None], e0, e1)
    k = np.where(flip[:, None], 15 - k, k)
    out = []
    for n in range(len(v)):  # step 6
        bits, pos = 1 << 6, 7
        for c in range(4):
            for e in (e0, e1):
                bits |= (int(e[n, c]) >> 1) << pos
                pos += 7
        for e in (e0, e1):
            bits |= (int(e[n, 0]) & 1) << pos
            pos += 1
        bits |= int(k[n, 0]) << pos
        pos += 3
        for p in range(1, 16):
            bits |= int(k[n, p]) << pos
            pos += 4
        assert pos == 128
        out.append(np.frombuffer(bits.to_bytes(16, "little"), np.uint8))
    blocks = np.stack(out) if out else np.zeros((0, 16), np.uint8)
    return (blocks, sse, final, take) if stages else blocks


def oracle_encode(img, gh=None, gw=None, swap=False):
    """[h, w, 3 or 4] uint8 image -> the block stream (bytes) of the grid max(h, gh) x max(w, gw)."""
    return encode_texels(block_texels(img, gh, gw, swap)).tobytes()


def sse_of(img, blocks):
    """Summed RGBA squared error of a BC7 block stream against the image ([h, w, 3 or 4]; A = 255 for 3 components)."""
    h, w, comps = img.shape
    dec = decode(blocks, h, w).reshape(h, w, 4).astype(np.int64)
    src = img.astype(np.int64)
    if comps == 3:
        src = np.concatenate([src, np.full((h, w, 1), 255, np.int64)], axis=2)
    return int(((dec - src) ** 2).sum())


# ---- test images (integer-only generators: every machine gets the same bytes)

CONTENTS = ("noise", "smooth", "ramp", "flat", "two_colour", "varying_alpha")


def content(name, h, w, comps, seed=0):
    """[h, w, comps] uint8, comps 3 or 4."""
    g = np.random.Generator(np.random.PCG64(0xBC7000 + 977 * seed + 31 * h + w))
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    img = np.empty((h, w, 4), np.int64)
    if name == "noise":
        img[...] = g.integers(0, 256, (h, w, 4))
    elif name == "smooth":  # low-frequency waves + 3 bits of noise, opaque but for an alpha that follows the waves
        n = g.integers(0, 8, (h, w))
        def tri(t, p):  # integer triangle wave 0..p
            return np.abs(t % (2 * p) - p)
        img[..., 0] = 28 + 200 * tri(2 * x + y, 64) // 64 + n
        img[..., 1] = 28 + 200 * tri(x + 3 * y + 20, 96) // 96 + n
        img[..., 2] = 28 + 200 * tri(3 * x - y + 500, 80) // 80 + n
        img[..., 3] = 150 + 100 * tri(x + y, 48) // 48
    elif name == "ramp":
        img[..., 0] = 255 * x // max(w - 1, 1)
        img[..., 1] = 255 * y // max(h - 1, 1)
        img[..., 2] = 255 * (x + y) // max(w + h - 2, 1)
        img[..., 3] = 255 - 255 * x // max(w - 1, 1)
    elif name == "flat":  # 8 x 8 tiles of one colour: flat blocks
        t = g.integers(0, 256, ((h + 7) // 8, (w + 7) // 8, 4))
        img[...] = t.repeat(8, 0).repeat(8, 1)[:h, :w]
    elif name == "two_colour":  # per 8 x 8 tile two colours dealt out at random
        t = g.integers(0, 256, ((h + 7) // 8, (w + 7) // 8, 2, 4))
        pick = g.integers(0, 2, (h, w))
        both = t.repeat(8, 0).repeat(8, 1)[:h, :w]
        img[...] = np.where(pick[..., None] == 0, both[:, :, 0], both[:, :, 1])
    elif name == "varying_alpha":  # calm colour, alpha over its whole range: c* = A in most blocks
        img[..., :3] = 90 + g.integers(0, 6, (h, w, 3))
        img[..., 3] = g.integers(0, 256, (h, w))
    else:
        raise ValueError(name)
    return np.clip(img, 0, 255).astype(np.uint8)[..., :comps].copy()


def mixed_wave_image():
    """256 x 256 RGBA8: every 4 x 4 block of a 64-block row segment (one wave of the wide kernel) is dealt one of five kinds --
    flat, opaque noise, translucent noise, a descending ramp (texel 0 the brightest: the anchor flips), an outlier block (the
    refit is taken) -- so the lanes of every wave disagree at every branch of the encoder."""
    g = np.random.Generator(np.random.PCG64(0xBC7256))
    kinds = g.integers(0, 5, (64, 64))
    img = np.zeros((256, 256, 4), np.uint8)
    i = np.arange(16).reshape(4, 4)
    for by in range(64):
        for bx in range(64):
            k = kinds[by, bx]
            if k == 0:
                b = np.broadcast_to(g.integers(0, 256, 4), (4, 4, 4))
            elif k == 1:
                b = np.concatenate([g.integers(0, 256, (4, 4, 3)), np.full((4, 4, 1), 255)], axis=2)
            elif k == 2:
                b = g.integers(0, 256, (4, 4, 4))
            elif k == 3:
                b = np.stack([240 - 16 * i] * 3 + [np.full((4, 4), 255)], axis=2)
            else:
                b = np.stack([100 + 2 * i] * 3 + [np.full((4, 4), 255)], axis=2)
                b[1, 1, :3] = 255
            img[4 * by:4 * by + 4, 4 * bx:4 * bx + 4] = b
    return img, kinds


# ---- random blocks for the decoder tests

def random_block(g, mode, partition=None, rotation=None, sel=None, ones=False):
    """A block of `mode` (8: reserved): the named fields fixed, every other bit random (or all ones)."""
    v = (1 << 128) - 1 if ones else int.from_bytes(g.integers(0, 256, 16, dtype=np.uint8).tobytes(), "little")
    if mode == 8:
        return ((v >> 8) << 8).to_bytes(16, "little")
    v = (v >> (mode + 1) << (mode + 1)) | 1 << mode
    pos = mode + 1
    for bits, val in ((MODES[mode][1], partition), (MODES[mode][2], rotation), (MODES[mode][3], sel)):
        if bits and val is not None:
            v = (v & ~(((1 << bits) - 1) << pos)) | val << pos
        pos += bits
    return v.to_bytes(16, "little")


def stratified_blocks(n, seed):
    """n blocks cycling over the eight modes and the reserved form, fields random."""
    g = np.random.Generator(np.random.PCG64(seed))
    return b"".join(random_block(g, i % 9) for i in range(n))
