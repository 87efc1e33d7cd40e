"""BC7 with the opt-in mode-1 / mode-5 candidates (include/ic_amd.h ICAMD_BC7_MODES_EXTENDED): the definition
restated in numpy.  The mode-6 block and its sse are bc7_oracle's, unchanged; this file adds the sub-fit F, the partition rule,
the two candidates and the choice.  The kernels (csrc/bc7_modes_block.h) and their host twin are bit-exact against this file."""
import numpy as np

import bc7_oracle as B

MODES_DEFAULT, MODES_EXTENDED = 0, 1
W2, W3 = np.array(B.WEIGHTS[2], np.int64), np.array(B.WEIGHTS[3], np.int64)
MASKS = B.P2.astype(bool)  # [64, 16]: texel i of partition s lies in subset 1


def e7(x):
    return (x << 1) | (x >> 6)


_E7 = e7(np.arange(128, dtype=np.int64))


def nearest7(t, allowed):
    """[...] targets -> the x of `allowed` (ascending) that minimises |e7(x) - t|, ties to the smaller x: the plain search."""
    allowed = np.asarray(allowed, np.int64)
    d = np.abs(_E7[allowed][(None,) * t.ndim] - t[..., None])
    return allowed[d.argmin(axis=-1)]  # argmin: the first minimum


def q1(t0, t1):
    """Mode 1's quantiser: [N, 3] targets of both endpoints -> (x0, x1) [N, 3] 7-bit values of one shared parity."""
    cand, err = [], []
    for p in (0, 1):
        allowed = np.arange(p, 128, 2)
        x0, x1 = nearest7(t0, allowed), nearest7(t1, allowed)
        cand.append((x0, x1))
        err.append(((e7(x0) - t0) ** 2).sum(axis=1) + ((e7(x1) - t1) ** 2).sum(axis=1))
    one = (err[1] < err[0])[:, None]
    x0, x1 = np.where(one, cand[1][0], cand[0][0]), np.where(one, cand[1][1], cand[0][1])
    return e7(x0), e7(x1)


def q5(t0, t1):
    allowed = np.arange(128)
    return e7(nearest7(t0, allowed)), e7(nearest7(t1, allowed))


def identity(t0, t1):
    return t0, t1


def search(u, S, e0, e1, W):
    """(k [N, 16], sse [N] summed over S)."""
    pal = ((64 - W)[None, :, None] * e0[:, None, :] + W[None, :, None] * e1[:, None, :] + 32) >> 6
    d = ((pal[:, None, :, :] - u[:, :, None, :]) ** 2).sum(axis=3)
    return d.argmin(axis=2), np.where(S, d.min(axis=2), 0).sum(axis=1)


def subfit(v, S, C, W, Q, stages=False):
    """F(S, C, weights, Q): v [N, 16, 4] texels, S [N, 16] bool (no empty set), C the channels.
    -> (E0, E1 [N, len(C)] decoded endpoint bytes, k [N, 16], sse [N]); stages: + (has_refit, first sse, refit taken)."""
    u = v[:, :, list(C)]
    n = np.arange(len(v))
    Sc = S[:, :, None]
    cnt = S.sum(axis=1)
    lo, hi = np.where(Sc, u, 255).min(axis=1), np.where(Sc, u, 0).max(axis=1)
    cs = np.argmax(hi - lo, axis=1)
    star = np.where(S, u[n, :, cs], 0)
    us = np.where(Sc, u, 0)
    cov = cnt[:, None] * (star[:, :, None] * us).sum(axis=1) - star.sum(axis=1)[:, None] * us.sum(axis=1)
    flip = cov < 0
    flip[n, cs] = False
    t0, t1 = np.where(flip, hi, lo), np.where(flip, lo, hi)
    e0, e1 = Q(t0, t1)
    k, sse = search(u, S, e0, e1, W)
    w = np.where(S, W[k], 0)
    m = np.where(S, 64 - W[k], 0)
    a, b, c = (m * m).sum(axis=1), (m * w).sum(axis=1), (w * w).sum(axis=1)
    x, y = (m[:, :, None] * u).sum(axis=1), (w[:, :, None] * u).sum(axis=1)
    det = a * c - b * b
    ok = det != 0
    d = np.where(ok, det, 1)[:, None]
    r0 = np.clip(B.rdiv(64 * (c[:, None] * x - b[:, None] * y), d), 0, 255)
    r1 = np.clip(B.rdiv(64 * (a[:, None] * y - b[:, None] * x), d), 0, 255)
    f0, f1 = Q(r0, r1)
    k2, sse2 = search(u, S, f0, f1, W)
    take = ok & (sse2 < sse)
    t = take[:, None]
    out = (np.where(t, f0, e0), np.where(t, f1, e1), np.where(t, k2, k), np.where(take, sse2, sse))
    return out + (ok, sse, take) if stages else out


def best_partition(v):
    """[N, 16, 4] -> [N] the partition of the smallest within-subset scatter of R, G, B; exact integers, ties to the smaller."""
    rgb = v[:, :, :3].astype(np.int64)
    m = MASKS.astype(np.int64)
    n1 = m.sum(axis=1)
    n0 = 16 - n1
    s1 = np.einsum("sp,npc->nsc", m, rgb)
    s0 = rgb.sum(axis=1)[:, None, :] - s1
    N = n1[None, :] * (s0 * s0).sum(axis=2) + n0[None, :] * (s1 * s1).sum(axis=2)  # [N, 64], below 2^32
    d = n0 * n1
    out = np.zeros(len(v), np.int64)
    bn, bd = N[:, 0].copy(), np.full(len(v), d[0])
    for s in range(1, 64):
        better = N[:, s] * bd > bn * d[s]
        out[better], bn[better], bd[better] = s, N[better, s], d[s]
    return out


def _flip(e0, e1, k, anchor_k, top):
    f = anchor_k >= (top + 1) // 2
    return np.where(f[:, None], e1, e0), np.where(f[:, None], e0, e1), np.where(f[:, None], top - k, k), f


def mode1(v, stages=False):
    """[N, 16, 4] opaque texels -> (blocks [N, 16] uint8, sse1 [N])."""
    part = best_partition(v)
    S1 = MASKS[part]
    fits = [subfit(v, S, (0, 1, 2), W3, q1, stages=True) for S in (~S1, S1)]
    sse = fits[0][3] + fits[1][3]
    anchor = [np.zeros(len(v), np.int64), B.A2[part].astype(np.int64)]
    n = np.arange(len(v))
    ends, flips = [], []
    k = np.zeros((len(v), 16), np.int64)
    for j, S in enumerate((~S1, S1)):
        e0, e1, kj = fits[j][:3]
        e0, e1, kj, f = _flip(e0, e1, kj, kj[n, anchor[j]], 7)
        ends += [e0, e1]
        flips.append(f)
        k = np.where(S, kj, k)
    blocks = []
    for i in range(len(v)):
        bits, pos = 2 | int(part[i]) << 2, 8
        for c in range(3):
            for e in ends:
                bits |= (int(e[i, c]) >> 2) << pos
                pos += 6
        for j in (0, 1):
            bits |= ((int(ends[2 * j][i, 0]) >> 1) & 1) << pos
            pos += 1
        for p in range(16):
            nb = 2 if p in (0, int(anchor[1][i])) else 3
            assert int(k[i, p]) < 1 << nb
            bits |= int(k[i, p]) << pos
            pos += nb
        assert pos == 128
        blocks.append(np.frombuffer(bits.to_bytes(16, "little"), np.uint8))
    blocks = np.stack(blocks) if blocks else np.zeros((0, 16), np.uint8)
    if stages:
        return blocks, sse, dict(partition=part, fits=fits, flips=flips, p=[(ends[0][:, 0] >> 1) & 1, (ends[2][:, 0] >> 1) & 1])
    return blocks, sse


def mode5(v, stages=False):
    """[N, 16, 4] texels -> (blocks [N, 16] uint8, sse5 [N]); rotation 0."""
    S = np.ones((len(v), 16), bool)
    col = subfit(v, S, (0, 1, 2), W2, q5, stages=True)
    alp = subfit(v, S, (3,), W2, identity, stages=True)
    sse = col[3] + alp[3]
    c0, c1, kc, fc = _flip(col[0], col[1], col[2], col[2][:, 0], 3)
    a0, a1, ka, fa = _flip(alp[0], alp[1], alp[2], alp[2][:, 0], 3)
    blocks = []
    for i in range(len(v)):
        bits, pos = 1 << 5, 8
        for c in range(3):
            for e in (c0, c1):
                bits |= (int(e[i, c]) >> 1) << pos
                pos += 7
        for e in (a0, a1):
            bits |= int(e[i, 0]) << pos
            pos += 8
        for k in (kc, ka):
            for p in range(16):
                nb = 1 if p == 0 else 2
                assert int(k[i, p]) < 1 << nb
                bits |= int(k[i, p]) << pos
                pos += nb
        assert pos == 128
        blocks.append(np.frombuffer(bits.to_bytes(16, "little"), np.uint8))
    blocks = np.stack(blocks) if blocks else np.zeros((0, 16), np.uint8)
    if stages:
        return blocks, sse, dict(colour=col, alpha=alp, flips=[fc, fa])
    return blocks, sse


def encode_texels(v, modes=MODES_EXTENDED, stages=False):
    """[N, 16, 4] int64 texels -> [N, 16] uint8 blocks.  stages: also (sse6 [N], candidate sse [N], claimed sse [N], mode [N])."""
    b6, _, sse6, _ = B.encode_texels(v, stages=True)
    if modes == MODES_DEFAULT:
        return (b6, sse6, sse6, sse6, np.full(len(v), 6)) if stages else b6
    opaque = (v[:, :, 3] == 255).all(axis=1)
    blocks, cand, mode = b6.copy(), sse6.copy(), np.full(len(v), 6)
    for sel, fn, m in ((opaque, mode1, 1), (~opaque, mode5, 5)):
        if sel.any():
            bm, sm = fn(v[sel])
            cand[sel] = sm
            take = sm < sse6[sel]
            idx = np.flatnonzero(sel)[take]
            blocks[idx] = bm[take]
            mode[idx] = m
    claimed = np.minimum(cand, sse6)
    return (blocks, sse6, cand, claimed, mode) if stages else blocks


def oracle_encode(img, gh=None, gw=None, swap=False, modes=MODES_EXTENDED):
    """[h, w, 3 or 4] uint8 image -> the block stream (bytes) of the grid max(h, gh) x max(w, gw)."""
    return encode_texels(B.block_texels(img, gh, gw, swap), modes).tobytes()


def block_modes(blocks):
    """Block stream -> [N] the mode of each block, read from byte 0."""
    b0 = np.frombuffer(bytes(blocks), np.uint8).reshape(-1, 16)[:, 0].astype(np.int64)
    return np.array([(int(x) & -int(x)).bit_length() - 1 for x in b0])


def three_colour_block(part, a=(200, 40, 40), b=(40, 180, 60), c=(40, 150, 100)):
    """The partition probe: subset 0 flat a, subset 1 alternating b and c; [16, 4] opaque texels."""
    out, t = np.zeros((16, 4), np.int64), 0
    for p in range(16):
        if MASKS[part][p]:
            out[p, :3] = b if t % 2 == 0 else c
            t += 1
        else:
            out[p, :3] = a
    out[:, 3] = 255
    return out


def stepped_edge_image(h, w, comps=3):
    """Two shaded regions that meet along a stepped diagonal edge: the content mode 1's partitions are for."""
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    left = (x + 2 * (y // 3)) % 16 < 8
    img = np.empty((h, w, 4), np.int64)
    shade = (3 * x + 5 * y) % 24
    img[..., 0] = np.where(left, 190 + shade, 30 + shade)
    img[..., 1] = np.where(left, 60 + shade // 2, 140 + shade)
    img[..., 2] = np.where(left, 40 + shade, 200 - shade)
    img[..., 3] = 255
    return img.astype(np.uint8)[..., :comps].copy()


def modes_wave_image():
    """256 x 256 RGBA8: every 4 x 4 block of a 64-block row segment (one wave of the wide kernel) is dealt one of eight kinds --
    the three-colour probe of a random partition (mode 1, subset 0 with det = 0), opaque flat (det = 0 in both subsets), an
    opaque ramp on one line (mode 6 kept), translucent noise (mode 5, every flip), colour and alpha on one line (non-opaque,
    mode 6 kept), colour and alpha ramps that disagree, flat translucent (half of them with even bytes: mode 6 exact, the
    candidate is never fitted), opaque noise (mode 1, every flip) -- so the lanes of every wave disagree at every branch
    (asserted in tests/test_bc7_modes_host.py)."""
    g = np.random.Generator(np.random.PCG64(0xBC7157))
    kinds = g.integers(0, 8, (64, 64))
    img = np.zeros((256, 256, 4), np.uint8)
    i = np.arange(16).reshape(4, 4)
    for by in range(64):
        for bx in range(64):
            k = kinds[by, bx]
            if k == 0:
                b = three_colour_block(int(g.integers(0, 64))).reshape(4, 4, 4)
            elif k == 1:
                b = np.broadcast_to(np.append(g.integers(0, 256, 3), 255), (4, 4, 4))
            elif k == 2:
                b = np.stack([240 - 16 * i, 230 - 12 * i, 20 + 3 * i, np.full((4, 4), 255)], axis=2)
            elif k == 3:
                b = g.integers(0, 256, (4, 4, 4))
            elif k == 4:
                b = np.stack([16 * i] * 4, axis=2)
            elif k == 5:
                b = np.stack([10 + 15 * i, 20 + 9 * i, 30 + (i * 7) % 50, 250 - 13 * i + (i % 3) * 20], axis=2)
            elif k == 6:
                b = np.broadcast_to(g.integers(0, 255, 4) & (0xfe if g.integers(0, 2) else 0xff), (4, 4, 4))  # even: mode 6 is exact
            else:
                b = np.concatenate([g.integers(0, 256, (4, 4, 3)), np.full((4, 4, 1), 255)], axis=2)
            img[4 * by:4 * by + 4, 4 * bx:4 * bx + 4] = np.clip(b, 0, 255)
    return img, kinds
