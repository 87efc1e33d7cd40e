"""BC6H with the opt-in two-subset candidate (include/ic_amd.h ICAMD_BC6H_MODES_EXTENDED): the DEFINITION restated
in numpy on top of bc6h_oracle (the one-subset definition, the decoder's arithmetic, the mode layouts).  The kernels
(csrc/bc6h_modes_block.h) and their host twin are bit-exact against this file; what it writes is read back by bc6h_oracle's
decode_blocks, which this file does not touch."""
import numpy as np

import bc6h_oracle as B

MODES_DEFAULT, MODES_EXTENDED = 0, 1
LADDER = (0, 5, 6, 7, 8, 1, 9)  # rows of B.MODES in the order they are tried: 00, 01110, 10010, 10110, 11010, 01, 11110
LADDER_FIELDS = tuple(B.MODES[m][0] for m in LADDER)
ONE_SUBSET_FIELD = 0b00011
MASKS = np.asarray(B.P2, np.int64)    # [32, 16]: texel i of partition s lies in subset 1
ANCHORS = np.asarray(B.A2, np.int64)  # [32]: subset 1's anchor
W3 = B.W3
NO_REFIT, TAKEN, NOT_BETTER, INFEASIBLE = 0, 1, 2, 3  # a subset's refit: det = 0 | taken | refused, not strictly smaller | refused, infeasible


def q_range(b, signed):
    return (-((1 << (b - 1)) - 1), (1 << (b - 1)) - 1) if signed else (0, (1 << b) - 1)


def D(q, b, signed):
    """The t-domain value a b-bit endpoint q decodes to at weight 0."""
    d = B.finish(B.unquantise(q, b, signed), signed)
    return B._signed_value(d) if signed else d


def quantise(T, b, signed):
    """Q_b by the definition: the smallest q minimising |D_b(q) - T|."""
    lo, hi = q_range(b, signed)
    q = np.arange(lo, hi + 1)
    d = D(q, b, signed)
    T = np.asarray(T, np.int64)
    err = np.abs(d[None, :] - T.reshape(-1, 1))
    return q[err.argmin(axis=1)].reshape(T.shape)


def best_partition(t):
    """Step 1: the largest N_s / d_s over the 32 partitions, exact, ties to the smaller s."""
    t = np.asarray(t, np.int64)
    tot = t.sum(axis=1)
    best = np.zeros(len(t), np.int64)
    bn, bd = np.zeros(len(t), np.int64), np.ones(len(t), np.int64)
    for s in range(32):
        m = MASKS[s]
        n1 = int(m.sum())
        n0 = 16 - n1
        s1 = (t * m[None, :, None]).sum(axis=1)
        s0 = tot - s1
        N = n1 * (s0 * s0).sum(axis=1) + n0 * (s1 * s1).sum(axis=1)
        d = n0 * n1
        better = N * bd > bn * d
        best, bn, bd = np.where(better, s, best), np.where(better, N, bn), np.where(better, d, bd)
    return best


def subset_targets(t, mask):
    """Step 2 over the texels of `mask` ([N, 16] bool, never empty): T0, T1 [N, 3]."""
    big = 1 << 40
    lo = np.where(mask[:, :, None], t, big).min(axis=1)
    hi = np.where(mask[:, :, None], t, -big).max(axis=1)
    cs = np.argmax(hi - lo, axis=1)
    n = np.arange(len(t))
    tm = t * mask[:, :, None]
    star = tm[n, :, cs]
    cov = mask.sum(axis=1)[:, None] * (star[:, :, None] * tm).sum(axis=1) - star.sum(axis=1)[:, None] * tm.sum(axis=1)
    flip = cov < 0
    flip[n, cs] = False
    return np.where(flip, hi, lo), np.where(flip, lo, hi)


def feasible(E, li, signed):
    """E [N, 4, 3] endpoints -> [N] bool: the ladder's mode li can hold them."""
    _, _, _, delta, transformed, _, _ = B.MODES[LADDER[li]]
    ok = np.ones(len(E), bool)
    if not transformed:
        return ok
    for c in range(3):
        lo, hi = -(1 << (delta[c] - 1)), (1 << (delta[c] - 1)) - 1
        for base in (0, 1):
            d = E[:, :, c] - E[:, base, c][:, None]
            ok &= ((d >= lo) & (d <= hi)).all(axis=1)
    if signed:
        ok &= (E >= 0).all(axis=(1, 2))
    return ok


def palette(e0, e1, b, signed):
    """[N, 3] endpoints -> [N, 8, 3] palette in the t domain: the decoder's arithmetic."""
    u0, u1 = B.unquantise(e0, b, signed), B.unquantise(e1, b, signed)
    p = B.finish(B.interpolate(u0[:, None, :], u1[:, None, :], W3[None, :, None]), signed)
    return B._signed_value(p) if signed else p


def search(t, mask, e0, e1, b, signed):
    """Indices [N, 16] (the smallest k of the least distance) and the sub-sse over the texels of `mask`."""
    pal = palette(e0, e1, b, signed)
    d = ((pal[:, None, :, :] - t[:, :, None, :]) ** 2).sum(axis=3)
    return d.argmin(axis=2), (d.min(axis=2) * mask).sum(axis=1)


def refit_targets(t, mask, k, signed):
    w = W3[k] * mask
    m = (64 - W3[k]) * mask
    a, b, c = (m * m).sum(axis=1), (m * w).sum(axis=1), (w * w).sum(axis=1)
    x, y = (m[:, :, None] * t).sum(axis=1), (w[:, :, None] * t).sum(axis=1)
    det = a * c - b * b
    ok = det != 0
    d = np.where(ok, det, 1)[:, None]
    lo = -B.T_MAX if signed else 0
    t0 = np.clip(B.rdiv(64 * (c[:, None] * x - b[:, None] * y), d), lo, B.T_MAX)
    t1 = np.clip(B.rdiv(64 * (a[:, None] * y - b[:, None] * x), d), lo, B.T_MAX)
    return t0, t1, ok


def pack(li, E, part, k):
    """Step 6.  E [N, 4, 3] after the anchor exchanges, k [N, 16] likewise."""
    m = LADDER[li]
    field, mbits, ep, delta, transformed, _, _ = B.MODES[m]
    lay = B.layout(m)
    out = []
    for n in range(len(E)):
        f = [0] * 13
        for c in range(3):
            e0 = int(E[n, 0, c])
            f[4 * c] = e0 & ((1 << ep) - 1)
            for e in (1, 2, 3):
                v = int(E[n, e, c]) - e0 if transformed else int(E[n, e, c])
                if transformed:
                    assert -(1 << (delta[c] - 1)) <= v < (1 << (delta[c] - 1))
                f[4 * c + e] = v & ((1 << delta[c]) - 1)
        f[12] = int(part[n])
        bits, pos = field, mbits
        for fi, fb in lay:
            bits |= ((f[fi] >> fb) & 1) << pos
            pos += 1
        assert pos == 82
        anchor = int(ANCHORS[part[n]])
        for i in range(16):
            width = 2 if i in (0, anchor) else 3
            assert int(k[n, i]) < (1 << width)
            bits |= int(k[n, i]) << pos
            pos += width
        assert pos == 128
        out.append(np.frombuffer(bits.to_bytes(16, "little"), np.uint8))
    return np.stack(out) if out else np.zeros((0, 16), np.uint8)


def candidate(t, signed):
    """Steps 1-6 of the two-subset candidate: (blocks [N, 16] uint8, sse2 [N], stages dict)."""
    t = np.asarray(t, np.int64)
    n_blocks = len(t)
    part = best_partition(t)
    masks = [MASKS[part] == 0, MASKS[part] == 1]
    T = np.zeros((n_blocks, 4, 3), np.int64)
    for j in (0, 1):
        T[:, 2 * j], T[:, 2 * j + 1] = subset_targets(t, masks[j])
    # step 3: the first feasible mode of the ladder
    ladder = np.full(n_blocks, -1, np.int64)
    E = np.zeros((n_blocks, 4, 3), np.int64)
    for li, m in enumerate(LADDER):
        q = quantise(T, B.MODES[m][2], signed)
        take = (ladder < 0) & feasible(q, li, signed)
        ladder[take] = li
        E[take] = q[take]
    assert (ladder >= 0).all()
    first = np.zeros((2, n_blocks), np.int64)
    final = np.zeros((2, n_blocks), np.int64)
    outcome = np.zeros((2, n_blocks), np.int64)
    k = np.zeros((n_blocks, 16), np.int64)
    # step 4, mode by mode (b is the mode's)
    for li, m in enumerate(LADDER):
        sel = np.flatnonzero(ladder == li)
        if len(sel) == 0:
            continue
        b = B.MODES[m][2]
        ts, Es = t[sel], E[sel].copy()
        ks = np.zeros((len(sel), 16), np.int64)
        for j in (0, 1):
            mk = masks[j][sel]
            k1, sse_a = search(ts, mk, Es[:, 2 * j], Es[:, 2 * j + 1], b, signed)
            r0, r1, ok = refit_targets(ts, mk, k1, signed)
            f0, f1 = quantise(r0, b, signed), quantise(r1, b, signed)
            k2, sse_b = search(ts, mk, f0, f1, b, signed)
            trial = Es.copy()
            trial[:, 2 * j], trial[:, 2 * j + 1] = f0, f1
            better, fits = ok & (sse_b < sse_a), feasible(trial, li, signed)
            take = better & fits
            Es[take] = trial[take]
            kj = np.where(take[:, None], k2, k1)
            ks = np.where(mk, kj, ks)
            first[j, sel], final[j, sel] = sse_a, np.where(take, sse_b, sse_a)
            outcome[j, sel] = np.where(~ok, NO_REFIT, np.where(take, TAKEN, np.where(better, INFEASIBLE, NOT_BETTER)))
        E[sel], k[sel] = Es, ks
    # step 5
    rows = np.arange(n_blocks)
    anchors = [np.zeros(n_blocks, np.int64), ANCHORS[part]]
    flips = []
    for j in (0, 1):
        flip = k[rows, anchors[j]] >= 4
        flips.append(flip)
        e0, e1 = E[:, 2 * j].copy(), E[:, 2 * j + 1].copy()
        E[:, 2 * j], E[:, 2 * j + 1] = np.where(flip[:, None], e1, e0), np.where(flip[:, None], e0, e1)
        k = np.where(flip[:, None] & masks[j], 7 - k, k)
    blocks = np.zeros((n_blocks, 16), np.uint8)
    for li in range(len(LADDER)):
        sel = np.flatnonzero(ladder == li)
        if len(sel):
            blocks[sel] = pack(li, E[sel], part[sel], k[sel])
    stages = {"partition": part, "ladder": ladder, "first": first, "final": final, "refit": outcome, "flips": flips, "E": E}
    return blocks, final.sum(axis=0), stages


def encode_texels(t, signed, modes=MODES_EXTENDED, stages=False):
    """[N, 16, 3] int64 targets -> [N, 16] uint8 blocks.  stages: (blocks, dict) with the candidate's stages and sse1 (the
    one-subset block's final sse), sse2, chosen (the candidate was written), claimed (the written block's sse)."""
    t = np.asarray(t, np.int64)
    one, _, sse1, _, _ = B.encode_texels(t, signed, stages=True)
    if modes == MODES_DEFAULT:
        st = {"sse1": sse1, "sse2": sse1, "chosen": np.zeros(len(t), bool), "claimed": sse1}
        return (one, st) if stages else one
    assert modes == MODES_EXTENDED
    cand, sse2, st = candidate(t, signed)
    chosen = sse2 < sse1
    blocks = np.where(chosen[:, None], cand, one)
    st.update(sse1=sse1, sse2=sse2, chosen=chosen, claimed=np.where(chosen, sse2, sse1))
    return (blocks, st) if stages else blocks


def oracle_encode(img, signed, gh=None, gw=None, modes=MODES_EXTENDED):
    return encode_texels(B.block_texels(img, signed, gh, gw), signed, modes).tobytes()


def block_fields(blocks):
    """The mode field of every block (bits 0..1 where they are 00 or 01, else bits 0..4), from byte 0."""
    b0 = np.frombuffer(bytes(blocks), np.uint8).reshape(-1, 16)[:, 0].astype(np.int64)
    return np.where((b0 & 3) < 2, b0 & 3, b0 & 31)


def stored_endpoints(blocks, signed):
    """The header fields of two-subset blocks through bc6h_oracle's layouts: [(mode row, e0 [3], deltas [3, 3] sign-extended)]."""
    out = []
    for blk in np.frombuffer(bytes(blocks), np.uint8).reshape(-1, 16):
        m = B.mode_of(int(blk[0]))
        _, mbits, ep, delta, transformed, ns, _ = B.MODES[m]
        v = int.from_bytes(bytes(blk), "little")
        f = [0] * 13
        for pos, (fi, fb) in enumerate(B.layout(m), start=mbits):
            f[fi] |= ((v >> pos) & 1) << fb
        e0 = [f[4 * c] for c in range(3)]
        if signed:
            e0 = [int(B._sext(np.int64(x), ep)) for x in e0]
        d = [[int(B._sext(np.int64(f[4 * c + e]), delta[c])) for e in (1, 2, 3)] for c in range(3)]
        out.append((m, e0, d))
    return out


# ---- test content (integer-only)

EDGE_GAPS = (60, 150, 400, 900, 1500, 2200, 3000, 5500, 9000, 14000)
EDGE_SCALES = ((4, 4, 4), (10, 4, 4), (4, 10, 4), (4, 4, 10))  # quarters: the gap of R, G, B


def edge_content(h, w, chans, seed=0):
    """[h, w, chans] uint16 half bits.  Every 4 x 4 block holds two small colour ramps separated by a straight edge (vertical,
    horizontal or diagonal); the gap between the sides cycles over EDGE_GAPS t-units, scaled per channel by EDGE_SCALES; every
    seventh block's far side is negative (zero to the unsigned format)."""
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    n = (y // 4) * ((w + 3) // 4) + x // 4 + 5 * seed
    u, v = x % 4, y % 4
    kind = n % 3
    side = np.where(kind == 0, u >= 2, np.where(kind == 1, v >= 2, u + v >= 4)).astype(np.int64)
    along = np.where(kind == 0, v, np.where(kind == 1, u, (u - v) % 4))
    gap = np.array(EDGE_GAPS)[n % len(EDGE_GAPS)]
    scale = np.array(EDGE_SCALES)[(n // 2) % len(EDGE_SCALES)]  # [h, w, 3]
    base = 2000 + (n * 911) % 9000
    step = 6 + (n * 7) % 40
    img = np.zeros((h, w, 4), np.int64)
    for c in range(4):
        s = scale[..., min(c, 2)]
        val = base + 300 * c + side * (gap * s // 4) + along * step * (1 + (c + side) % 2) + ((u * 3 + v * 5 + c) % 4)
        val = np.clip(val, 0, B.T_MAX)
        img[..., c] = np.where((n % 7 == 3) & (side == 1), val | 0x8000, val)
    return (img & 0xFFFF).astype(np.uint16)[..., :chans].copy()


def content(name, h, w, chans, seed=0):
    return edge_content(h, w, chans, seed) if name == "edge" else B.content(name, h, w, chans, seed)


CONTENTS = B.CONTENTS + ("edge",)


# ---- a wave whose lanes disagree

def blocks_of(img):
    """[h, w, c] (h, w multiples of 4) -> [n, 4, 4, c]: the image's blocks in raster order."""
    h, w, c = img.shape
    return img.reshape(h // 4, 4, w // 4, 4, c).transpose(0, 2, 1, 3, 4).reshape(-1, 4, 4, c)


def wave_flags(st):
    """Per-block booleans of the stages a wave's lanes should disagree in."""
    flags = {"ladder %s" % format(f, "05b" if i not in (0, 5) else "02b"): st["ladder"] == i for i, f in enumerate(LADDER_FIELDS)}
    flags["replaced"] = st["chosen"]
    for j in (0, 1):
        flags["refit taken, subset %d" % j] = st["refit"][j] == TAKEN
        flags["refit not better, subset %d" % j] = st["refit"][j] == NOT_BETTER
        flags["anchor exchange, subset %d" % j] = st["flips"][j]
    flags["negative endpoint"] = (st["E"] < 0).any(axis=(1, 2))
    return flags


def wave_image(signed, chans=3):
    """([32, 32, chans] uint16, flags): 64 blocks -- one wave -- picked from the contents by the oracle's stages so that every flag
    of wave_flags that the pool can show is true in some lanes and false in others (the signed format alone has negative
    endpoints)."""
    pool = np.concatenate([blocks_of(content(name, hw, hw, chans)) for name, hw in
                           (("edge", 64), ("noise", 32), ("ldr", 32), ("gradient", 32), ("exponents", 32), ("two_valued", 32))])
    t = B.target(pool[..., :3], signed).reshape(-1, 16, 3)
    _, st = encode_texels(t, signed, stages=True)
    picked = []
    for f in wave_flags(st).values():
        for want in (True, False):
            picked += [i for i in np.flatnonzero(f == want)[:2] if i not in picked]
    picked += [i for i in range(0, len(pool), 7) if i not in picked]
    picked = np.array(picked[:64])
    assert len(picked) == 64
    img = pool[picked].reshape(8, 8, 4, 4, chans).transpose(0, 2, 1, 3, 4).reshape(32, 32, chans)
    _, st = encode_texels(t[picked], signed, stages=True)
    return np.ascontiguousarray(img), wave_flags(st)
