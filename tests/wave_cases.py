"""Probe and partner blocks for the kernels' wave votes (wave_all / wave_count in ic_device.h), and the 64-lane waves
built from them.  Shared by the host tier (tests/test_wave_votes_host.py: a lockstep wave in the host emulation) and the
GPU tier (tests/test_gpu_wave_votes.py: the same mixes laid out as textures).

A probe sits at the boundary of a vote's predicate; a partner vetoes a shortcut that the probe would take alone.  A
composition is a list of up to 64 blocks, one per lane.  Blocks are (4, 4, 4) uint8 RGBA arrays (RGB sources use the
first three channels); compressed words are little-endian uint32 arrays of 2 (DXT1 / ETC1) or 4 (DXT5) dwords.

Plain numpy, no GPU and no library: every block is a function of its name.
"""
import numpy as np

LANES = 64
BUSY_SPREAD = 4 * 141                 # ICAMD_ETC1_BUSY_SPREAD: spread of 2 (r + g + b) over the block
DXT_WIDE = 27                         # dxt_block.h: threshold index search iff every lane's L(max) - L(min) >= 27
ETC_A = (2, 5, 9, 13, 18, 24, 33, 47)
ETC_B = (8, 17, 29, 42, 60, 80, 106, 183)
# the values an ETC1 base channel can decode to: Extend5Bit (differential) and 17 q (individual)
BASE5 = sorted({(q << 3) | (q >> 2) for q in range(32)})
BASE4 = [17 * q for q in range(16)]


def _rng(name):
    return np.random.Generator(np.random.PCG64(sum(ord(c) * (i + 1) for i, c in enumerate(name))))


def block(rgb, alpha=255):
    """A (4, 4, 4) block from a (4, 4, 3) array-like of colours."""
    b = np.empty((4, 4, 4), np.uint8)
    b[..., :3] = np.clip(np.asarray(rgb, np.int64), 0, 255)
    b[..., 3] = alpha
    return b


def solid(rgb, alpha=255):
    return block(np.broadcast_to(np.asarray(rgb), (4, 4, 3)), alpha)


def checker(base, d):
    """base +/- d on a checkerboard: every sub-block of both ETC1 partitions averages to exactly `base`, so all four
    searches see the decoded base `base` (when it is an Extend5Bit value) and deviations of d."""
    y, x = np.mgrid[0:4, 0:4]
    s = np.where((x + y) % 2 == 0, 1, -1)[..., None]
    return block(np.asarray(base)[None, None, :] + s * np.asarray(d)[None, None, :])


# ------------------------------------------------------------------------------------------------ probes (encoders)


def dxt_luma(rgb):
    rgb = np.asarray(rgb, np.int64)
    return 4 * rgb[..., 0] + 8 * rgb[..., 1] + rgb[..., 2]   # the encoder's 16 L / 16 for R, G, B order


def dxt_range_probe(rng_l, variant=0):
    """Two colours whose luminance range is exactly rng_l (and distinct 565 endpoints), on a pattern."""
    lo = np.array([96, 100, 104]) + 8 * variant
    if variant % 3 == 0:
        hi = lo + [0, 0, rng_l]                   # range in blue
    elif variant % 3 == 1:
        hi = lo + [rng_l // 4, 0, rng_l % 4]      # mostly red
    else:
        hi = lo + [0, rng_l // 8, rng_l % 8]      # mostly green
    y, x = np.mgrid[0:4, 0:4]
    pat = ((x * 5 + y * 3 + variant) % 4)[..., None]
    mid = lo + (hi - lo) // 2
    rgb = np.where(pat == 0, lo, np.where(pat == 1, hi, mid))
    assert dxt_luma(rgb).max() - dxt_luma(rgb).min() == rng_l
    return block(rgb)


def dxt5_park_probe(a_lo, a_hi, n255=3, n0=2):
    """DXT5 alpha in the six-value mode (two or more 0 / 255 pixels) with a1 < 255: park != 0 for the 255 pixels."""
    a = np.linspace(a_lo, a_hi, 16).round().astype(np.int64).reshape(4, 4)
    flat = a.reshape(-1)
    flat[:n255] = 255
    flat[n255:n255 + n0] = 0
    b = block(np.full((4, 4, 3), 128) + np.arange(16).reshape(4, 4, 1))
    b[..., 3] = a
    return b


def etc_room_values(cw):
    """Base values whose room min(v, 255 - v) is the nearest attainable below, at and above kEtcB[cw] (gray bases)."""
    rooms = sorted({min(v, 255 - v) for v in BASE5})
    t = ETC_B[cw]
    below = [r for r in rooms if r < t]
    above = [r for r in rooms if r > t]
    out = []
    if below:
        out.append(below[-1])
    if t in rooms:
        out.append(t)
    if above:
        out.append(above[0])
    return out


def etc_room_probe(room, d=1, tint=0):
    """Checkerboard around a gray Extend5Bit base whose room is `room` (one channel tinted towards the middle)."""
    base = np.array([room, room, room])
    if tint:
        base[1] = BASE5[min(len(BASE5) - 1, BASE5.index(room) + tint)] if room in BASE5 else room
    return checker(base, [d, d, d])


def etc_d1_probe(d1):
    """One pixel at L1 distance d1 from the decoded base 132 of every sub-block containing it (pruning: d1 < 141)."""
    rgb = np.full((4, 4, 3), 128)
    per = [d1 // 3 + (1 if i < d1 % 3 else 0) for i in range(3)]
    rgb[0, 0] = [132 + per[0], 132 + per[1], 132 + per[2]]
    rgb[3, 3] = [126, 127, 128]
    return block(rgb)


def etc_spread_probe(spread):
    """Sums r + g + b spreading by spread / 2 (spread is even): busy iff spread >= 564."""
    half = spread // 2
    rgb = np.full((4, 4, 3), 60)
    rgb[1, 2] = 60 + np.array([half // 3 + (half % 3 > 0), half // 3 + (half % 3 > 1), half // 3])
    rgb[2, 1] = [61, 60, 60]
    assert 2 * (rgb.sum(-1).max() - rgb.sum(-1).min()) == spread
    return block(rgb)


def symmetric_block(seed, amp):
    """Transpose-symmetric content: the left | right and top | bottom partitions tie exactly (flip = 0 must win)."""
    r = np.random.Generator(np.random.PCG64(seed)).integers(-amp, amp + 1, (4, 4, 3))
    r = (r + r.transpose(1, 0, 2)) // 2
    return block(120 + r)


def near_tie_codewords(seed):
    """Small symmetric deviations on mid-tones: neighbouring codewords score within a few units."""
    g = np.random.Generator(np.random.PCG64(seed))
    base = np.array(BASE5[12:20])[g.integers(0, 8, 3)]
    d = g.integers(3, 8)
    y, x = np.mgrid[0:4, 0:4]
    s = np.where((x + 2 * y) % 3 == 0, 1, np.where((x + 2 * y) % 3 == 1, -1, 0))[..., None]
    return block(base + s * d)


def encoder_probes():
    """name -> block, for the DXT and ETC1 encoders."""
    p = {}
    for v in range(3):
        for l in (DXT_WIDE - 1, DXT_WIDE, DXT_WIDE + 1):
            p["dxt_lrange%d_v%d" % (l, v)] = dxt_range_probe(l, v)
    p["dxt5_park_6mode"] = dxt5_park_probe(40, 200)
    p["dxt5_park_a1_254"] = dxt5_park_probe(3, 254, n255=4, n0=3)
    p["dxt5_park_narrow"] = dxt5_park_probe(100, 110, n255=2, n0=2)
    for cw in range(8):
        for room in etc_room_values(cw):
            p["etc_room%d_cw%d" % (room, cw)] = etc_room_probe(room)
            p["etc_room%d_cw%d_tint" % (room, cw)] = etc_room_probe(room, d=2, tint=1)
    for d1 in (140, 141, 142):
        p["etc_d1_%d" % d1] = etc_d1_probe(d1)
    for s in (BUSY_SPREAD - 2, BUSY_SPREAD, BUSY_SPREAD + 2):
        p["etc_spread%d" % s] = etc_spread_probe(s)
    p["one_colour_mid"] = solid([131, 77, 200])
    p["one_colour_white"] = solid([255, 255, 255])
    p["one_colour_black"] = solid([0, 0, 0])
    ga = solid([40, 180, 90])
    ga[..., 3] = _rng("alpha").integers(0, 256, (4, 4))
    p["one_colour_varying_alpha"] = ga
    for i in range(3):
        p["sym_tie_%d" % i] = symmetric_block(100 + i, 6 + 10 * i)
        p["cw_near_tie_%d" % i] = near_tie_codewords(200 + i)
    return p


# ------------------------------------------------------------------------------------------------ partners (encoders)


def encoder_partners():
    """name -> block: each vetoes some vote that a probe would pass alone."""
    g = _rng("partners")
    p = {}
    p["saturated"] = block(g.choice(np.array([0, 255]), (4, 4, 3)))               # room 0 in every search
    p["saturated_gray"] = checker(np.array([8, 8, 8]), [8, 8, 8])                  # base 8: codeword 0 only
    p["noise_wide_d1"] = block(g.integers(0, 256, (4, 4, 3)))                      # d1 >= 141, busy, wide luminance
    p["narrow_luma"] = dxt_range_probe(5, 1)                                       # DXT: plain scan
    p["one_colour"] = solid([17, 201, 99])
    p["busy"] = block(np.where(g.random((4, 4, 1)) < 0.5, 20, 230) + g.integers(-5, 6, (4, 4, 3)))
    p["calm"] = block(100 + np.add.outer(np.arange(4), np.arange(4))[..., None] * [3, 2, 1])
    b = dxt5_park_probe(0, 0, n255=0, n0=0)
    b[..., 3] = g.integers(30, 220, (4, 4))                                        # eight-value alpha: park = 0
    p["alpha8"] = b
    return p


# ------------------------------------------------------------------------------------------------ compressed words


def dxt1_word(c0, c1, bits):
    return np.array([c0 | c1 << 16, bits], np.uint32)


def etc1_word(hi, lo):
    """ETC1 block from its big-endian high / low words, as the little-endian dwords the kernels read."""
    def bswap(v):
        v = int(v) & 0xffffffff
        return ((v & 0xff) << 24) | ((v >> 8 & 0xff) << 16) | ((v >> 16 & 0xff) << 8) | (v >> 24)
    return np.array([bswap(hi), bswap(lo)], np.uint32)


def etc1_diff_hi(b5, d3, cw0, cw1, flip):
    """Differential high word: 5-bit bases b5[3], 3-bit signed deltas d3[3]."""
    hi = 2 | flip | cw0 << 5 | cw1 << 2
    for ch in range(3):
        hi |= (b5[ch] & 31) << (27 - 8 * ch) | (d3[ch] & 7) << (24 - 8 * ch)
    return hi


def word_probes(codec):
    """name -> words of probes for the block operations (decode, Pad, Downsample, transcode)."""
    g = _rng("words%d" % codec)
    p = {}
    if codec == 0:
        p["dxt1_c0_lt_c1"] = dxt1_word(0x1234, 0xf00f, int(g.integers(0, 2**32)))
        p["dxt1_c0_lt_c1_black"] = dxt1_word(0x0000, 0xffff, 0xffffffff)   # index 3 = black everywhere
        p["dxt1_c0_eq_c1"] = dxt1_word(0x7bef, 0x7bef, int(g.integers(0, 2**32)))
        p["dxt1_c0_lt_c1_adjacent"] = dxt1_word(0x8410, 0x8411, 0xaaaa5555)
    elif codec == 1:
        # six-value alpha (a0 <= a1) next to the colour block; the colour half is always four-colour
        w = np.array([10 | 200 << 8 | 0x1234 << 16, 0x89abcdef, 0x1234 | 0xf00f << 16, 0x1b1b1b1b], np.uint32)
        p["dxt5_alpha6"] = w
        p["dxt5_alpha6_equal"] = np.array([77 | 77 << 8 | 0xfac0 << 16, 0x12345678, 0xffff, 0xe4e4e4e4], np.uint32)
        p["dxt5_alpha6_0_255"] = np.array([0 | 255 << 8 | 0xffff << 16, 0xffffffff, 0x0000ffff, 0], np.uint32)
    else:
        lo = int(g.integers(0, 2**32))
        p["etc1_base_below0"] = etc1_word(etc1_diff_hi([0, 1, 2], [-4, -4, -3], 7, 7, 0), lo)
        p["etc1_base_above255"] = etc1_word(etc1_diff_hi([31, 30, 29], [3, 3, 3], 6, 7, 1), lo)
        p["etc1_base_one_channel_out"] = etc1_word(etc1_diff_hi([16, 0, 16], [0, -1, 0], 3, 5, 0), lo)
    return p


def word_partners(codec):
    g = _rng("wordpartners%d" % codec)
    p = {}
    if codec == 0:
        p["dxt1_c0_gt_c1"] = dxt1_word(0xf00f, 0x1234, int(g.integers(0, 2**32)))
    elif codec == 1:
        p["dxt5_alpha8"] = np.array([220 | 12 << 8 | 0x5555 << 16, 0x12345678, 0xf00f | 0x1234 << 16, 0x4e4e4e4e],
                                    np.uint32)
    else:
        p["etc1_in_range"] = etc1_word(etc1_diff_hi([16, 12, 20], [1, -1, 0], 2, 4, 1), int(g.integers(0, 2**32)))
        p["etc1_individual"] = etc1_word(0x3c5a0000 | 0x1c | 0, int(g.integers(0, 2**32)))
    return p


def random_words(codec, n, seed):
    w = np.random.Generator(np.random.PCG64(seed)).integers(0, 2**32, (n, 4 if codec == 1 else 2), dtype=np.uint64)
    return w.astype(np.uint32)


# ------------------------------------------------------------------------------------------------ compositions


def _fill(probe, partner, n_partner, where="spread"):
    """64 lanes: the probe everywhere except n_partner lanes of the partner (spread over the wave)."""
    lanes = [probe] * LANES
    if n_partner:
        idx = np.linspace(0, LANES - 1, n_partner).round().astype(int) if where == "spread" else range(n_partner)
        for i in idx:
            lanes[int(i)] = partner
    return lanes


def encoder_compositions(family=None):
    """[(name, [64 blocks])]: every probe alone, with exactly one partner of each kind, and one probe among partners.
    family "dxt" / "etc": only the probes aimed at that encoder's votes (plus the shared one-colour and tie blocks)."""
    probes, partners = encoder_probes(), encoder_partners()
    out = []
    for pn, pb in probes.items():
        if family and pn.startswith(("dxt", "etc")) and not pn.startswith(family):
            continue
        out.append((pn + "/alone", [pb] * LANES))
        for qn, qb in partners.items():
            out.append((pn + "/one_" + qn, _fill(pb, qb, 1)))
            out.append((pn + "/among_" + qn, _fill(qb, pb, 1)))
    return out


def etc1_busy_compositions():
    """Busy counts 47 / 48 / 49 of 64 (the busy-wave vote, no one-colour lanes) and the 3/4 rule among non-constant lanes
    with 1, 16 and 63 one-colour lanes, below / at / above equality where the count allows it."""
    g = _rng("busy")
    busy = [block(np.where(g.random((4, 4, 1)) < 0.5, 10, 240) + g.integers(-9, 10, (4, 4, 3))) for _ in range(8)]
    calm = [block(90 + 10 * i + np.add.outer(np.arange(4), np.arange(4))[..., None] * [2, 1, 3]) for i in range(8)]
    const = [solid(g.integers(0, 256, 3)) for _ in range(8)]
    out = []
    for nb in (47, 48, 49):
        lanes = [busy[i % 8] if i < nb else calm[i % 8] for i in range(LANES)]
        order = np.random.Generator(np.random.PCG64(nb)).permutation(LANES)
        out.append(("busy%d_of_64" % nb, [lanes[i] for i in order]))
    for nc in (1, 16, 63):
        nn = LANES - nc
        # busy counts b with 4 b vs 3 nn: just below, equal (when 3 nn / 4 is whole), just above
        eq = 3 * nn / 4
        counts = sorted({int(np.ceil(eq)) - 1, int(np.floor(eq)) + 1} | ({int(eq)} if eq == int(eq) else set()))
        for nb in counts:
            if nb < 0 or nb > nn:
                continue
            lanes = [const[i % 8] for i in range(nc)] + [busy[i % 8] for i in range(nb)] + \
                    [calm[i % 8] for i in range(nn - nb)]
            order = np.random.Generator(np.random.PCG64(1000 * nc + nb)).permutation(LANES)
            rel = "eq" if 4 * nb == 3 * nn else ("above" if 4 * nb > 3 * nn else "below")
            out.append(("const%d_busy%d_%s" % (nc, nb, rel), [lanes[i] for i in order]))
    return out


def etc1_fast_dropout_compositions():
    """The unclamped shortcut (`fast`) drops out at codeword k = 1..7 for the wave while the probe lane (mid-tone, tiny
    deviations) wins codeword 0 on it: partners have room in [kEtcB[k-1], kEtcB[k]) and deviations that want codeword >= k,
    so some lanes won fast and some did not (the won_fast field rebuild)."""
    base_for_k = {1: 16, 2: 24, 3: 41, 4: 57, 5: 74, 6: 99, 7: 123}
    dev_for_k = {1: 16, 2: 24, 3: 41, 4: 57, 5: 74, 6: 99, 7: 47}
    probe = checker(np.array([123, 123, 123]), [1, 1, 1])
    out = []
    for k in range(1, 8):
        v, d = base_for_k[k], dev_for_k[k]
        partner = checker(np.array([v, v, v]), [d, d, d])
        for n_partner in (1, 32, 63):
            out.append(("fast_drop_cw%d_p%d" % (k, n_partner), _fill(probe, partner, n_partner)))
    return out


def word_compositions(codec):
    probes, partners = word_probes(codec), word_partners(codec)
    rnd = random_words(codec, LANES, 17 + codec)
    out = []
    for pn, pw in probes.items():
        out.append((pn + "/alone", [pw] * LANES))
        out.append((pn + "/among_random", [pw if i == 0 else rnd[i] for i in range(LANES)]))
        for qn, qw in partners.items():
            out.append((pn + "/one_" + qn, _fill(pw, qw, 1)))
            out.append((pn + "/among_" + qn, _fill(qw, pw, 1)))
    return out


# ------------------------------------------------------------------------------------------------ layouts


def is_one_colour(b):
    """What etc1_constant_block decides for the lane: the 16 pixels have one R, G, B (alpha does not count)."""
    return bool((b[..., :3] == b[0, 0, :3]).all())


def block_from(img, by, bx):
    """Block (by, bx) of an RGBA image as a (4, 4, 4) block."""
    b = np.asarray(img[4 * by:4 * by + 4, 4 * bx:4 * bx + 4])
    if b.shape[-1] == 3:
        b = np.concatenate([b, np.full(b.shape[:-1] + (1,), 255, np.uint8)], axis=-1)
    return np.ascontiguousarray(b)


def strip(blocks, comps):
    """The blocks side by side: a 4 x (4 n) image (each block is then encoded alone by the oracle)."""
    return np.ascontiguousarray(np.concatenate([b[..., :comps] for b in blocks], axis=1))


def to_dwords(blocks, comps):
    """n x 16 pixel dwords in the kernels' load format (load_block_interior): byte k = channel k; for 3-byte sources
    byte 3 is whatever the wide row load put there (the next pixel's first byte, 0 after the last pixel of a row)."""
    n = len(blocks)
    if comps == 4:
        return np.ascontiguousarray(np.stack(blocks).reshape(n, 16, 4)).view("<u4").reshape(n, 16)
    rows = np.stack([b[..., :3] for b in blocks]).reshape(n, 4, 12)
    rows = np.concatenate([rows, np.zeros((n, 4, 4), np.uint8)], axis=2)  # 12 row bytes, then 0
    out = np.empty((n, 4, 4), np.uint32)
    for x in range(4):
        out[:, :, x] = rows[:, :, 3 * x:3 * x + 4].copy().view("<u4")[..., 0]
    if comps == 3:
        out[:, :, 3] &= 0x00ffffff
    return out.reshape(n, 16)


# ------------------------------------------------------------------------------------------------ GPU motifs
# The GPU tier cannot place a block on a chosen lane: the lane -> block map differs per launch form (256 x 1 or
# 2^k x (256 >> k) tiles, 16 x 4-block ETC1 waves, tile columns dealt out per XCD, four lanes per block in the quad forms).
# So a composition becomes a 4 x 4-block MOTIF whose every row and column holds the same mix; tiled over a region of
# 4 block rows x 64 block columns it gives every aligned wave layout the library ships (64 x 1, 32 x 2, 16 x 4, and
# 16 blocks x 4 lanes) the same mix.  Exact counts (47 / 48 / 49, the +/-1 thresholds) belong to the host tier.

REGION_ROWS, REGION_COLS = 4, 64


def latin_motif(a, b, k):
    """16 items in raster order: b at k of the 4 places of every row and every column (cyclic diagonals), a elsewhere."""
    return [b if (x - y) % 4 < k else a for y in range(4) for x in range(4)]


def rows_motif(row):
    """A motif whose rows are the four cyclic shifts of `row` (4 items): every row and column holds the items of `row`."""
    return [row[(x + y) % 4] for y in range(4) for x in range(4)]


def region_grid(motifs, regions_across):
    """Item grid (block rows x block columns, a list of lists) holding each motif tiled over its own region."""
    n_rows = -(-len(motifs) // regions_across)
    grid = [[None] * (REGION_COLS * regions_across) for _ in range(REGION_ROWS * n_rows)]
    for m in range(n_rows * regions_across):
        motif = motifs[m % len(motifs)]
        r0, c0 = REGION_ROWS * (m // regions_across), REGION_COLS * (m % regions_across)
        for r in range(REGION_ROWS):
            for c in range(REGION_COLS):
                grid[r0 + r][c0 + c] = motif[4 * (r % 4) + c % 4]
    return grid


def grid_image(grid, comps):
    """An image from a grid of (4, 4, 4) blocks."""
    rows = [np.concatenate([b[..., :comps] for b in row], axis=1) for row in grid]
    return np.ascontiguousarray(np.concatenate(rows, axis=0))


def grid_words(grid):
    """Block bytes (raster order) from a grid of word arrays."""
    return np.ascontiguousarray(np.stack([np.asarray(w, np.uint32) for row in grid for w in row])).tobytes()


def encoder_motifs(family):
    """Every probe alone, with a partner at a quarter of the places, and at three quarters."""
    probes, partners = encoder_probes(), encoder_partners()
    out = []
    for pn, pb in probes.items():
        if pn.startswith(("dxt", "etc")) and not pn.startswith(family):
            continue
        out.append(latin_motif(pb, pb, 0))
        for qb in partners.values():
            out.append(latin_motif(pb, qb, 1))
            out.append(latin_motif(pb, qb, 3))
    return out


def etc1_wave_motifs():
    """Busy / calm / one-colour mixes (per row and column; per 64-lane wave x 16): a busy wave at exactly 48 of 64, a calm
    one at 32, mixed waves above and below the 3/4 rule, an all-one-colour wave; then the `fast` drop-out at codewords
    1..7 next to a lane that wins codeword 0 on the shortcut."""
    g = _rng("gpu-busy")
    busy = [block(np.where(g.random((4, 4, 1)) < 0.5, 10, 240) + g.integers(-9, 10, (4, 4, 3))) for _ in range(4)]
    calm = [block(90 + 10 * i + np.add.outer(np.arange(4), np.arange(4))[..., None] * [2, 1, 3]) for i in range(4)]
    const = [solid(g.integers(0, 256, 3)) for _ in range(4)]
    out = [rows_motif([busy[0], busy[1], busy[2], calm[0]]),     # busy 48 of 64
           rows_motif([busy[0], busy[1], calm[1], calm[2]]),     # calm
           rows_motif([const[0], busy[1], busy[2], busy[3]]),    # one-colour lanes, 3/4 rule: busy
           rows_motif([const[0], busy[1], busy[2], calm[3]]),    # 3/4 rule: 32 of 48, calm
           rows_motif([const[0], const[1], const[2], busy[3]]),  # 16 searching lanes, all busy
           rows_motif([const[0], const[1], const[2], calm[3]]),
           rows_motif([const[0], const[1], const[2], const[3]])]
    for name, lanes in etc1_fast_dropout_compositions():
        if name.endswith("_p1"):
            probe, partner = lanes[1], lanes[0]
            out.append(latin_motif(probe, partner, 1))
            out.append(latin_motif(probe, partner, 3))
    return out


def word_motifs(codec):
    probes, partners = word_probes(codec), word_partners(codec)
    rnd = random_words(codec, 16, 99 + codec)
    out = [list(rnd)]
    for pw in probes.values():
        out.append(latin_motif(pw, pw, 0))
        out.append(latin_motif(list(rnd)[0], pw, 1))
        for qw in partners.values():
            out.append(latin_motif(pw, qw, 1))
            out.append(latin_motif(pw, qw, 3))
    return out
