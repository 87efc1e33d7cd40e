"""DXT1 -> ETC2 RGB8, BC4 -> EAC R11 and BC5 -> EAC RG11 transcodes (include/ic_amd.h, icamd_transcode_dxt1_to_etc2_rgb8 /
_bc4_to_eac_r11 / _bc5_to_eac_rg11) as DEFINED in DESIGN.md 3.15: the target encoding of the pixels the source blocks decode to.
No codec maths of its own -- a composition of oracles the tests already trust:

* DXT1 decode: the C oracle (tests/ic_testlib.py); BC4 / BC5 decode: tests/bc45_oracle.py;
* ETC2 RGB8 encode (kHeuristic): tests/etc2_colour_oracle.py; EAC R11 / RG11 encode: tests/eac11_oracle.py.

Also the block sets the tests share and one shuffled POOL per transcode whose expected output is computed once per process (the
transcodes work block by block, so any selection of pool blocks expects the same selection of the pool's expected blocks).
Shared by tests/test_transcode_family_host.py (CPU tier), tests/test_gpu_transcode_family.py (GPU tier) and
scripts/bench_transcode_family.py."""
import functools

import numpy as np

import bc45_oracle as B
import eac11_oracle as R
import etc2_colour_oracle as C
import ic_testlib as T
import transcode5_oracle as X5

KINDS = ("dxt1", "bc4", "bc5")
BLOCK = {"dxt1": 8, "bc4": 8, "bc5": 16}
N_RANDOM = 1 << 14


def _split(blocks, block):
    b = np.frombuffer(bytes(blocks), np.uint8)
    n = b.size // block
    return b[:n * block], b[n * block:].tobytes(), n


def dxt1_pixels(blocks):
    """[4, 4 n, 3] RGB888 image of n DXT1 blocks laid side by side."""
    b, _, n = _split(blocks, 8)
    return T.oracle_decode(T.DXT1, b.tobytes(), 4, 4 * n).reshape(4, 4 * n, 3)


def oracle_dxt1(blocks, return_choice=False):
    """Expected bytes (and, on request, which blocks became planar): the whole blocks as a 4 x 4n image, then the tail."""
    b, tail, n = _split(blocks, 8)
    if n == 0:
        return (tail, np.zeros(0, bool)) if return_choice else tail
    out, planar = C.oracle_encode(dxt1_pixels(b), 4, 4 * n, 3, 0, T.HEURISTIC, return_choice=True)
    return (out + tail, planar) if return_choice else out + tail


def _oracle_bc(src_codec, dst_codec, blocks):
    block = B.block_bytes(src_codec)
    b, tail, n = _split(blocks, block)
    if n == 0:
        return tail
    comps = B.comps_out(src_codec)
    px = B.oracle_decode(src_codec, b.tobytes(), 4, 4 * n).reshape(4, 4 * n, comps)
    return R.oracle_encode(dst_codec, px, 4, 4 * n, comps) + tail


def oracle_bc4(blocks):
    return _oracle_bc(B.BC4, R.EAC_R11, blocks)


def oracle_bc5(blocks):
    return _oracle_bc(B.BC5, R.EAC_RG11, blocks)


ORACLE = {"dxt1": oracle_dxt1, "bc4": oracle_bc4, "bc5": oracle_bc5}


def _rng(index):
    return np.random.Generator(np.random.PCG64(T.SEED0 + 9700 + index))


def dxt1_endpoints(blocks):
    b = np.asarray(blocks, np.uint8).reshape(-1, 8).astype(np.int64)
    return b[:, 0] | b[:, 1] << 8, b[:, 2] | b[:, 3] << 8


def dxt1_indices(blocks):
    """[n, 16] 2-bit indices, texel 4 y + x."""
    b = np.asarray(blocks, np.uint8).reshape(-1, 8).astype(np.int64)
    bits = b[:, 4] | b[:, 5] << 8 | b[:, 6] << 16 | b[:, 7] << 24
    return np.stack([(bits >> (2 * p)) & 3 for p in range(16)], axis=1)


def _dxt1_words(c0, c1, idx):
    n = len(c0)
    b = np.zeros((n, 8), np.uint8)
    c0, c1 = np.asarray(c0, np.int64), np.asarray(c1, np.int64)
    b[:, 0], b[:, 1], b[:, 2], b[:, 3] = c0 & 255, c0 >> 8, c1 & 255, c1 >> 8
    bits = np.zeros(n, np.int64)
    for p in range(16):
        bits |= np.asarray(idx, np.int64)[:, p] << (2 * p)
    for i in range(4):
        b[:, 4 + i] = (bits >> (8 * i)) & 255
    return b


def _dxt1_encoded(gen, h, w, index):
    img = B.image(gen, h, w, 3, index=index)
    return np.frombuffer(T.oracle_encode(T.DXT1, img, h, w, 3), np.uint8).reshape(-1, 8).copy()


@functools.lru_cache(maxsize=None)
def dxt1_sets():
    """name -> [n, 8] uint8 DXT1 blocks."""
    sets = {"random": _rng(0).integers(0, 256, size=(N_RANDOM, 8), dtype=np.uint8)}
    g = _rng(1)
    n = 96
    a, b = g.integers(0, 65536, size=n), g.integers(0, 65536, size=n)
    hi, lo = np.maximum(a, b) | 1, np.minimum(a, b) & ~1  # never equal
    idx = g.integers(0, 4, size=(n, 16))
    sets["c0_gt_c1"] = _dxt1_words(hi, lo, idx)
    sets["c0_lt_c1"] = _dxt1_words(lo, hi, idx)
    sets["c0_eq_c1"] = _dxt1_words(a, a, idx)
    # one index for the whole block: every index, both modes
    sets["single_index"] = _dxt1_words(np.where(np.arange(n) & 4, hi, lo), np.where(np.arange(n) & 4, lo, hi),
                                       np.repeat((np.arange(n) % 4)[:, None], 16, axis=1))
    # three-colour blocks whose texels use index 3 (black): at least one texel each, some of them all black
    idx3 = g.integers(0, 4, size=(n, 16))
    idx3[np.arange(n), g.integers(0, 16, size=n)] = 3
    idx3[:4] = 3
    sets["three_colour_black"] = _dxt1_words(lo, hi, idx3)
    # nearby endpoints: the near-flat blocks of real textures, where the planar word's 6 / 7 / 6 bits can beat ETC1's 5 + 3
    near = a ^ g.integers(0, 2, size=n) ^ (g.integers(0, 2, size=n) << 5) ^ (g.integers(0, 2, size=n) << 11)
    sets["near_endpoints"] = _dxt1_words(np.maximum(a, near), np.minimum(a, near), idx)
    # the DXT1 encoder's own output.  The smooth generator carries 0..31 of per-pixel noise, which ETC1's luminance modifiers
    # follow and a plane cannot: at 32 x 48 its ramps are steep enough (21 to 32 per block) that the definition takes the planar
    # word for a few blocks and the ETC1 word for the rest (index 65 of the generator: two planar blocks of 96)
    sets["encoded_smooth"] = _dxt1_encoded("smooth", 32, 48, 65)
    sets["encoded_mixed"] = _dxt1_encoded("mixed", 64, 96, 61)
    return sets


def bc4_palette(words):
    """[n, 8] decoded palette of BC4 words."""
    b = np.zeros((np.asarray(words).reshape(-1, 8).shape[0], 16), np.uint8)
    b[:, :8] = np.asarray(words, np.uint8).reshape(-1, 8)
    return X5.alpha_palette(b)


def bc4_codes(words):
    b = np.zeros((np.asarray(words).reshape(-1, 8).shape[0], 16), np.uint8)
    b[:, :8] = np.asarray(words, np.uint8).reshape(-1, 8)
    return X5.unpack_codes(b)


def _bc4_words(a0, a1, codes):
    n = len(a0)
    b = np.zeros((n, 8), np.uint8)
    b[:, 0], b[:, 1] = a0, a1
    b[:, 2:] = X5.pack_codes(codes)
    return b


@functools.lru_cache(maxsize=None)
def bc4_sets():
    """name -> [n, 8] uint8 BC4 words."""
    sets = {"random": _rng(10).integers(0, 256, size=(N_RANDOM, 8), dtype=np.uint8)}
    g = _rng(11)
    n = 96
    a, b = g.integers(0, 256, size=n), g.integers(0, 256, size=n)
    hi, lo = np.maximum(a, b) | 1, np.minimum(a, b) & ~1
    codes = g.integers(0, 8, size=(n, 16))
    sets["a0_gt_a1"] = _bc4_words(hi, lo, codes)
    # six-value mode with the 0 and 255 entries in use: codes 6 and 7 on at least two texels of every block
    c6 = codes.copy()
    c6[:, 0], c6[:, 5] = 6, 7
    sets["a0_le_a1_0_255"] = _bc4_words(lo, hi, c6)
    sets["a0_eq_a1"] = _bc4_words(a, a, codes)
    # flat: one code everywhere, every code, both modes (a wave of these leaves the search at once)
    sets["flat"] = _bc4_words(np.where(np.arange(n) & 8, hi, lo), np.where(np.arange(n) & 8, lo, hi),
                              np.repeat((np.arange(n) % 8)[:, None], 16, axis=1))
    # no texel uses an extreme palette entry: lo / hi must come from the used entries only.  Eight-value mode: codes 2..7 (the
    # endpoints are the extremes); six-value mode: codes 0..5 (0 and 255 are).
    eight = (np.arange(n) & 1) == 0
    inner = np.where(eight[:, None], 2 + g.integers(0, 6, size=(n, 16)), g.integers(0, 6, size=(n, 16)))
    wide_hi, wide_lo = g.integers(160, 255, size=n), g.integers(1, 96, size=n)
    sets["inner_codes"] = _bc4_words(np.where(eight, wide_hi, wide_lo), np.where(eight, wide_lo, wide_hi), inner)
    # ... and narrowly: one or two neighbouring inner entries only, so the used range is a fraction of the palette's
    pick = np.where(eight, 2 + g.integers(0, 5, size=n), g.integers(2, 5, size=n))[:, None] + g.integers(0, 2, size=(n, 16))
    sets["inner_narrow"] = _bc4_words(np.where(eight, wide_hi, wide_lo), np.where(eight, wide_lo, wide_hi), pick)
    return sets


@functools.lru_cache(maxsize=None)
def bc5_sets():
    """name -> [n, 16] uint8 BC5 blocks: the BC4 sets paired with a shuffle of themselves, so the two channels differ in kind."""
    out = {}
    for i, (name, w) in enumerate(sorted(bc4_sets().items())):
        other = w[_rng(20 + i).permutation(w.shape[0])]
        out[name] = np.ascontiguousarray(np.concatenate([w, other], axis=1))
    allw = np.concatenate([bc4_sets()[k] for k in sorted(bc4_sets()) if k != "random"], axis=0)
    out["kinds_crossed"] = np.ascontiguousarray(np.concatenate([allw, allw[_rng(40).permutation(allw.shape[0])]], axis=1))
    out["flat_both"] = np.ascontiguousarray(np.concatenate([bc4_sets()["flat"], bc4_sets()["flat"][::-1]], axis=1))
    return out


SETS = {"dxt1": dxt1_sets, "bc4": bc4_sets, "bc5": bc5_sets}


def block_sets(kind):
    return SETS[kind]()


@functools.lru_cache(maxsize=None)
def set_oracle(kind, name):
    """Expected [n, block] blocks of one block set."""
    return np.frombuffer(ORACLE[kind](block_sets(kind)[name].tobytes()), np.uint8).reshape(-1, BLOCK[kind])


@functools.lru_cache(maxsize=None)
def dxt1_choice(name):
    """[n] bool: the blocks of a DXT1 set the oracle makes planar."""
    return oracle_dxt1(dxt1_sets()[name].tobytes(), return_choice=True)[1]


@functools.lru_cache(maxsize=None)
def pool(kind):
    """([n, block] blocks of every set in a fixed shuffled order -- of `random`, the first 4096 --, [n, block] expected)."""
    sets = block_sets(kind)
    parts, wants = [], []
    for k in sorted(sets):
        m = min(sets[k].shape[0], 4096)
        parts.append(sets[k][:m])
        wants.append(set_oracle(kind, k)[:m])
    allb, want = np.concatenate(parts, axis=0), np.concatenate(wants, axis=0)
    order = _rng(50 + KINDS.index(kind)).permutation(allb.shape[0])
    allb, want = np.ascontiguousarray(allb[order]), np.ascontiguousarray(want[order])
    allb.setflags(write=False)
    want.setflags(write=False)
    return allb, want


def pool_blocks(kind, n, tail=b""):
    """(input bytes, expected bytes) of the first n pool blocks followed by `tail`, which stays as it is."""
    blocks, want = pool(kind)
    assert n <= blocks.shape[0]
    return blocks[:n].tobytes() + tail, want[:n].tobytes() + tail
