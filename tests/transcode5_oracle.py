"""DXT5 -> ETC2 RGBA8 transcode (include/ic_amd.h, icamd_transcode_dxt5_to_etc2_rgba8) as DEFINED in DESIGN.md 3.12: the ETC2
RGBA8 encoding (kHeuristic, no swap) of the pixels the DXT5 blocks decode to, built only from helpers the tests already trust --
the C oracle's DXT5 decoder and ETC1 encoder (tests/ic_testlib.py) and the numpy EAC definition (tests/etc2_oracle.py).

Also the block sets the tests share, and one POOL of them whose expected output is computed once per process: the transcode
works block by block, so the expected bytes of any selection of pool blocks are the same selection of the pool's expected blocks.
Shared by tests/test_transcode5_host.py (CPU tier), tests/test_gpu_transcode5.py (GPU tier) and scripts/bench_transcode5.py."""
import functools

import numpy as np

import bc45_oracle as B
import etc2_oracle as E
import ic_testlib as T


def oracle_transcode5(blocks):
    """Expected bytes: the n whole 16-byte blocks taken as a 4 x 4n image, then the untouched tail bytes."""
    b = np.frombuffer(bytes(blocks), np.uint8)
    n = b.size // 16
    if n == 0:
        return b.tobytes()
    px = T.oracle_decode(T.DXT5, b[:16 * n].tobytes(), 4, 4 * n).reshape(4, 4 * n, 4)
    return E.oracle_encode(px, 4, 4 * n, 0, T.HEURISTIC) + b[16 * n:].tobytes()


def _rng(index):
    return np.random.Generator(np.random.PCG64(T.SEED0 + 9500 + index))


def pack_codes(codes):
    """[n, 16] 3-bit codes, texel 4 y + x -> [n, 6] bytes, 48 little-endian bits."""
    c = np.asarray(codes, np.uint64)
    v = np.zeros(c.shape[0], np.uint64)
    for p in range(16):
        v |= c[:, p] << np.uint64(3 * p)
    return np.stack([((v >> np.uint64(8 * i)) & np.uint64(255)).astype(np.uint8) for i in range(6)], axis=1)


def unpack_codes(blocks):
    """[n, 16] uint8 DXT5 blocks -> [n, 16] codes, texel 4 y + x."""
    b = np.asarray(blocks, np.uint8).reshape(-1, 16)
    v = np.zeros(b.shape[0], np.uint64)
    for i in range(6):
        v |= b[:, 2 + i].astype(np.uint64) << np.uint64(8 * i)
    return np.stack([((v >> np.uint64(3 * p)) & np.uint64(7)).astype(np.int64) for p in range(16)], axis=1)


def alpha_palette(blocks):
    """[n, 8] decoded palette of the alpha words (the reference's truncating DecodeAlphaValues)."""
    b = np.asarray(blocks, np.uint8).reshape(-1, 16).astype(np.int64)
    a0, a1 = b[:, 0], b[:, 1]
    eight = np.stack([a0, a1] + [((7 - k) * a0 + k * a1) // 7 for k in range(1, 7)], axis=1)
    six = np.stack([a0, a1] + [((5 - k) * a0 + k * a1) // 5 for k in range(1, 5)] + [a0 * 0, a0 * 0 + 255], axis=1)
    return np.where((a0 > a1)[:, None], eight, six)


def _with_alpha(g, n, a0, a1, codes):
    """n blocks: random colour words, the given endpoints and codes."""
    b = g.integers(0, 256, size=(n, 16), dtype=np.uint8)
    b[:, 0], b[:, 1] = a0, a1
    b[:, 2:8] = pack_codes(codes)
    return b


def _encoded(gen, h, w, index):
    img = B.image(gen, h, w, 4, index=index)
    return np.frombuffer(T.oracle_encode(T.DXT5, img, h, w, 4), np.uint8).reshape(-1, 16).copy()


@functools.lru_cache(maxsize=None)
def block_sets(n_random=4096):
    """name -> [n, 16] uint8 DXT5 blocks."""
    sets = {}
    # any sixteen bytes: both alpha modes, colour words with c0 <= c1
    sets["random"] = _rng(0).integers(0, 256, size=(n_random, 16), dtype=np.uint8)
    # the DXT5 encoder's own output
    for i, gen in enumerate(("mixed", "noise", "saturated", "flat")):
        sets["encoded_" + gen] = _encoded(gen, 32, 48, 40 + i)
    g = _rng(1)
    n = 96
    a = g.integers(0, 256, size=n)
    sets["a0_eq_a1"] = _with_alpha(g, n, a, a, g.integers(0, 8, size=(n, 16)))
    # six-value mode, codes 6 and 7 alone: alphas 0 and 255 only (the first two blocks all 0 / all 255)
    a0 = g.integers(0, 200, size=n)
    codes = g.integers(6, 8, size=(n, 16))
    codes[0], codes[1] = 6, 7
    sets["zero_255_only"] = _with_alpha(g, n, a0, a0 + g.integers(0, 56, size=n), codes)
    # one code for the whole block: every code, both modes
    a0, a1 = g.integers(0, 256, size=n), g.integers(0, 256, size=n)
    sets["single_code"] = _with_alpha(g, n, a0, a1, np.repeat((np.arange(n) % 8)[:, None], 16, axis=1))
    # no texel uses an endpoint: lo / hi of the block lie inside the palette's range
    a0, a1 = g.integers(0, 256, size=n), g.integers(0, 256, size=n)
    top = np.where(a0 > a1, 8, 6)  # (six-value mode: the interpolated values only, not 0 / 255)
    sets["inner_codes"] = _with_alpha(g, n, a0, a1, 2 + g.integers(0, 1 << 30, size=(n, 16)) % (top - 2)[:, None])
    # flat alpha by equal endpoints and code 0 (a wave of these leaves the search at once), opaque included
    a = g.integers(0, 256, size=n)
    a[:4] = 255
    sets["flat_alpha"] = _with_alpha(g, n, a, a, np.zeros((n, 16), np.int64))
    return sets


@functools.lru_cache(maxsize=None)
def pool():
    """([n, 16] blocks of every set in a fixed shuffled order, [n, 16] expected ETC2 RGBA8 blocks)."""
    sets = block_sets()
    allb = np.concatenate([sets[k] for k in sorted(sets)], axis=0)
    allb = np.ascontiguousarray(allb[_rng(2).permutation(allb.shape[0])])
    want = np.frombuffer(oracle_transcode5(allb.tobytes()), np.uint8).reshape(-1, 16)
    allb.setflags(write=False)
    return allb, want


def pool_blocks(n, tail=b""):
    """(input bytes, expected bytes) of the first n pool blocks followed by `tail`, which stays as it is."""
    blocks, want = pool()
    assert n <= blocks.shape[0]
    return blocks[:n].tobytes() + tail, want[:n].tobytes() + tail


@functools.lru_cache(maxsize=None)
def set_oracle(name):
    """Expected [n, 16] blocks of one block set."""
    return np.frombuffer(oracle_transcode5(block_sets()[name].tobytes()), np.uint8).reshape(-1, 16)
