"""CPU tier: the kernels' wave votes with lanes that disagree.

tests/host_emul/wave_emul.cc runs the shipping per-block functions (image-compression_amd/csrc/*_block.h) for up to 64
blocks as one lockstep wave of host threads, so wave_all / wave_count see real neighbours: a block that would take a
shortcut alone runs the general code when another lane vetoes it.  Every lane's bytes must still be the oracle's bytes for
that block alone.  The waves come from tests/wave_cases.py (probes at each vote's boundary, partners that veto them).
The emulator also checks that every lane reaches the same votes (lockstep); a violation fails the wave.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ic_testlib as T
import wave_cases as W

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, "host_emul")
CSRC = os.path.join(T.ROOT, "image-compression_amd", "csrc")

ETC1_FORMS = [(s, c) for s in (0, 1, 2, 3) for c in (3, 4)]


@pytest.fixture(scope="module")
def wave():
    so = os.path.join(EMUL_DIR, "libic_wave_emul.so")
    src = os.path.join(EMUL_DIR, "wave_emul.cc")
    deps = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".inc"))]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in deps):
        subprocess.check_call(["g++", "-O2", "-g", "-std=c++20", "-pthread", "-fPIC", "-shared",
                               "-DICAMD_HOST_EMULATION", "-DICAMD_EMUL_WAVE",
                               "-I" + CSRC, "-o", so, src])
    L = ctypes.CDLL(so)
    ci, vp = T.ci, T.vp
    for name, args in [("wemul_dxt", [ci, ci, ci, vp, vp]), ("wemul_etc1", [ci, ci, vp, vp]),
                       ("wemul_etc1_classify", [ci, vp, vp]), ("wemul_etc1_inst", [ci, ci, ci, ci, ci, vp, vp, vp]),
                       ("wemul_decode", [ci, ci, vp, vp]), ("wemul_downsample", [ci, ci, ci, vp, vp]),
                       ("wemul_transcode", [ci, vp, vp]), ("wemul_etc1_pad", [ci, ci, vp, vp, vp])]:
        getattr(L, name).restype = ci
        getattr(L, name).argtypes = args
    L.wemul_error.restype = ctypes.c_char_p
    L.so_path = so
    yield L
    T.assert_no_emul_violations(L, "test_wave_votes_host")


def _check(L, ok, what):
    if not ok:
        msg = L.wemul_error().decode()
        pytest.fail("%s: the wave broke lockstep: %s" % (what, msg))


def _blocks_bytes(codec):
    return 16 if codec == T.DXT5 else 8


def _oracle_blocks(codec, blocks, comps, swap=0, strategy=2):
    img = W.strip(blocks, comps)
    return T.oracle_encode(codec, img, 4, 4 * len(blocks), comps, swap, strategy)


def _emul_encode(L, codec, blocks, comps, swap=0, strategy=2):
    px = W.to_dwords(blocks, comps)
    n = len(blocks)
    out = np.zeros((n, 4 if codec == T.DXT5 else 2), np.uint32)
    if codec == T.ETC1:
        ok = L.wemul_etc1(strategy, n, px.ctypes.data, out.ctypes.data)
    else:
        ok = L.wemul_dxt(codec, swap, n, px.ctypes.data, out.ctypes.data)
    _check(L, ok, "encode codec %d" % codec)
    return out.tobytes()


def _assert_lanes(got, want, bb, name):
    if got != want:
        bad = [i for i in range(len(want) // bb) if got[i * bb:(i + 1) * bb] != want[i * bb:(i + 1) * bb]]
        pytest.fail("%s: lanes %s differ from the oracle (lane %d: got %s, want %s)"
                    % (name, bad[:8], bad[0], got[bad[0] * bb:(bad[0] + 1) * bb].hex(), want[bad[0] * bb:(bad[0] + 1) * bb].hex()))


def _run_encode(L, codec, comps, swap, strategy, comps_list):
    for name, blocks in comps_list:
        want = _oracle_blocks(codec, blocks, comps, swap, strategy)
        got = _emul_encode(L, codec, blocks, comps, swap, strategy)
        _assert_lanes(got, want, _blocks_bytes(codec), name)


# ---------------------------------------------------------------------------------------------------- encoders


@pytest.mark.parametrize("codec,comps,swap", [(T.DXT1, 3, 0), (T.DXT1, 4, 1), (T.DXT5, 4, 0), (T.DXT5, 4, 1)])
def test_dxt_compositions_match_oracle(wave, codec, comps, swap):
    _run_encode(wave, codec, comps, swap, 2, W.encoder_compositions("dxt"))


@pytest.mark.parametrize("strategy,comps", ETC1_FORMS)
def test_etc1_compositions_match_oracle(wave, strategy, comps):
    # every composition for kSmallerError on RGB888 and for kHeuristic (no searches: cheap); a quarter of them for the
    # single-partition strategies and RGBA8 sources (an emulated wave costs ~20 ms of thread switches per search)
    cases = W.encoder_compositions("etc")
    _run_encode(wave, T.ETC1, comps, 0, strategy, cases if (strategy, comps) in ((2, 3), (3, 3), (3, 4)) else cases[::4])


@pytest.mark.parametrize("strategy,comps", ETC1_FORMS)
def test_etc1_busy_and_three_quarter_rule(wave, strategy, comps):
    _run_encode(wave, T.ETC1, comps, 0, strategy, W.etc1_busy_compositions())


def test_etc1_compositions_classify_as_named(wave):
    """The busy / one-colour counts the classifier sees are the ones the composition names claim."""
    for name, blocks in W.etc1_busy_compositions():
        px = W.to_dwords(blocks, 3)
        flags = np.zeros(len(blocks), np.uint32)
        _check(wave, wave.wemul_etc1_classify(len(blocks), px.ctypes.data, flags.ctypes.data), name)
        n_const = int(((flags & 2) != 0).sum())
        n_busy = int(((flags == 1)).sum())
        if name.startswith("busy"):
            assert (n_const, n_busy) == (0, int(name[4:6])), name
        else:
            c, b = name.split("_")[:2]
            assert (n_const, n_busy) == (int(c[5:]), int(b[4:])), name


@pytest.mark.parametrize("strategy", [0, 1, 2])
def test_etc1_fast_shortcut_dropping_out_at_each_codeword(wave, strategy):
    _run_encode(wave, T.ETC1, 3, 0, strategy, W.etc1_fast_dropout_compositions())


INSTANTIATIONS = [(t, p, s, 2) for t in (False, True) for p in (False, True) for s in (False, True)] + \
                 [(t, p, True, st) for st in (0, 1) for t, p in ((True, False), (False, True))]


@pytest.mark.parametrize("tier,prune,skip_form,strategy", INSTANTIATIONS)
def test_etc1_instantiations_match_oracle(wave, tier, prune, skip_form, strategy):
    """Every <TIER, PRUNE, SKIP> form (kSmallerError; the shipping SKIP forms also for the single-partition strategies)
    on the compositions; SKIP forms with the one-colour lanes skipped (their bytes are replaced by the classifier, so only
    the searching lanes are compared)."""
    cases = W.encoder_compositions("etc")[::8] + W.etc1_busy_compositions() + W.etc1_fast_dropout_compositions()
    for name, blocks in cases:
        n = len(blocks)
        px = W.to_dwords(blocks, 3)
        skip = np.array([skip_form and W.is_one_colour(b) for b in blocks], np.uint8)
        out = np.zeros((n, 2), np.uint32)
        ok = wave.wemul_etc1_inst(int(tier), int(prune), int(skip_form), strategy, n, px.ctypes.data, skip.ctypes.data,
                                  out.ctypes.data)
        _check(wave, ok, name)
        want = np.frombuffer(_oracle_blocks(T.ETC1, blocks, 3, 0, strategy), np.uint32).reshape(n, 2)
        keep = skip == 0
        bad = np.nonzero(keep & (out != want).any(axis=1))[0]
        assert bad.size == 0, "%s: lanes %s differ" % (name, bad[:8].tolist())


def test_partial_waves_match_oracle(wave):
    """Waves with fewer than 64 lanes (the right / bottom edges of a texture): the absent lanes do not vote."""
    for name, blocks in W.encoder_compositions()[::29] + W.etc1_busy_compositions():
        for n in (1, 17, 63):
            sub = blocks[-n:]
            for codec, comps, strategy in ((T.DXT1, 3, 2), (T.DXT5, 4, 2), (T.ETC1, 3, 2), (T.ETC1, 4, 0)):
                want = _oracle_blocks(codec, sub, comps, 0, strategy)
                got = _emul_encode(wave, codec, sub, comps, 0, strategy)
                _assert_lanes(got, want, _blocks_bytes(codec), "%s[-%d:] codec %d" % (name, n, codec))


# ---------------------------------------------------------------------------------------------------- block operations


def _words(ws):
    return np.ascontiguousarray(np.stack([np.asarray(w, np.uint32) for w in ws]))


@pytest.mark.parametrize("codec", [T.DXT1, T.DXT5, T.ETC1])
def test_decode_compositions_match_oracle(wave, codec):
    for name, ws in W.word_compositions(codec):
        words = _words(ws)
        n = len(ws)
        out = np.zeros((n, 16), np.uint32)
        _check(wave, wave.wemul_decode(codec, n, words.ctypes.data, out.ctypes.data), name)
        comps = 4 if codec == T.DXT5 else 3
        # the oracle decodes the blocks as one block row
        img = T.oracle_decode(codec, words.tobytes(), 4, 4 * n).reshape(4, n, 4, comps).transpose(1, 0, 2, 3)
        got = out.view(np.uint8).reshape(n, 4, 4, 4)[..., :comps]
        bad = np.nonzero((got != img).reshape(n, -1).any(axis=1))[0]
        assert bad.size == 0, "%s: lanes %s differ" % (name, bad[:8].tolist())


def test_transcode_compositions_match_oracle(wave):
    for name, ws in W.word_compositions(T.DXT1):
        words = _words(ws)
        n = len(ws)
        out = np.zeros((n, 2), np.uint32)
        _check(wave, wave.wemul_transcode(n, words.ctypes.data, out.ctypes.data), name)
        _assert_lanes(out.tobytes(), T.oracle_transcode(words.tobytes()), 8, name)


def _downsample_source(ws, codec):
    """Lane i's 2 x 2 source blocks: the probe words of lane i (top left) with three neighbours from the wave."""
    n = len(ws)
    quads = [[ws[i], ws[(i + 1) % n], ws[(i + 7) % n], ws[(i + 13) % n]] for i in range(n)]
    return quads


@pytest.mark.parametrize("codec,fmt,strategy", [(T.DXT1, T.RGB, 2), (T.DXT5, T.RGBA, 2), (T.ETC1, T.RGB, 2),
                                                (T.ETC1, T.RGB, 0), (T.ETC1, T.RGB, 3)])
def test_downsample_compositions_match_oracle(wave, codec, fmt, strategy):
    comp = T.ETC if codec == T.ETC1 else T.DXTC
    for name, ws in W.word_compositions(codec)[::2]:
        quads = _downsample_source(ws, codec)
        n = len(quads)
        words = _words([w for q in quads for w in q])
        out = np.zeros((n, 4 if codec == T.DXT5 else 2), np.uint32)
        _check(wave, wave.wemul_downsample(codec, strategy, n, words.ctypes.data, out.ctypes.data), name)
        # the same quads as one 8 x 8 n texture: block row 0 = tops, row 1 = bottoms
        grid = [[None] * (2 * n) for _ in range(2)]
        for i, q in enumerate(quads):
            grid[0][2 * i], grid[0][2 * i + 1], grid[1][2 * i], grid[1][2 * i + 1] = q
        src = _words([w for row in grid for w in row]).tobytes()
        want = T.oracle_downsample(comp, fmt, src, 8, 8 * n, strategy)
        _assert_lanes(out.tobytes(), want, _blocks_bytes(codec), name)


@pytest.mark.parametrize("strategy", [0, 1, 2, 3])
def test_etc1_pad_compositions_match_oracle(wave, strategy):
    """Pad's re-encoded border blocks (one lane per pad block), column and row kinds mixed in one wave with corners."""
    for name, ws in W.word_compositions(T.ETC1)[::2] + [("random", list(W.random_words(T.ETC1, 64, 5)))]:
        n = len(ws)
        words = _words(ws)
        # the oracle: a one-block-wide column of n blocks padded one block to the right (column kind) and n blocks in a
        # row padded one block down (row kind); the corner of a single block
        col = T.oracle_pad(T.ETC, T.RGB, words.tobytes(), 4 * n, 4, 4 * n, 8, strategy)
        row = T.oracle_pad(T.ETC, T.RGB, words.tobytes(), 4, 4 * n, 8, 4 * n, strategy)
        want_col = np.frombuffer(col, np.uint32).reshape(n, 2, 2)[:, 1]
        want_row = np.frombuffer(row, np.uint32).reshape(2, n, 2)[1]
        kinds = np.array([i % 3 for i in range(n)], np.uint8)
        out = np.zeros((n, 2), np.uint32)
        _check(wave, wave.wemul_etc1_pad(strategy, n, words.ctypes.data, kinds.ctypes.data, out.ctypes.data), name)
        for i in range(n):
            if kinds[i] == 0:
                assert (out[i] == want_col[i]).all(), (name, i, "column")
            elif kinds[i] == 1:
                assert (out[i] == want_row[i]).all(), (name, i, "row")
            else:
                corner = T.oracle_pad(T.ETC, T.RGB, words[i].tobytes(), 4, 4, 8, 8, strategy)
                assert (out[i] == np.frombuffer(corner, np.uint32).reshape(2, 2, 2)[1, 1]).all(), (name, i, "corner")


# ---------------------------------------------------------------------------------------------------- random waves


RANDOM_FORMS = [(T.DXT1, 3, 0, 2), (T.DXT1, 4, 1, 2), (T.DXT5, 4, 0, 2), (T.ETC1, 3, 0, 0), (T.ETC1, 3, 0, 1),
                (T.ETC1, 3, 0, 2), (T.ETC1, 4, 0, 2), (T.ETC1, 3, 0, 3)]


@pytest.mark.parametrize("codec,comps,swap,strategy", RANDOM_FORMS)
def test_random_waves_match_oracle(wave, codec, comps, swap, strategy):
    """Seeded waves of 64 blocks drawn from the catalogue and from soak_image content."""
    rng = np.random.Generator(np.random.PCG64(4242 + 10 * codec + strategy))
    pool = list(W.encoder_probes().values()) + list(W.encoder_partners().values())
    n_waves = 300 if codec != T.ETC1 else 120
    for k in range(n_waves):
        img = T.soak_image(rng, 16, 64, 4)
        soak = [W.block_from(img, by, bx) for by in range(4) for bx in range(16)]
        n_cat = int(rng.integers(0, 65))
        lanes = [pool[int(rng.integers(0, len(pool)))] if i < n_cat else soak[i] for i in range(64)]
        lanes = [lanes[i] for i in rng.permutation(64)]
        want = _oracle_blocks(codec, lanes, comps, swap, strategy)
        got = _emul_encode(wave, codec, lanes, comps, swap, strategy)
        _assert_lanes(got, want, _blocks_bytes(codec), "random wave %d" % k)
