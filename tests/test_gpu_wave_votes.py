"""GPU tier (-m gpu): the kernels' wave votes with lanes that disagree, on the MI355X.

The probe and partner blocks of tests/wave_cases.py, laid out as textures of 4 x 4-block motifs (wave_cases.region_grid)
so that every aligned wave layout the library ships sees each composition's mix, whatever the launch form's lane -> block
map.  Every output block must equal the oracle's.  The exact-count and +/-1 threshold waves run in the host tier
(tests/test_wave_votes_host.py); which waves a motif makes busy / calm / mixed follows from the launch code (16 x 4-block
ETC1 waves inside 16 x 16-block tiles, 256 x 1 or 2^k x (256 >> k) DXT tiles).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import ic_testlib as T
import mips_oracle as M
import wave_cases as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    import torch
    import ic_amd_loader
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    p = ic_amd_loader.load_package()
    assert p.lib().icamd_device_count() >= 1
    return p


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).copy()).cuda()


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().tobytes()


def _first_bad_block(got, want, bb):
    for i in range(0, len(want), bb):
        if got[i:i + bb] != want[i:i + bb]:
            return i // bb
    return None


def _texture(family, comps, regions_across=8):
    motifs = W.encoder_motifs(family) + (W.etc1_wave_motifs() if family == "etc" else [])
    return W.grid_image(W.region_grid(motifs, regions_across), comps)


def _encode_and_compare(pkg, codec, img, comps, swap=0, strategy=2):
    h, w = img.shape[:2]
    want = T.oracle_encode(codec, img, h, w, comps, swap, strategy, threads=16)
    got = _host(pkg.encode_device(codec, _dev(img), h, w, comps, swap_rb=bool(swap), etc_strategy=strategy))
    bad = _first_bad_block(got, want, 16 if codec == T.DXT5 else 8)
    assert bad is None, "block %d (row %d, column %d) differs" % (bad, bad // ((w + 3) // 4), bad % ((w + 3) // 4))


@pytest.mark.parametrize("codec,comps,swap", [(T.DXT1, 3, 0), (T.DXT1, 4, 1), (T.DXT5, 4, 0), (T.DXT5, 4, 1)])
@pytest.mark.parametrize("regions_across", [8, 2])  # 2048 px wide: 256 x 1 tiles; 512 px: the narrow kernels
def test_dxt_motifs_match_oracle(pkg, codec, comps, swap, regions_across):
    _encode_and_compare(pkg, codec, _texture("dxt", comps, regions_across), comps, swap)


@pytest.mark.parametrize("strategy", [0, 1, 2, 3])
@pytest.mark.parametrize("comps", [3, 4])
def test_etc1_motifs_match_oracle(pkg, strategy, comps):
    _encode_and_compare(pkg, T.ETC1, _texture("etc", comps), comps, 0, strategy)


def test_etc1_quad_and_one_lane_forms_match_oracle():
    """kSmallerError through the four-lanes-per-block form (threshold forced up, on the big texture) and the one-lane form
    (threshold 0, on a texture small enough for the quad form by default); the threshold is read once per process."""
    code = r"""
import os, sys, numpy as np, torch
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import ic_amd_loader, ic_testlib as T, wave_cases as W
pkg = ic_amd_loader.load_package()
bad = 0
motifs = W.encoder_motifs("etc") + W.etc1_wave_motifs()
for comps in (3, 4):
    for img in (W.grid_image(W.region_grid(motifs, 8), comps), W.grid_image(W.region_grid(motifs[::9], 2), comps)):
        h, w = img.shape[:2]
        out = pkg.encode_device(T.ETC1, torch.from_numpy(img.reshape(-1).copy()).cuda(), h, w, comps)
        torch.cuda.synchronize()
        bad += out.cpu().numpy().tobytes() != T.oracle_encode(T.ETC1, img, h, w, comps, threads=16)
print("BAD", bad)
""" % (T.ROOT, T.ROOT)
    for setting in ("0", str(1 << 40)):
        env = dict(os.environ, ICAMD_ETC1_QUAD_MAX_BLOCKS=setting)
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stdout.strip().endswith("BAD 0"), (setting, r.stdout[-300:], r.stderr[-800:])


@pytest.mark.parametrize("strategy", [2, 0])
def test_etc1_mip_chain_of_motifs_matches_oracle(pkg, strategy):
    import torch
    motifs = W.encoder_motifs("etc")[::5] + W.etc1_wave_motifs()
    img = W.grid_image(W.region_grid(motifs, 4), 3)
    h, w = img.shape[:2]
    _, views = pkg.encode_mips_device(T.ETC1, _dev(img), h, w, 3, levels=3, etc_strategy=strategy)
    torch.cuda.synchronize()
    for level, p in enumerate(M.pyramid(img, 3)):
        assert views[level].cpu().numpy()[0].tobytes() == M.oracle_encode(T.ETC1, p, 3, 0, strategy), level


# ---------------------------------------------------------------------------------------------------- block operations

FORMATS = {T.DXT1: (T.DXTC, T.RGB, 8), T.DXT5: (T.DXTC, T.RGBA, 16), T.ETC1: (T.ETC, T.RGB, 8)}


def _word_grid(codec, regions_across=2):
    grid = W.region_grid(W.word_motifs(codec), regions_across)
    return W.grid_words(grid), 4 * len(grid), 4 * len(grid[0])


@pytest.mark.parametrize("codec", [T.DXT1, T.DXT5, T.ETC1])
def test_decode_batch_of_motifs_matches_oracle(pkg, codec):
    """decode_device with three images per call: the catalogue's words, then two random grids of the same shape."""
    words, h, w = _word_grid(codec)
    rnd = [np.random.Generator(np.random.PCG64(i)).integers(0, 256, len(words), dtype=np.uint8).tobytes() for i in (1, 2)]
    images = [words] + rnd
    got = pkg.decode_device(codec, _dev(np.frombuffer(b"".join(images), np.uint8)), h, w, n_images=3)
    got = got.cpu().numpy()
    for i, b in enumerate(images):
        assert got[i].tobytes() == T.oracle_decode(codec, b, h, w).tobytes(), i


@pytest.mark.parametrize("codec,strategy", [(T.DXT1, 2), (T.DXT5, 2), (T.ETC1, 2), (T.ETC1, 0)])
def test_downsample_of_motifs_matches_oracle(pkg, codec, strategy):
    comp, fmt, _ = FORMATS[codec]
    words, h, w = _word_grid(codec)
    got = pkg.downsample_device(comp, fmt, _dev(np.frombuffer(words, np.uint8)).reshape(1, -1), h, w, etc_strategy=strategy)
    assert _host(got) == T.oracle_downsample(comp, fmt, words, h, w, strategy)


def test_transcode_device_of_motifs_matches_oracle(pkg):
    import torch
    words, _, _ = _word_grid(T.DXT1)
    d = _dev(np.frombuffer(words, np.uint8))
    st = pkg.lib().icamd_transcode_dxt1_to_etc1_device(d.data_ptr(), d.numel(), None)
    assert st == 0
    torch.cuda.synchronize()
    assert _host(d) == T.oracle_transcode(words)


PAD_CODE = r"""
import os, sys, numpy as np, torch
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import ic_amd_loader, ic_testlib as T, wave_cases as W
pkg = ic_amd_loader.load_package()
bad = 0
for codec, comp, fmt in ((T.ETC1, T.ETC, T.RGB), (T.DXT1, T.DXTC, T.RGB), (T.DXT5, T.DXTC, T.RGBA)):
    grid = W.region_grid(W.word_motifs(codec), 1)
    words = W.grid_words(grid)
    h, w = 4 * len(grid), 4 * len(grid[0])
    for strategy in ((2, 0) if codec == T.ETC1 else (2,)):
        for ph, pw in ((h + 8, w + 8), (h + 4, w), (h, w + 12)):
            src = torch.from_numpy(np.frombuffer(words, np.uint8).copy()).cuda().reshape(1, -1)
            out = pkg.pad_batch_device(comp, fmt, src, h, w, ph, pw, etc_strategy=strategy)
            torch.cuda.synchronize()
            bad += out.cpu().numpy()[0].tobytes() != T.oracle_pad(comp, fmt, words, h, w, ph, pw, strategy)
print("BAD", bad)
"""


@pytest.mark.parametrize("quad", ["0", "1"])
def test_pad_of_motifs_matches_oracle(quad):
    """Pad's border blocks re-encoded from the catalogue's words, one lane per pad block (ICAMD_PAD_BORDER_QUAD=0) and four
    (the default); the switch is read once per process."""
    env = dict(os.environ, ICAMD_PAD_BORDER_QUAD=quad)
    r = subprocess.run([sys.executable, "-c", PAD_CODE % (T.ROOT, T.ROOT)], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("BAD 0"), (quad, r.stdout[-300:], r.stderr[-800:])
