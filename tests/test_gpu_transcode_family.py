"""GPU tier for the DXT1 -> ETC2 RGB8, BC4 -> EAC R11 and BC5 -> EAC RG11 transcodes (include/ic_amd.h): the
HIP kernels through the C ABI, the Python wrappers and the C++ functions, every case byte for byte against the definition
(tests/transcode_family_oracle.py) and against the route each one replaces, the library's own decode followed by its encode."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

import bc45_oracle as B
import ic_testlib as T
import transcode_family_oracle as X

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("image-compression_amd")

DEVICE = {"dxt1": pkg.transcode_dxt1_to_etc2_rgb8_device, "bc4": pkg.transcode_bc4_to_eac_r11_device,
          "bc5": pkg.transcode_bc5_to_eac_rg11_device}
HOST = {"dxt1": pkg.transcode_dxt1_to_etc2_rgb8_host, "bc4": pkg.transcode_bc4_to_eac_r11_host,
        "bc5": pkg.transcode_bc5_to_eac_rg11_host}
SYMBOL = {"dxt1": "icamd_transcode_dxt1_to_etc2_rgb8_device", "bc4": "icamd_transcode_bc4_to_eac_r11_device",
          "bc5": "icamd_transcode_bc5_to_eac_rg11_device"}
# kind -> (source codec, target codec, components of the decoded image)
CODECS = {"dxt1": (pkg.DXT1, pkg.ETC2_RGB8, 3), "bc4": (pkg.BC4, pkg.EAC_R11, 1), "bc5": (pkg.BC5, pkg.EAC_RG11, 2)}


@pytest.fixture(scope="module")
def dev():
    import torch
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


def _to_dev(buf, dev):
    import torch
    return torch.from_numpy(np.frombuffer(bytes(buf), np.uint8).copy()).to(dev)


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().tobytes()


def _first_bad_block(got, want, block):
    for i in range(0, len(want), block):
        if got[i:i + block] != want[i:i + block]:
            return i // block
    return None


CASES = [(k, n, 0) for k in X.KINDS for n in (1, 63, 64, 65, 257, 4096 + 37)] + [("dxt1", 65, 7), ("bc4", 65, 3), ("bc5", 65, 15)]


@pytest.mark.parametrize("kind,n,tail", CASES)
def test_device_form_matches_definition(dev, kind, n, tail):
    block = X.BLOCK[kind]
    src, want = X.pool_blocks(kind, n, bytes(range(200, 200 + tail)))
    d = _to_dev(src, dev)
    assert DEVICE[kind](d) is d  # in place
    got = _host(d)
    assert len(got) == block * n + tail and got[block * n:] == src[block * n:]
    assert got == want, "block %r differs" % _first_bad_block(got, want, block)


@pytest.mark.parametrize("kind", X.KINDS)
@pytest.mark.parametrize("h,w", [(64, 64), (256, 128)])
def test_device_form_equals_decode_then_encode(dev, kind, h, w):
    src_codec, dst_codec, comps = CODECS[kind]
    img = B.image("mixed", h, w, comps, index=h + w)
    blocks = pkg.encode_device(src_codec, _to_dev(img.tobytes(), dev), h, w, comps).reshape(-1)
    pixels = pkg.decode_device(src_codec, blocks, h, w).reshape(-1)
    route = _host(pkg.encode_device(dst_codec, pixels, h, w, comps, etc_strategy=pkg.ETC_HEURISTIC))
    work = blocks.clone()
    DEVICE[kind](work)
    got = _host(work)
    assert got == route, "block %r differs" % _first_bad_block(got, route, X.BLOCK[kind])


def _waves(flat, noisy):
    """3 x 64 + 5 blocks, one or four waves per workgroup: a wave of `flat` blocks alone, a wave alternating flat and noisy blocks,
    a wave with a single noisy lane, and the partial last wave."""
    assert flat.shape[0] >= 64 + 32 and noisy.shape[0] >= 53
    w0 = flat[:64]
    w1 = np.empty_like(w0)
    w1[0::2], w1[1::2] = flat[64:96], noisy[:32]
    w2 = flat[:64].copy()
    w2[37] = noisy[40]
    tail = np.stack([noisy[50], flat[3], noisy[51], noisy[52], flat[4]])
    return np.concatenate([w0, w1, w2, tail])


@pytest.mark.parametrize("kind", ["bc4", "bc5"])
def test_waves_whose_lanes_disagree_about_the_search_exit(dev, kind):
    # the search leaves when every lane of the wave is at sse 0: flat blocks are there after the first candidates, noisy ones
    # never -- the exit must not be taken for the lanes that still search
    sets = X.block_sets(kind)
    flat = sets["flat_both" if kind == "bc5" else "flat"]
    src = _waves(flat, sets["random"]).tobytes()
    want = X.ORACLE[kind](src)
    got = _host(DEVICE[kind](_to_dev(src, dev)))
    assert got == want, "block %r differs" % _first_bad_block(got, want, X.BLOCK[kind])


def test_bc5_wave_with_one_channel_flat(dev):
    # the two searches of a BC5 lane exit on their own: a wave whose R words are all flat and whose G words are not, and the
    # other way round
    flat, noisy = X.bc4_sets()["flat"][:64], X.bc4_sets()["random"][:64]
    src = np.concatenate([np.concatenate([flat, noisy], axis=1), np.concatenate([noisy, flat], axis=1)]).tobytes()
    want = X.oracle_bc5(src)
    got = _host(pkg.transcode_bc5_to_eac_rg11_device(_to_dev(src, dev)))
    assert got == want, "block %r differs" % _first_bad_block(got, want, 16)


def test_dxt1_waves_whose_lanes_disagree_about_the_palette_mode(dev):
    # the DXT1 kernel inherits two wave-uniform shortcuts: the three-colour palette is only built where some lane has c0 < c1
    # (dxt_palette_planes), and the out-of-range base colours of the ETC1 word only where some lane has one.  Waves of
    # four-colour blocks alone, alternating with three-colour blocks that use black, with a single three-colour lane, partial
    sets = X.dxt1_sets()
    src = _waves(sets["c0_gt_c1"], sets["three_colour_black"]).tobytes()
    want = X.oracle_dxt1(src)
    got = _host(pkg.transcode_dxt1_to_etc2_rgb8_device(_to_dev(src, dev)))
    assert got == want, "block %r differs" % _first_bad_block(got, want, 8)


@pytest.mark.parametrize("kind", X.KINDS)
def test_host_form_matches_definition(kind):
    src, want = X.pool_blocks(kind, 1000, b"\x07\x08\x09")
    assert HOST[kind](src) == want


@pytest.mark.parametrize("kind", X.KINDS)
def test_misaligned_device_pointer_is_refused_with_a_device(dev, kind):
    import torch
    d = torch.zeros(64, dtype=torch.uint8, device=dev)
    for off in (4, X.BLOCK[kind] // 2):
        st = getattr(pkg.lib(), SYMBOL[kind])(ctypes.c_void_p(d.data_ptr() + off), 32, None)
        assert st == -4
    assert not _host(d).strip(b"\0")


METRIC_SETS = [("dxt1", "encoded_mixed"), ("dxt1", "random"), ("dxt1", "three_colour_black"), ("bc4", "flat"), ("bc4", "random"),
               ("bc4", "inner_narrow"), ("bc5", "flat_both"), ("bc5", "random")]


@pytest.mark.parametrize("kind,name", METRIC_SETS)
def test_result_decodes_and_the_metric_judges_it(dev, kind, name):
    import torch
    src_codec, dst_codec, comps = CODECS[kind]
    blocks = X.block_sets(kind)[name][:96]
    n = blocks.shape[0]
    d = _to_dev(blocks.tobytes(), dev)
    pixels = pkg.decode_device(src_codec, d, 4, 4 * n).reshape(-1)  # what the source blocks mean
    DEVICE[kind](d)
    dec = pkg.decode_device(dst_codec, d, 4, 4 * n)
    assert dec is not None
    sse, mx = pkg.measure_error_device(dst_codec, pixels, d, 4, 4 * n, comps)
    torch.cuda.synchronize()
    sse, mx = sse[0].cpu().numpy()[:comps], mx[0].cpu().numpy()[:comps]
    diff = dec.cpu().numpy().reshape(4, 4 * n, comps).astype(np.int64) - pixels.cpu().numpy().reshape(4, 4 * n, comps)
    assert (sse == (diff * diff).sum(axis=(0, 1))).all() and (mx == np.abs(diff).max(axis=(0, 1))).all()
    assert (sse <= 16 * n * 255 ** 2).all() and (mx <= 255).all()
    if name in ("flat", "flat_both"):  # a block of one value is reproduced exactly
        assert (mx == 0).all() and (sse == 0).all()


@pytest.mark.parametrize("kind", X.KINDS)
def test_transcode_under_stream_capture(dev, kind):
    # one transcode of 4096 blocks captured on a single stream (one node, no branches), replayed once
    import torch
    src, want = X.pool_blocks(kind, 4096)
    clean = _to_dev(src, dev)
    work = clean.clone()
    fn = getattr(pkg.lib(), SYMBOL[kind])

    def run(stream):
        assert fn(ctypes.c_void_p(work.data_ptr()), work.numel(), ctypes.c_void_p(stream)) == 0

    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # (the kernel's first launch loads its code: not under capture)
        run(s.cuda_stream)
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            run(torch.cuda.current_stream().cuda_stream)
    work.copy_(clean)  # the capture ran nothing: the replay transcodes source blocks, not its own output
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    got = _host(work)
    assert got == want, "block %r differs" % _first_bad_block(got, want, X.BLOCK[kind])


def test_cxx_functions_equal_the_c_abi(tmp_path):
    """TranscodeDxt1ToEtc2Rgb8 / TranscodeBc4ToEacR11 / TranscodeBc5ToEacRg11 of the C++ layer leave the bytes of the C ABI's
    host forms (tests/cxx_transcode/transcode_family_driver.cc, built here against the C++ classes)."""
    pkg_dir = os.path.join(T.ROOT, "image-compression_amd")
    exe = os.path.join(str(tmp_path), "transcode_family_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(pkg_dir, "cxx"), "-I" + os.path.join(T.ROOT, "include"),
                           "-o", exe, os.path.join(T.ROOT, "tests", "cxx_transcode", "transcode_family_driver.cc"),
                           "-L" + pkg_dir, "-limagecompression_amd", "-lic_amd", "-Wl,-rpath," + pkg_dir])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out = r.stdout.decode()
    assert r.returncode == 0, out + r.stderr.decode()
    assert out.count("OK ") == 3 and "BAD" not in out, out
