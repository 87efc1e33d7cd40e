"""GPU tier for the DXT5 -> ETC2 RGBA8 transcode (include/ic_amd.h, icamd_transcode_dxt5_to_etc2_rgba8): the HIP
kernel through the C ABI and the Python wrappers, every case byte for byte against the definition (tests/transcode5_oracle.py)
and against the route it replaces, the library's own DXT5 decode followed by its ETC2 RGBA8 encode."""
import ctypes
import importlib

import numpy as np
import pytest

import bc45_oracle as B
import transcode5_oracle as X

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("image-compression_amd")


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


def _first_bad_block(got, want):
    for i in range(0, len(want), 16):
        if got[i:i + 16] != want[i:i + 16]:
            return i // 16
    return None


@pytest.mark.parametrize("n,tail", [(1, 0), (63, 0), (64, 0), (65, 0), (257, 0), (4096 + 37, 0), (65, 8)])
def test_device_form_matches_definition(dev, n, tail):
    src, want = X.pool_blocks(n, bytes(range(200, 200 + tail)))
    d = _to_dev(src, dev)
    assert pkg.transcode_dxt5_to_etc2_rgba8_device(d) is d  # in place
    got = _host(d)
    assert len(got) == 16 * n + tail and got[16 * n:] == src[16 * n:]
    assert got == want, "block %r differs" % _first_bad_block(got, want)


@pytest.mark.parametrize("h,w", [(64, 64), (256, 128)])
def test_device_form_equals_decode_then_encode(dev, h, w):
    img = B.image("mixed", h, w, 4, index=h + w)
    dxt5 = pkg.encode_device(pkg.DXT5, _to_dev(img.tobytes(), dev), h, w, 4).reshape(-1)
    pixels = pkg.decode_device(pkg.DXT5, dxt5, h, w).reshape(-1)
    route = _host(pkg.encode_device(pkg.ETC2_RGBA8, pixels, h, w, 4, etc_strategy=pkg.ETC_HEURISTIC))
    work = dxt5.clone()
    pkg.transcode_dxt5_to_etc2_rgba8_device(work)
    got = _host(work)
    assert got == route, "block %r differs" % _first_bad_block(got, route)


def test_waves_whose_lanes_disagree(dev):
    # one launch of 3 x 64 + 5 blocks, one wave per workgroup: a wave of flat alpha alone (every lane at sse 0 after the first
    # candidates: the wave leaves the search), a wave alternating flat and noisy blocks and a wave with a single noisy lane (the
    # exit must not be taken for the lanes that still search), and the partial last wave
    sets = X.block_sets()
    flat, noisy = sets["flat_alpha"], sets["random"]
    assert flat.shape[0] >= 64 + 32
    w0 = flat[:64]
    w1 = np.empty((64, 16), np.uint8)
    w1[0::2], w1[1::2] = flat[64:96], noisy[:32]
    w2 = flat[:64].copy()
    w2[37] = noisy[40]
    tail = np.stack([noisy[50], flat[3], noisy[51], noisy[52], flat[4]])
    src = np.concatenate([w0, w1, w2, tail]).tobytes()
    want = X.oracle_transcode5(src)
    got = _host(pkg.transcode_dxt5_to_etc2_rgba8_device(_to_dev(src, dev)))
    assert got == want, "block %r differs" % _first_bad_block(got, want)


def test_host_form_matches_definition():
    src, want = X.pool_blocks(1000, b"\x07\x08\x09")
    assert pkg.transcode_dxt5_to_etc2_rgba8_host(src) == want


def test_misaligned_device_pointer_is_refused_with_a_device(dev):
    import torch
    d = torch.zeros(64, dtype=torch.uint8, device=dev)
    st = pkg.lib().icamd_transcode_dxt5_to_etc2_rgba8_device(ctypes.c_void_p(d.data_ptr() + 8), 32, None)
    assert st == -4 and not _host(d).strip(b"\0")


@pytest.mark.parametrize("name", ["flat_alpha", "zero_255_only", "encoded_mixed", "random"])
def test_result_decodes_and_the_metric_judges_it(dev, name):
    import torch
    blocks = X.block_sets()[name][:96]
    n = blocks.shape[0]
    d = _to_dev(blocks.tobytes(), dev)
    pixels = pkg.decode_device(pkg.DXT5, d, 4, 4 * n).reshape(-1)  # what the DXT5 blocks mean
    pkg.transcode_dxt5_to_etc2_rgba8_device(d)
    dec = pkg.decode_device(pkg.ETC2_RGBA8, d, 4, 4 * n)
    assert dec is not None
    sse, mx = pkg.measure_error_device(pkg.ETC2_RGBA8, pixels, d, 4, 4 * n, 4)
    torch.cuda.synchronize()
    sse, mx = sse[0].cpu().numpy(), mx[0].cpu().numpy()
    # the metric's figures are those of the decoded pixels
    diff = dec.cpu().numpy().reshape(4, 4 * n, 4).astype(np.int64) - pixels.cpu().numpy().reshape(4, 4 * n, 4)
    assert (sse == (diff * diff).sum(axis=(0, 1))).all() and (mx == np.abs(diff).max(axis=(0, 1))).all()
    assert (sse >= 0).all() and (sse <= 16 * n * 255 ** 2).all() and (mx <= 255).all()
    if name in ("flat_alpha", "zero_255_only"):  # flat and 0 / 255 alpha is reproduced exactly
        assert mx[3] == 0 and sse[3] == 0


def test_transcode_under_stream_capture(dev):
    # one transcode of 4096 blocks captured on a single stream (one node, no branches), replayed once
    import torch
    src, want = X.pool_blocks(4096)
    clean = _to_dev(src, dev)
    work = clean.clone()
    lib = pkg.lib()

    def run(stream):
        assert lib.icamd_transcode_dxt5_to_etc2_rgba8_device(ctypes.c_void_p(work.data_ptr()), work.numel(),
                                                             ctypes.c_void_p(stream)) == 0

    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # (the kernel's first launch loads its code: not under capture)
        run(s.cuda_stream)
    s.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            run(torch.cuda.current_stream().cuda_stream)
    work.copy_(clean)  # the capture ran nothing: the replay transcodes DXT5 blocks, not its own output
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    got = _host(work)
    assert got == want, "block %r differs" % _first_bad_block(got, want)
