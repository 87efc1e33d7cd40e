"""GPU tier for the ETC2 RGBA8 extension (include/ic_amd.h, ICAMD_ETC2_RGBA8): the HIP kernels through the C ABI and the
Python wrappers, every case bit-exact against the numpy definition (tests/etc2_oracle.py)."""
import ctypes
import importlib

import numpy as np
import pytest

import bc45_oracle as B
import etc2_oracle as E
import ic_testlib as T

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("image-compression_amd")
C = E.ETC2_RGBA8


@pytest.fixture(scope="module")
def dev():
    import torch
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


def _to_dev(buf, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.frombuffer(bytes(buf), np.uint8)).copy()).to(dev)


def _encode(flat, h, w, dev, **kw):
    import torch
    out = pkg.encode_device(C, _to_dev(flat, dev), h, w, 4, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _stats(img, dec):
    d = img.astype(np.int64) - dec.astype(np.int64)
    return (d * d).sum(axis=(0, 1)), np.abs(d).max(axis=(0, 1))


@pytest.mark.parametrize("gen", sorted(B.GENERATORS))
def test_encode_every_shape_strategy_and_swap(dev, gen):
    for i, (h, w, pad) in enumerate(B.SHAPES):
        img = B.image(gen, h, w, 4, index=i)
        flat = T.with_row_padding(img, pad).tobytes()
        alpha = E.eac_encode(E.block_alphas(img[..., 3], h, w, h, w))  # (does not depend on strategy or swap)
        largest = h * w == max(s[0] * s[1] for s in B.SHAPES)
        for strategy in ((T.SMALLER_ERROR,) if largest else E.STRATEGIES):
            for swap in (0, 1):
                got = _encode(flat, h, w, dev, swap_rb=bool(swap), etc_strategy=strategy, row_stride_bytes=w * 4 + pad)
                assert got.tobytes() == E.oracle_encode(img, h, w, swap, strategy, alpha_words=alpha), (gen, h, w, pad, strategy, swap)


@pytest.mark.parametrize("h,w,gh,gw", [(30, 30, 40, 48), (5, 3, 16, 16), (1, 1, 9, 13), (64, 61, 64, 64), (17, 33, 24, 48)])
def test_encode_padded_grid(dev, h, w, gh, gw):
    img = B.image("saturated", h, w, 4, index=h + w)
    for strategy in E.STRATEGIES:
        got = _encode(img.tobytes(), h, w, dev, etc_strategy=strategy, grid_height=gh, grid_width=gw)
        assert got.tobytes() == E.oracle_encode(img, h, w, 0, strategy, gh=gh, gw=gw), (h, w, gh, gw, strategy)


def test_colour_half_is_the_etc1_kernels_output(dev):
    import torch
    h, w = 61, 59
    img = B.image("mixed", h, w, 4, index=5)
    d = _to_dev(img.tobytes(), dev)
    for strategy in E.STRATEGIES:
        for gh, gw in ((h, w), (72, 64)):
            two = pkg.encode_device(C, d, h, w, 4, etc_strategy=strategy, grid_height=gh, grid_width=gw)
            one = pkg.encode_device(pkg.ETC1, d, h, w, 4, etc_strategy=strategy, grid_height=gh, grid_width=gw)
            torch.cuda.synchronize()
            assert (two.cpu().numpy().reshape(-1, 16)[:, 8:] == one.cpu().numpy().reshape(-1, 8)).all(), (strategy, gh, gw)


def test_encode_every_range(dev):
    strip = E.every_range_strip()
    h, w = strip.shape
    img = B.image("noise", h, w, 4, index=77)
    img[..., 3] = strip
    assert _encode(img.tobytes(), h, w, dev, etc_strategy=T.HEURISTIC).tobytes() == E.oracle_encode(img, h, w, 0, T.HEURISTIC)


def test_encode_batch_with_image_stride_and_odd_alignment(dev):
    # 3 images of 37 x 70, each in a slot larger than the image, the batch starting one byte into the buffer
    import torch
    h, w, n, pad = 37, 70, 3, 3
    stride = w * 4 + pad
    slot = h * stride + 29
    buf = np.zeros(1 + n * slot, np.uint8)
    imgs = [B.image("mixed", h, w, 4, index=20 + i) for i in range(n)]
    for i, im in enumerate(imgs):
        buf[1 + i * slot:1 + i * slot + h * stride] = T.with_row_padding(im, pad)
    d = _to_dev(buf.tobytes(), dev)
    per = E.encoded_size(h, w)
    out = torch.zeros(1 + n * per + 5, dtype=torch.uint8, device=dev)
    st = pkg.lib().icamd_encode_device(C, 2, 4, 0, h, w, h, w, stride, n, slot, per, ctypes.c_void_p(d.data_ptr() + 1),
                                       ctypes.c_void_p(out.data_ptr() + 1), None)
    assert st == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got[0] == 0 and not got[1 + n * per:].any()
    for i, im in enumerate(imgs):
        assert got[1 + i * per:1 + (i + 1) * per].tobytes() == E.oracle_encode(im, h, w), i


def test_encode_many_images_are_chunked(dev):
    # 70 000 images of 4 x 8: more than one launch's 65 535 images in grid.z
    import torch
    h, w, n = 4, 8, 70000
    g = np.random.Generator(np.random.PCG64(99))
    imgs = g.integers(0, 256, size=(n, h, w, 4), dtype=np.uint8)
    out = pkg.encode_device(C, torch.from_numpy(imgs).to(dev), h, w, 4, n_images=n)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for i in (0, 1, 65534, 65535, 65536, n - 1):
        assert got[i].tobytes() == E.oracle_encode(imgs[i], h, w), i


def test_wave_whose_lanes_disagree(dev):
    # one launch, one wave (16 x 4 blocks): flat blocks, R = 255 blocks and blocks at both multiplier clamps interleaved per
    # lane, on flat, busy and one-colour colour content -- the search's wave-uniform exit (every lane at sse 0) must not fire
    # for a lane that still searches, and the colour half's votes see lanes that disagree
    g = np.random.Generator(np.random.PCG64(T.SEED0 + 9400))
    h, w = 16, 64
    img = np.zeros((h, w, 4), np.uint8)
    for by in range(4):
        for bx in range(16):
            lane = by * 16 + bx
            kind = lane % 4
            if kind == 0:    # flat alpha (m0 clamps up to 1), one colour
                a = np.full((4, 4), int(g.integers(0, 256)))
                rgb = np.broadcast_to(g.integers(0, 256, 3), (4, 4, 3))
            elif kind == 1:  # R = 255 (m0 = 9 .. 15: the upper clamp for the narrow tables)
                a = g.integers(0, 256, (4, 4))
                a[0, 0], a[3, 3] = 0, 255
                rgb = g.integers(0, 256, (4, 4, 3))
            elif kind == 2:  # R of a few units: m0 = 1 after clamping, m - 1 clamps again
                lo = int(g.integers(0, 250))
                a = lo + g.integers(0, 6, (4, 4))
                rgb = 100 + g.integers(0, 40, (4, 4, 3))
            else:            # only 0 and 255
                a = g.integers(0, 2, (4, 4)) * 255
                rgb = g.integers(0, 2, (4, 4, 3)) * 255
            img[by * 4:by * 4 + 4, bx * 4:bx * 4 + 4, :3] = rgb
            img[by * 4:by * 4 + 4, bx * 4:bx * 4 + 4, 3] = a
    for strategy in E.STRATEGIES:
        assert _encode(img.tobytes(), h, w, dev, etc_strategy=strategy).tobytes() == E.oracle_encode(img, h, w, 0, strategy), strategy


@pytest.mark.parametrize("swap", [0, 1])
def test_decode_metric_and_decode_then_compare_agree(dev, swap):
    import torch
    for i, (h, w, pad) in enumerate(B.SHAPES[:-1]):
        words = E.random_words(h, w, seed=400 + i)
        got = pkg.decode_device(C, _to_dev(words, dev), h, w, swap_rb=bool(swap), padding_bytes_per_row=pad)
        torch.cuda.synchronize()
        assert got.cpu().numpy().tobytes() == E.oracle_decode(words, h, w, swap, pad).tobytes(), (h, w, pad)
        # the library's own blocks: decode, and the metric against numpy on the oracle's decode, exactly
        img = B.image("mixed", h, w, 4, index=40 + i)
        flat = T.with_row_padding(img, pad)
        d_src = _to_dev(flat.tobytes(), dev)
        blocks = pkg.encode_device(C, d_src, h, w, 4, row_stride_bytes=w * 4 + pad)
        sse, mx = pkg.measure_error_device(C, d_src, blocks.reshape(-1), h, w, 4, swap_rb=bool(swap), row_stride_bytes=w * 4 + pad)
        dec = pkg.decode_device(C, blocks.reshape(-1), h, w, swap_rb=bool(swap))
        torch.cuda.synchronize()
        want = E.oracle_decode(blocks.cpu().numpy().tobytes(), h, w, swap).reshape(h, w, 4)
        assert (dec.cpu().numpy().reshape(h, w, 4) == want).all()
        want_sse, want_max = _stats(img, want)
        assert (sse[0].cpu().numpy() == want_sse).all() and (mx[0].cpu().numpy() == want_max).all(), (h, w, pad)


def test_metric_on_a_padded_grid_and_a_batch(dev):
    import torch
    h, w, gh, gw, n = 30, 30, 40, 48, 3
    imgs = np.stack([B.image("saturated", h, w, 4, index=60 + i) for i in range(n)])
    d = torch.from_numpy(imgs.reshape(-1)).to(dev)
    blocks = pkg.encode_device(C, d, h, w, 4, grid_height=gh, grid_width=gw, n_images=n)
    sse, mx = pkg.measure_error_device(C, d, blocks.reshape(-1), h, w, 4, grid_height=gh, grid_width=gw, n_images=n)
    torch.cuda.synchronize()
    for i in range(n):
        grid = np.frombuffer(blocks[i].cpu().numpy().tobytes(), np.uint8).reshape((gh + 3) // 4, (gw + 3) // 4, 16)
        own = grid[:(h + 3) // 4, :(w + 3) // 4].tobytes()
        want_sse, want_max = _stats(imgs[i], E.oracle_decode(own, h, w).reshape(h, w, 4))
        assert (sse[i].cpu().numpy() == want_sse).all() and (mx[i].cpu().numpy() == want_max).all(), i


def test_unassigned_codec_is_rejected_with_a_device(dev):
    import torch
    src = torch.zeros(8 * 8 * 4, dtype=torch.uint8, device=dev)
    dst = torch.zeros(64, dtype=torch.uint8, device=dev)
    for codec in (7, 15, 17):
        st = pkg.lib().icamd_encode_device(codec, 2, 4, 0, 8, 8, 8, 8, 32, 1, 0, 0, ctypes.c_void_p(src.data_ptr()),
                                           ctypes.c_void_p(dst.data_ptr()), None)
        assert st == -4, codec


def test_encode_and_decode_under_stream_capture(dev):
    # one encode + decode captured into a graph (a single chain of nodes: no parallel branches), replayed once
    import torch
    h, w = 61, 59
    img = B.image("mixed", h, w, 4, index=90)
    src = _to_dev(img.tobytes(), dev)
    per = E.encoded_size(h, w)
    blocks = torch.zeros((1, per), dtype=torch.uint8, device=dev)
    pixels = torch.zeros(h * w * 4, dtype=torch.uint8, device=dev)
    lib = pkg.lib()

    def run(stream):
        assert lib.icamd_encode_device(C, 2, 4, 0, h, w, h, w, w * 4, 1, 0, 0, ctypes.c_void_p(src.data_ptr()),
                                       ctypes.c_void_p(blocks.data_ptr()), ctypes.c_void_p(stream)) == 0
        assert lib.icamd_decode_device(C, 0, h, w, 0, 1, 0, 0, ctypes.c_void_p(blocks.data_ptr()),
                                       ctypes.c_void_p(pixels.data_ptr()), ctypes.c_void_p(stream)) == 0

    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # (the kernels' first launch loads their code: not under capture)
        run(s.cuda_stream)
    s.synchronize()
    blocks.zero_()
    pixels.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            run(torch.cuda.current_stream().cuda_stream)
    graph.replay()
    torch.cuda.synchronize()
    want = E.oracle_encode(img, h, w)
    assert blocks.cpu().numpy().tobytes() == want
    assert pixels.cpu().numpy().tobytes() == E.oracle_decode(want, h, w).tobytes()
