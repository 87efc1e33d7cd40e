"""GPU tier for the BC4 / BC5 (RGTC) extension (include/ic_amd.h, ICAMD_BC4): the HIP kernels through the C ABI and the
Python wrappers, every case against the definition computed with the oracle's DXT5 (tests/bc45_oracle.py)."""
import ctypes
import importlib

import numpy as np
import pytest

import bc45_oracle as B
import ic_testlib as T

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
    return torch.from_numpy(np.ascontiguousarray(np.frombuffer(bytes(buf), np.uint8)).copy()).to(dev)


def _encode(codec, flat, h, w, comps, dev, **kw):
    import torch
    out = pkg.encode_device(codec, _to_dev(flat, dev), h, w, comps, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("gen", sorted(B.GENERATORS))
def test_encode_every_shape_and_layout(dev, gen):
    for i, (h, w, pad) in enumerate(B.SHAPES):
        img = B.image(gen, h, w, 4, index=i)
        for codec, comps, swap in B.LAYOUTS:
            src = np.ascontiguousarray(img[..., :comps])
            got = _encode(codec, T.with_row_padding(src, pad).tobytes(), h, w, comps, dev, swap_rb=bool(swap),
                          row_stride_bytes=w * comps + pad)
            assert got.tobytes() == B.oracle_encode(codec, src, h, w, comps, swap), (gen, h, w, pad, codec, comps, swap)


@pytest.mark.parametrize("h,w,gh,gw", [(30, 30, 40, 48), (5, 3, 16, 16), (1, 1, 9, 13), (64, 61, 64, 64), (17, 33, 24, 48)])
def test_encode_padded_grid(dev, h, w, gh, gw):
    img = B.image("saturated", h, w, 4, index=h + w)
    for codec, comps, swap in B.LAYOUTS:
        src = np.ascontiguousarray(img[..., :comps])
        got = _encode(codec, src.tobytes(), h, w, comps, dev, swap_rb=bool(swap), grid_height=gh, grid_width=gw)
        assert got.tobytes() == B.oracle_encode(codec, src, h, w, comps, swap, gh=gh, gw=gw), (h, w, gh, gw, codec, comps)


def test_encode_every_endpoint_distance(dev):
    strip = B.every_range_strip()
    h, w = strip.shape
    rg = np.ascontiguousarray(np.stack([strip, strip[:, ::-1]], axis=-1))
    assert _encode(B.BC4, strip.tobytes(), h, w, 1, dev).tobytes() == B.oracle_encode(B.BC4, strip, h, w, 1)
    assert _encode(B.BC5, rg.tobytes(), h, w, 2, dev).tobytes() == B.oracle_encode(B.BC5, rg, h, w, 2)


@pytest.mark.parametrize("codec,comps", [(B.BC4, 1), (B.BC4, 2), (B.BC5, 2), (B.BC5, 4)])
def test_encode_batch_with_image_stride_and_odd_alignment(dev, codec, comps):
    # 3 images of 37 x 70, each in a slot larger than the image, the batch starting one byte into the buffer
    import torch
    h, w, n, pad = 37, 70, 3, 3
    stride = w * comps + pad
    slot = h * stride + 29
    buf = np.zeros(1 + n * slot, np.uint8)
    imgs = [B.image("mixed", h, w, comps, index=20 + i) for i in range(n)]
    for i, im in enumerate(imgs):
        buf[1 + i * slot:1 + i * slot + h * stride] = T.with_row_padding(im, pad)
    d = _to_dev(buf.tobytes(), dev)
    per = B.encoded_size(codec, h, w)
    out = torch.zeros(1 + n * per + 5, dtype=torch.uint8, device=dev)
    st = pkg.lib().icamd_encode_device(codec, 0, comps, 0, h, w, h, w, stride, n, slot, per, ctypes.c_void_p(d.data_ptr() + 1),
                                       ctypes.c_void_p(out.data_ptr() + 1), None)
    assert st == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got[0] == 0 and not got[1 + n * per:].any()
    for i, im in enumerate(imgs):
        assert got[1 + i * per:1 + (i + 1) * per].tobytes() == B.oracle_encode(codec, im, h, w, comps), i


def test_encode_many_images_are_chunked(dev):
    # 70 000 images of 4 x 8: more than one launch's 65 535 images in grid.z
    import torch
    h, w, n = 4, 8, 70000
    g = np.random.Generator(np.random.PCG64(99))
    imgs = g.integers(0, 256, size=(n, h, w), dtype=np.uint8)
    out = pkg.encode_device(pkg.BC4, torch.from_numpy(imgs).to(dev), h, w, 1, n_images=n)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for i in (0, 1, 65534, 65535, 65536, n - 1):
        assert got[i].tobytes() == B.oracle_encode(B.BC4, imgs[i], h, w, 1), i


def test_encode_16384_r8_single_image(dev):
    # one 16384^2 R8 image (256 MiB, 2^24 blocks, 2^12 lane-group tile rows): the first and the last block rows are checked
    import torch
    n = 16384
    g = np.random.Generator(np.random.PCG64(5))
    tail = g.integers(0, 256, size=(64, n), dtype=np.uint8)
    src = torch.zeros((n, n), dtype=torch.uint8, device=dev)
    src[-64:] = torch.from_numpy(tail).to(dev)
    src[:8] = torch.from_numpy(tail[:8]).to(dev)
    out = pkg.encode_device(pkg.BC4, src, n, n, 1)
    torch.cuda.synchronize()
    got = out.view(n // 4, n // 4, 8).cpu().numpy()
    assert got[-16:].tobytes() == B.oracle_encode(B.BC4, tail, 64, n, 1)
    assert got[:2].tobytes() == B.oracle_encode(B.BC4, tail[:8], 8, n, 1)
    # BC5 of the same rows as RG (twice the output bytes) through the decoder as well
    del src, out
    rg = torch.zeros((n, n, 2), dtype=torch.uint8, device=dev)
    rg[-64:] = torch.from_numpy(np.stack([tail, tail[::-1]], axis=-1)).to(dev)
    out = pkg.encode_device(pkg.BC5, rg, n, n, 2)
    torch.cuda.synchronize()
    assert out.view(n // 4, n // 4, 16)[-16:].cpu().numpy().tobytes() == \
        B.oracle_encode(B.BC5, np.stack([tail, tail[::-1]], axis=-1), 64, n, 2)
    dec = pkg.decode_device(pkg.BC5, out.view(-1), n, n)
    torch.cuda.synchronize()
    want = B.oracle_decode(B.BC5, out.view(n // 4, n // 4, 16)[-16:].cpu().numpy().tobytes(), 64, n)
    assert dec.view(n, n * 2)[-64:].cpu().numpy().tobytes() == want.tobytes()


def test_batch_sharded_on_one_device_twice(dev):
    import torch
    h, w = 61, 59
    for codec, comps in [(B.BC4, 1), (B.BC5, 2), (B.BC5, 4)]:
        imgs = [B.image("mixed", h, w, comps, index=40 + i) for i in range(3)]
        srcs = [torch.from_numpy(im.copy()).to(dev) for im in imgs]
        statuses, _, gathered = pkg.encode_batch_sharded_device(codec, srcs, h, w, comps, [0, 0], gather_device=0)
        assert statuses == [0, 0, 0]
        assert gathered.shape[1] == B.encoded_size(codec, h, w)
        for i, im in enumerate(imgs):
            assert gathered[i].cpu().numpy().tobytes() == B.oracle_encode(codec, im, h, w, comps), (codec, i)


@pytest.mark.parametrize("codec", [B.BC4, B.BC5])
def test_decode_random_words_and_encoder_output(dev, codec):
    import torch
    c = B.comps_out(codec)
    for i, (h, w, pad) in enumerate(B.SHAPES + [(256, 1024, 0), (64, 4096, 16)]):
        words = B.random_words(codec, h, w, seed=300 + i)
        got = pkg.decode_device(codec, _to_dev(words, dev), h, w, padding_bytes_per_row=pad)
        torch.cuda.synchronize()
        assert got.cpu().numpy().reshape(-1).tobytes() == B.oracle_decode(codec, words, h, w, pad).tobytes(), (h, w, pad)
        img = B.image("smooth", h, w, c, index=i)
        blocks = pkg.encode_device(codec, torch.from_numpy(img).to(dev), h, w, c)
        got = pkg.decode_device(codec, blocks.view(-1), h, w, padding_bytes_per_row=pad)
        torch.cuda.synchronize()
        assert got.cpu().numpy().reshape(-1).tobytes() == B.oracle_decode(codec, blocks.cpu().numpy().tobytes(), h, w, pad).tobytes()


def test_decode_batch(dev):
    import torch
    h, w, n = 33, 70, 5
    for codec in (B.BC4, B.BC5):
        per = B.encoded_size(codec, h, w)
        words = [B.random_words(codec, h, w, seed=500 + i) for i in range(n)]
        got = pkg.decode_device(codec, _to_dev(b"".join(words), dev), h, w, padding_bytes_per_row=2, n_images=n)
        torch.cuda.synchronize()
        for i in range(n):
            assert got[i].cpu().numpy().tobytes() == B.oracle_decode(codec, words[i], h, w, 2).tobytes(), (codec, i)
        assert len(words[0]) == per


def test_python_wrappers_end_to_end(dev):
    import torch
    h, w = 128, 260
    r8 = B.image("mixed", h, w, 1, index=1)
    bc4 = pkg.encode_device(pkg.BC4, torch.from_numpy(r8).to(dev), h, w, 1)
    rgba = B.image("mixed", h, w, 4, index=1)
    bc5 = pkg.encode_device(pkg.BC5, torch.from_numpy(rgba).to(dev), h, w, 4, swap_rb=True)
    torch.cuda.synchronize()
    assert bc4.shape == (1, pkg.encoded_size(pkg.BC4, h, w)) and bc5.shape == (1, pkg.encoded_size(pkg.BC5, h, w))
    assert bc4.cpu().numpy().tobytes() == B.oracle_encode(B.BC4, r8, h, w, 1)
    assert bc5.cpu().numpy().tobytes() == B.oracle_encode(B.BC5, rgba, h, w, 4, swap=1)
    r = pkg.decode_device(pkg.BC4, bc4.view(-1), h, w)
    rg = pkg.decode_device(pkg.BC5, bc5.view(-1), h, w)
    torch.cuda.synchronize()
    assert r.shape == (1, h * w) and rg.shape == (1, h * w * 2)
    assert rg.cpu().numpy().tobytes() == B.oracle_decode(B.BC5, bc5.cpu().numpy().tobytes(), h, w).tobytes()
    # the R channel of BC5 (from byte 2: swap) is the BC4 of that byte
    bc4_b = pkg.encode_device(pkg.BC4, torch.from_numpy(rgba).to(dev), h, w, 4, swap_rb=True)
    torch.cuda.synchronize()
    assert bc4_b.view(-1, 8).cpu().numpy().tobytes() == bc5.view(-1, 16)[:, :8].cpu().numpy().tobytes()
