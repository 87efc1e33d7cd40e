"""GPU tier of the fused mip chain (include/ic_amd.h, mip-chain section): every level of icamd_encode_mips_device against
the oracle's encode of the numpy pyramid (tests/mips_oracle.py), large cases against icamd_encode_device of that pyramid,
the pixel-pyramid entry against numpy, the host form, containers, graph capture and a seeded soak."""
import importlib

import numpy as np
import pytest

import bc45_oracle as B
import ic_testlib as T
import mips_oracle as M

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("image-compression_amd")


@pytest.fixture(scope="module")
def dev():
    import torch
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


def _img(h, w, comps, index=0, gen=T.s_mixed):
    return np.ascontiguousarray(gen(h, w, 4, index=index).reshape(h, w, 4)[..., :comps])


def _fused(codec, img, comps, dev, **kw):
    """(chain bytes of image 0, offsets) through encode_mips_device."""
    import torch
    h, w = img.shape[:2]
    d = torch.from_numpy(np.ascontiguousarray(img).reshape(-1).copy()).to(dev)
    flat, views = pkg.encode_mips_device(codec, d, h, w, comps, **kw)
    torch.cuda.synchronize()
    return flat.cpu().numpy(), [v.cpu().numpy() for v in views]


def _check_chain(codec, img, comps, dev, swap=0, strategy=T.SMALLER_ERROR, levels=None):
    h, w = img.shape[:2]
    flat, views = _fused(codec, img, comps, dev, swap_rb=bool(swap), etc_strategy=strategy, levels=levels)
    for l, p in enumerate(M.pyramid(img, levels)):
        want = M.oracle_encode(codec, p, comps, swap, strategy)
        assert views[l][0].tobytes() == want, (codec, comps, swap, strategy, h, w, l)


SMALL = [(1, 1), (2, 3), (5, 5), (13, 1000), (1000, 13), (4096, 1), (1, 4097), (61, 59), (130, 257)]


@pytest.mark.parametrize("codec,comps", M.LAYOUTS)
def test_every_codec_layout_and_swap(dev, codec, comps):
    for i, (h, w) in enumerate(SMALL):
        img = _img(h, w, comps, index=i)
        for swap in ((0, 1) if comps >= 3 else (0,)):
            _check_chain(codec, img, comps, dev, swap=swap)


@pytest.mark.parametrize("strategy", [0, 1, 2, 3, 7])
@pytest.mark.parametrize("comps", [3, 4])
def test_etc1_every_strategy(dev, strategy, comps):
    for i, (h, w) in enumerate([(5, 5), (61, 59), (200, 300), (1, 77)]):
        _check_chain(T.ETC1, _img(h, w, comps, index=10 + i), comps, dev, strategy=strategy)


def test_row_padding_and_unaligned_rgb888_rows(dev):
    import torch
    h, w, pad = 61, 59, 7
    for codec, comps in [(T.DXT1, 3), (T.ETC1, 3), (B.BC5, 3), (T.DXT5, 4), (B.BC4, 1)]:
        img = _img(h, w, comps, index=3)
        stride = w * comps + pad
        buf = np.zeros(1 + h * stride, np.uint8)  # one leading byte: rows start at odd addresses
        for y in range(h):
            buf[1 + y * stride:1 + y * stride + w * comps] = img[y].reshape(-1)
        d = torch.from_numpy(buf).to(dev)[1:]
        flat, views = pkg.encode_mips_device(codec, d, h, w, comps, row_stride_bytes=stride)
        torch.cuda.synchronize()
        for l, p in enumerate(M.pyramid(img)):
            assert views[l].cpu().numpy()[0].tobytes() == M.oracle_encode(codec, p, comps), (codec, comps, l)


def test_partial_levels(dev):
    import torch
    h, w = 300, 200
    for codec, comps in [(T.DXT1, 4), (T.ETC1, 3), (B.BC4, 2)]:
        img = _img(h, w, comps, index=4)
        d = torch.from_numpy(img.reshape(-1).copy()).to(dev)
        one = pkg.encode_mips_device(codec, d, h, w, comps, levels=1)[0]
        ref = pkg.encode_device(codec, d, h, w, comps)
        torch.cuda.synchronize()
        assert one.cpu().numpy().tobytes() == ref.cpu().numpy().tobytes()  # levels = 1 is icamd_encode_device
        for levels in (2, 3, 6, 7, 8):
            _check_chain(codec, img, comps, dev, levels=levels)


def _levels_by_encode_device(codec, img, comps, dev, levels=None):
    import torch
    out = []
    for p in M.pyramid(img, levels):
        lh, lw = p.shape[:2]
        e = pkg.encode_device(codec, torch.from_numpy(np.ascontiguousarray(p).reshape(-1)).to(dev), lh, lw, comps)
        out.append(e.cpu().numpy()[0].tobytes())
    return out


@pytest.mark.parametrize("codec,comps", [(T.DXT1, 4), (T.DXT1, 3), (T.DXT5, 4), (T.ETC1, 3), (B.BC4, 1), (B.BC5, 2)])
def test_4096_square(dev, codec, comps):
    img = _img(4096, 4096, comps, index=5)
    flat, views = _fused(codec, img, comps, dev)
    want = _levels_by_encode_device(codec, img, comps, dev)
    pyr = M.pyramid(img)
    for l in range(len(want)):
        assert views[l][0].tobytes() == want[l], (codec, comps, l)
        if l >= 5:  # the oracle itself on the small levels (both sides of the pass boundary at level 6)
            assert views[l][0].tobytes() == M.oracle_encode(codec, pyr[l], comps), (codec, comps, l)


def _big_img(h, w, seed):
    """A 16384^2 one-channel texture without s_mixed's int64 grids: a noise half and a smooth half."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 1), dtype=np.uint8)
    ramp = ((np.arange(w, dtype=np.uint32)[None, :] // 61 + np.arange(h, dtype=np.uint32)[:h // 2, None] // 37) & 255)
    img[:h // 2, :, 0] = ramp.astype(np.uint8)
    return img


def test_16384_square(dev):
    img = _big_img(16384, 16384, 6)
    flat, views = _fused(B.BC4, img, 1, dev)
    want = _levels_by_encode_device(B.BC4, img, 1, dev)
    pyr = M.pyramid(img)
    assert len(views) == 15
    for l in range(15):
        assert views[l][0].tobytes() == want[l], l
        if l >= 8:
            assert views[l][0].tobytes() == M.oracle_encode(B.BC4, pyr[l], 1), l


@pytest.mark.parametrize("n,size,codec,comps", [(64, 256, T.DXT1, 4), (64, 256, T.ETC1, 3), (16, 4096, B.BC4, 1),
                                                (16, 4096, T.DXT1, 3)])
def test_batches_with_non_tight_strides(dev, n, size, codec, comps):
    import torch
    h = w = size
    sis = h * w * comps + 160
    total, offs = pkg.mip_chain_size(codec, h, w)
    dis = total + 24
    src = np.zeros(n * sis, np.uint8)
    imgs = []
    for i in range(n):
        img = _img(h, w, comps, index=100 + i) if size <= 256 or i < 2 else np.roll(imgs[i % 2], 17 * i, axis=1)
        imgs.append(img)
        src[i * sis:i * sis + h * w * comps] = img.reshape(-1)
    d = torch.from_numpy(src).to(dev)
    flat, views = pkg.encode_mips_device(codec, d, h, w, comps, n_images=n, src_image_stride_bytes=sis, dst_image_stride_bytes=dis)
    torch.cuda.synchronize()
    got = flat.cpu().numpy()
    assert got.shape == (n, dis)
    for i in range(n):
        if size <= 256:
            want = M.oracle_chain(codec, imgs[i], comps)
        else:  # one image at a time through the same entry (single images are checked against the oracle above)
            one = _fused(codec, imgs[i], comps, dev)[0][0]
            want = one.tobytes()
            if i == 0:
                assert want == b"".join(_levels_by_encode_device(codec, imgs[0], comps, dev))
        assert got[i, :total].tobytes() == want, (codec, i)


@pytest.mark.parametrize("comps", [1, 2, 3, 4])
def test_pyramid_entry(dev, comps):
    import torch
    for i, (h, w) in enumerate([(1, 1), (2, 3), (13, 1000), (1000, 13), (257, 129), (2048, 2048), (3000, 17)]):
        img = _img(h, w, comps, index=20 + i)
        d = torch.from_numpy(img.reshape(-1).copy()).to(dev)
        flat, views = pkg.mip_pyramid_device(d, h, w, comps)
        torch.cuda.synchronize()
        pyr = M.pyramid(img)
        assert len(views) == len(pyr) - 1
        assert flat.cpu().numpy()[0, :pkg.mip_pyramid_size(comps, h, w)[0]].tobytes() == M.pyramid_bytes(img), (comps, h, w)
    # a batch with padded rows and non-tight strides, partial levels
    n, h, w, pad = 5, 300, 301, 9
    stride, sis = w * comps + pad, (w * comps + pad) * h + 40
    per, _ = pkg.mip_pyramid_size(comps, h, w, 5)
    src = np.zeros(n * sis, np.uint8)
    imgs = [_img(h, w, comps, index=40 + i) for i in range(n)]
    for i in range(n):
        for y in range(h):
            src[i * sis + y * stride:i * sis + y * stride + w * comps] = imgs[i][y].reshape(-1)
    flat, _ = pkg.mip_pyramid_device(torch.from_numpy(src).to(dev), h, w, comps, levels=5, n_images=n, row_stride_bytes=stride,
                                     src_image_stride_bytes=sis, dst_image_stride_bytes=per + 12)
    torch.cuda.synchronize()
    got = flat.cpu().numpy()
    for i in range(n):
        assert got[i, :per].tobytes() == M.pyramid_bytes(imgs[i], 5), i


def test_host_form_against_icamd_compress_per_level(dev):
    for compressor, fmt, comps in [(T.DXTC, T.RGB, 3), (T.DXTC, T.BGRA, 4), (T.ETC, T.RGB, 3)]:
        for h, w, pad in [(61, 59, 5), (300, 200, 0), (1, 9, 3)]:
            img = _img(h, w, comps, index=h)
            buf = _padded(img, pad) if pad else img.reshape(-1)
            got = pkg.compress_mips_host(compressor, fmt, buf, h, w, padding_bytes_per_row=pad)
            want = b"".join(pkg.compress_host(compressor, fmt, np.ascontiguousarray(p).reshape(-1), *p.shape[:2])
                            for p in M.pyramid(img))
            assert got == want, (compressor, fmt, h, w)
    assert pkg.compress_mips_host(T.ETC, T.RGBA, np.zeros(16 * 16 * 4, np.uint8), 16, 16) is None


def _padded(img, pad):
    h, w, c = img.shape
    out = np.zeros((h, w * c + pad), np.uint8)
    out[:, :w * c] = img.reshape(h, w * c)
    return out.reshape(-1)[:(h - 1) * (w * c + pad) + w * c]


@pytest.mark.parametrize("container,codec,comps", [(pkg.CONTAINER_KTX, T.ETC1, 3), (pkg.CONTAINER_DDS, T.DXT5, 4),
                                                   (pkg.CONTAINER_KTX, B.BC5, 2), (pkg.CONTAINER_DDS, T.DXT1, 3)])
def test_chain_as_container(dev, container, codec, comps):
    h, w = 200, 136
    img = _img(h, w, comps, index=8)
    flat, views = _fused(codec, img, comps, dev)
    fused = pkg.container_write(container, codec, h, w, [v[0].tobytes() for v in views])
    separate = pkg.container_write(container, codec, h, w, _levels_by_encode_device(codec, img, comps, dev))
    assert fused is not None and fused == separate


def test_graph_capture_and_replay(dev):
    import torch
    h, w, comps, codec = 1024, 768, 4, T.DXT1
    src = torch.from_numpy(_img(h, w, comps, index=9).reshape(-1).copy()).to(dev)
    total, _ = pkg.mip_chain_size(codec, h, w)
    out = torch.zeros((1, total), dtype=torch.uint8, device=dev)
    ws = torch.zeros((max(1, pkg.mip_workspace_size(codec, comps, h, w)),), dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside the capture
        pkg.encode_mips_device(codec, src, h, w, comps, out=out, workspace=ws, stream=s)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    out.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pkg.encode_mips_device(codec, src, h, w, comps, out=out, workspace=ws, stream=torch.cuda.current_stream())
    g.replay()
    torch.cuda.synchronize()
    first = out.cpu().numpy().tobytes()
    new = _img(h, w, comps, index=10)
    src.copy_(torch.from_numpy(new.reshape(-1).copy()).to(dev))
    g.replay()
    torch.cuda.synchronize()
    assert first == M.oracle_chain(codec, _img(h, w, comps, index=9), comps)
    assert out.cpu().numpy().tobytes() == M.oracle_chain(codec, new, comps)


def test_seeded_soak(dev):
    rng = np.random.default_rng(20261016)
    for case in range(200):
        codec, comps = M.LAYOUTS[rng.integers(len(M.LAYOUTS))]
        h = int(rng.integers(1, 300)) if rng.random() < 0.8 else int(rng.integers(1, 5))
        w = int(rng.integers(1, 300)) if rng.random() < 0.8 else int(rng.integers(1, 5))
        swap = int(rng.integers(2)) if comps >= 3 else 0
        levels = int(rng.integers(1, M.max_levels(h, w) + 1))
        strategy = int(rng.integers(4)) if codec == T.ETC1 else T.SMALLER_ERROR
        gen = ["noise", "smooth", "flat", "mixed"][case % 4]
        img = _img(h, w, comps, index=case, gen=T.GENERATORS[gen])
        _check_chain(codec, img, comps, dev, swap=swap, strategy=strategy, levels=levels)


def test_cxx_compress_mip_chain_equals_compress_per_level(tmp_path):
    """Compressor::CompressMipChain (owned and external storage) against Compress of each level's pixels, in C++
    (tests/cxx_mips/mip_chain_driver.cc, built here against the C++ classes)."""
    import os
    import subprocess
    pkg_dir = os.path.join(T.ROOT, "image-compression_amd")
    exe = os.path.join(str(tmp_path), "mip_chain_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(pkg_dir, "cxx"), "-I" + os.path.join(T.ROOT, "include"),
                           "-o", exe, os.path.join(T.ROOT, "tests", "cxx_mips", "mip_chain_driver.cc"), "-L" + pkg_dir,
                           "-limagecompression_amd", "-Wl,-rpath," + pkg_dir])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0, out + r.stderr.decode()
    assert out.count("OK ") == 13, out


def test_caller_buffers_are_checked(dev):
    import torch
    h, w = 300, 200
    src = torch.zeros(h * w * 4, dtype=torch.uint8, device=dev)
    total, _ = pkg.mip_chain_size(T.DXT1, h, w)
    for bad in (torch.empty((1, total - 1), dtype=torch.uint8, device=dev), torch.empty((total,), dtype=torch.uint8, device=dev),
                torch.empty((2, total), dtype=torch.uint8, device=dev), torch.empty((1, total), dtype=torch.int32, device=dev)):
        with pytest.raises(ValueError):
            pkg.encode_mips_device(T.DXT1, src, h, w, 4, out=bad)
    per, _ = pkg.mip_pyramid_size(4, h, w)
    with pytest.raises(ValueError):
        pkg.mip_pyramid_device(src, h, w, 4, out=torch.empty((1, per - 1), dtype=torch.uint8, device=dev))
    # a workspace smaller than icamd_mip_workspace_size is refused by the C side
    with pytest.raises(pkg.BackendError):
        pkg.encode_mips_device(T.DXT1, src, h, w, 4, workspace=torch.empty((1,), dtype=torch.uint8, device=dev))
