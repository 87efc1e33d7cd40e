"""GPU tier of the mip filters (include/ic_amd.h, "mip filters"): icamd_encode_mips_filtered_device, icamd_mip_pyramid_filtered_device
and icamd_compress_mips_filtered against the oracle pyramid (tests/mip_filter_oracle.py) fed to the existing oracle encoders;
filter 0 against the unfiltered entry points; the named properties as exact bytes; large cases, batches, padded rows; graph
capture, the host form, the C++ class and containers."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

import ic_testlib as T
import mip_filter_oracle as F
import mips_oracle as M

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("image-compression_amd")
SRGB, ALPHA, BOTH = pkg.MIP_FILTER_SRGB, pkg.MIP_FILTER_ALPHA_WEIGHTED, pkg.MIP_FILTER_SRGB | pkg.MIP_FILTER_ALPHA_WEIGHTED


@pytest.fixture(scope="module")
def dev():
    import torch
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


def _dev(arr, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).reshape(-1).copy()).to(dev)


def _fused(codec, img, comps, dev, **kw):
    import torch
    h, w = img.shape[:2]
    flat, views = pkg.encode_mips_device(codec, _dev(img, dev), h, w, comps, **kw)
    torch.cuda.synchronize()
    return flat.cpu().numpy(), [v.cpu().numpy() for v in views]


def _check_chain(codec, img, comps, mip_filter, dev, swap=0, strategy=T.SMALLER_ERROR, levels=None):
    h, w = img.shape[:2]
    flat, views = _fused(codec, img, comps, dev, swap_rb=bool(swap), etc_strategy=strategy, levels=levels, mip_filter=mip_filter)
    for l, p in enumerate(F.pyramid(img, mip_filter, levels)):
        want = M.oracle_encode(codec, p, comps, swap, strategy)
        assert views[l][0].tobytes() == want, (codec, comps, mip_filter, swap, strategy, h, w, l)


# ---- chains

@pytest.mark.parametrize("codec,comps,filters", F.LAYOUTS)
def test_every_codec_layout_filter_and_swap(dev, codec, comps, filters):
    for i, (h, w) in enumerate(F.SHAPES):
        img = F.gpu_image(h, w, comps, i)
        for f in filters:
            for swap in (0, 1):
                _check_chain(codec, img, comps, f, dev, swap=swap)


@pytest.mark.parametrize("codec,comps,filters", F.LAYOUTS)
def test_partial_levels(dev, codec, comps, filters):
    h, w = 300, 200
    img = F.gpu_image(h, w, comps, 4)
    for f in filters:
        for levels in (1, 2, 3, 6, 7, 8):
            _check_chain(codec, img, comps, f, dev, levels=levels)


@pytest.mark.parametrize("strategy", [0, 1, 2, 3])
def test_etc1_every_strategy(dev, strategy):
    for i, (h, w) in enumerate(F.ETC1_SHAPES):
        _check_chain(T.ETC1, F.gpu_image(h, w, 3, 10 + i), 3, SRGB, dev, strategy=strategy)
        for f in (SRGB, ALPHA, BOTH):
            _check_chain(T.ETC1, F.gpu_image(h, w, 4, 10 + i), 4, f, dev, strategy=strategy)


@pytest.mark.parametrize("comps,filters", [(3, (SRGB,)), (4, (SRGB, ALPHA, BOTH))])
def test_filtered_pyramid_entry(dev, comps, filters):
    import torch
    for i, (h, w) in enumerate(F.PYRAMID_SHAPES):
        img = F.gpu_image(h, w, comps, 20 + i)
        for f in filters:
            flat, views = pkg.mip_pyramid_device(_dev(img, dev), h, w, comps, mip_filter=f)
            torch.cuda.synchronize()
            assert len(views) == M.max_levels(h, w) - 1
            assert flat.cpu().numpy()[0, :pkg.mip_pyramid_size(comps, h, w)[0]].tobytes() == F.pyramid_bytes(img, f), (comps, f, h, w)
    # a batch with padded rows, non-tight strides and partial levels
    n, h, w, pad = 5, 300, 301, 9
    stride, sis = w * comps + pad, (w * comps + pad) * h + 40
    per, _ = pkg.mip_pyramid_size(comps, h, w, 5)
    src = np.zeros(n * sis, np.uint8)
    imgs = [F.gpu_image(h, w, comps, 40 + i) for i in range(n)]
    for i in range(n):
        for y in range(h):
            src[i * sis + y * stride:i * sis + y * stride + w * comps] = imgs[i][y].reshape(-1)
    f = filters[-1]
    flat, _ = pkg.mip_pyramid_device(torch.from_numpy(src).to(dev), h, w, comps, levels=5, n_images=n, row_stride_bytes=stride,
                                     src_image_stride_bytes=sis, dst_image_stride_bytes=per + 12, mip_filter=f)
    torch.cuda.synchronize()
    got = flat.cpu().numpy()
    for i in range(n):
        assert got[i, :per].tobytes() == F.pyramid_bytes(imgs[i], f, 5), i


# ---- filter 0 through the new entry points is the old entry points

def test_filter_zero_gives_the_bytes_of_the_unfiltered_entry_points(dev):
    import torch
    lib = pkg.lib()
    for (codec, comps), (h, w) in zip(M.LAYOUTS, F.FILTER_ZERO_SHAPES):
        img = F.gpu_image(h, w, 4, h)[..., :comps]
        d = _dev(img, dev)
        levels = pkg.mip_max_levels(h, w)
        total, _ = pkg.mip_chain_size(codec, h, w)
        ws_bytes = pkg.mip_workspace_size(codec, comps, h, w)
        ws = torch.zeros((max(ws_bytes, 1),), dtype=torch.uint8, device=dev)
        old = torch.zeros((total,), dtype=torch.uint8, device=dev)
        new = torch.zeros((total,), dtype=torch.uint8, device=dev)
        args = (h, w, w * comps, levels, 1, 0, 0, d.data_ptr())
        assert lib.icamd_encode_mips_device(codec, 2, comps, 0, *args, old.data_ptr(), ws.data_ptr(), ws_bytes, None) == 0
        assert lib.icamd_encode_mips_filtered_device(codec, 2, comps, 0, 0, *args, new.data_ptr(), ws.data_ptr(), ws_bytes, None) == 0
        torch.cuda.synchronize()
        assert torch.equal(old, new), (codec, comps)
        per, _ = pkg.mip_pyramid_size(comps, h, w)
        old = torch.zeros((max(per, 1),), dtype=torch.uint8, device=dev)
        new = torch.zeros((max(per, 1),), dtype=torch.uint8, device=dev)
        assert lib.icamd_mip_pyramid_device(comps, *args, old.data_ptr(), None) == 0
        assert lib.icamd_mip_pyramid_filtered_device(comps, 0, *args, new.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert torch.equal(old, new), comps
    for compressor, fmt, comps, codec in [(T.DXTC, T.RGB, 3, T.DXT1), (T.DXTC, T.BGRA, 4, T.DXT5), (T.ETC, T.RGB, 3, T.ETC1)]:
        h, w, pad = 61, 59, 5
        buf = _padded(F.gpu_image(h, w, comps, 2), pad)
        total = pkg.mip_chain_size(codec, h, w)[0]
        a, b = np.zeros(total, np.uint8), np.zeros(total, np.uint8)
        assert lib.icamd_compress_mips(compressor, 2, fmt, h, w, pad, 6, buf.ctypes.data, a.ctypes.data, total) == 0
        assert lib.icamd_compress_mips_filtered(compressor, 2, fmt, 0, h, w, pad, 6, buf.ctypes.data, b.ctypes.data, total) == 0
        assert a.tobytes() == b.tobytes()


# ---- the named properties, as exact bytes

def test_flat_images_stay_flat_under_srgb(dev):
    import torch
    h, w = 40, 24
    for comps in (3, 4):
        for f in ((SRGB,) if comps == 3 else (SRGB, BOTH)):
            imgs = np.zeros((256, h, w, comps), np.uint8)
            imgs[...] = np.arange(256, dtype=np.uint8)[:, None, None, None]
            flat, views = pkg.mip_pyramid_device(_dev(imgs, dev), h, w, comps, n_images=256, mip_filter=f)
            torch.cuda.synchronize()
            assert len(views) == 5
            for v in views:
                got = v.cpu().numpy()
                assert (got == np.arange(256, dtype=np.uint8)[:, None, None, None]).all(), (comps, f)


def _level1(img, mip_filter, dev):
    import torch
    h, w, c = img.shape
    flat, views = pkg.mip_pyramid_device(_dev(img, dev), h, w, c, levels=2, mip_filter=mip_filter)
    torch.cuda.synchronize()
    return views[0].cpu().numpy()[0]


def test_checkerboard_and_alpha_quads(dev):
    cb = np.zeros((8, 8, 3), np.uint8)
    cb[(np.arange(8)[:, None] + np.arange(8)[None, :]) % 2 == 0] = 255
    assert (_level1(cb, SRGB, dev) == 188).all()
    assert (_level1(cb, 0, dev) == 127).all()
    q = np.zeros((2, 2, 4), np.uint8)
    q[..., 0] = 255          # three (255, 0, 0, alpha 0) texels ...
    q[1, 1] = (0, 0, 255, 255)  # ... and one (0, 0, 255, alpha 255)
    for f in (ALPHA, BOTH):
        assert _level1(q, f, dev).tolist() == [[[0, 0, 255, 63]]], f
    assert _level1(q, 0, dev).tolist() == [[[191, 0, 63, 63]]]
    q[1, 1, 3] = 0  # all transparent: the unweighted value of the same filter
    assert _level1(q, ALPHA, dev).tolist() == _level1(q, 0, dev).tolist() == [[[191, 0, 63, 0]]]
    assert _level1(q, BOTH, dev).tolist() == _level1(q, SRGB, dev).tolist() == F.next_level(q, SRGB).tolist()
    # the alpha half of a DXT5 chain does not depend on the filter
    img = F.gpu_image(61, 59, 4, 7)
    chains = [_fused(T.DXT5, img, 4, dev, mip_filter=f)[0][0] for f in (0, SRGB, ALPHA, BOTH)]
    alpha_halves = [c.reshape(-1, 16)[:, :8].tobytes() for c in chains]
    assert alpha_halves[0] == alpha_halves[1] == alpha_halves[2] == alpha_halves[3]
    assert len({c.tobytes() for c in chains}) == 4


# ---- scale

def _levels_by_encode_device(codec, pyr, comps, dev):
    out = []
    for p in pyr:
        lh, lw = p.shape[:2]
        out.append(pkg.encode_device(codec, _dev(p, dev), lh, lw, comps).cpu().numpy()[0].tobytes())
    return out


@pytest.mark.parametrize("codec,mip_filter", [(T.DXT1, BOTH), (T.DXT5, ALPHA)])
def test_4096_square(dev, codec, mip_filter):
    img = F.gpu_image(4096, 4096, 4, 5)
    flat, views = _fused(codec, img, 4, dev, mip_filter=mip_filter)
    pyr = F.pyramid(img, mip_filter)
    want = _levels_by_encode_device(codec, pyr, 4, dev)  # icamd_encode_device is pinned to the oracle by the existing GPU tier
    for l in range(len(want)):
        assert views[l][0].tobytes() == want[l], (codec, l)
        if l >= 3:  # the oracle itself from 512^2 down (both sides of the pass boundary at level 6)
            assert views[l][0].tobytes() == M.oracle_encode(codec, pyr[l], 4), (codec, l)


@pytest.mark.parametrize("codec,comps,mip_filter", [(T.DXT1, 4, BOTH), (T.DXT5, 4, ALPHA), (T.ETC1, 3, SRGB), (T.DXT1, 3, SRGB)])
def test_batch_of_64_with_non_tight_strides(dev, codec, comps, mip_filter):
    """64 x 256^2 with padded rows (an odd stride: unaligned rows), gaps between the images and between the chains."""
    import torch
    n, h, w, pad = 64, 256, 256, 13
    stride = w * comps + pad
    sis = h * stride + 160
    total, offs = pkg.mip_chain_size(codec, h, w)
    dis = total + 24
    src = np.full(n * sis, 0xa5, np.uint8)
    imgs = [F.gpu_image(h, w, comps, 100 + i) for i in range(n)]
    for i in range(n):
        rows = src[i * sis:i * sis + h * stride].reshape(h, stride)
        rows[:, :w * comps] = imgs[i].reshape(h, w * comps)
    flat, views = pkg.encode_mips_device(codec, torch.from_numpy(src).to(dev), h, w, comps, n_images=n, row_stride_bytes=stride,
                                         src_image_stride_bytes=sis, dst_image_stride_bytes=dis, mip_filter=mip_filter)
    torch.cuda.synchronize()
    got = flat.cpu().numpy()
    assert got.shape == (n, dis)
    for i in range(n):
        assert got[i, :total].tobytes() == F.oracle_chain(codec, imgs[i], comps, mip_filter), (codec, i)


def _padded(img, pad):
    h, w, c = img.shape
    out = np.zeros((h, w * c + pad), np.uint8)
    out[:, :w * c] = img.reshape(h, w * c)
    return out.reshape(-1)[:(h - 1) * (w * c + pad) + w * c].copy()


def test_row_padding_and_unaligned_rgb888_rows(dev):
    import torch
    h, w, pad = 61, 59, 7
    for codec, comps, f in [(T.DXT1, 3, SRGB), (T.ETC1, 3, SRGB), (T.DXT5, 4, BOTH), (T.DXT1, 4, ALPHA)]:
        img = F.gpu_image(h, w, comps, 3)
        stride = w * comps + pad
        buf = np.zeros(1 + h * stride, np.uint8)  # one leading byte: rows start at odd addresses
        buf[1:1 + (h - 1) * stride + w * comps] = _padded(img, pad)
        d = torch.from_numpy(buf).to(dev)[1:]
        flat, views = pkg.encode_mips_device(codec, d, h, w, comps, row_stride_bytes=stride, mip_filter=f)
        torch.cuda.synchronize()
        for l, p in enumerate(F.pyramid(img, f)):
            assert views[l].cpu().numpy()[0].tobytes() == M.oracle_encode(codec, p, comps), (codec, comps, l)


# ---- other forms

def test_graph_capture_and_replay(dev):
    import torch
    h, w, comps, codec, f = 1024, 768, 4, T.DXT1, BOTH
    first_img, second_img = F.gpu_image(h, w, comps, 9), F.gpu_image(h, w, comps, 10)
    src = _dev(first_img, dev)
    total, _ = pkg.mip_chain_size(codec, h, w)
    out = torch.zeros((1, total), dtype=torch.uint8, device=dev)
    ws = torch.zeros((max(1, pkg.mip_workspace_size(codec, comps, h, w)),), dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside the capture
        pkg.encode_mips_device(codec, src, h, w, comps, out=out, workspace=ws, stream=s, mip_filter=f)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    eager = out.cpu().numpy().tobytes()
    out.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pkg.encode_mips_device(codec, src, h, w, comps, out=out, workspace=ws, stream=torch.cuda.current_stream(), mip_filter=f)
    g.replay()
    torch.cuda.synchronize()
    first = out.cpu().numpy().tobytes()
    src.copy_(_dev(second_img, dev))
    g.replay()
    torch.cuda.synchronize()
    assert first == eager == F.oracle_chain(codec, first_img, comps, f)
    assert out.cpu().numpy().tobytes() == F.oracle_chain(codec, second_img, comps, f)


def test_host_form_equals_device_form(dev):
    for compressor, fmt, comps, codec, filters in [(T.DXTC, T.RGB, 3, T.DXT1, (SRGB,)), (T.DXTC, T.BGRA, 4, T.DXT5, (SRGB, ALPHA, BOTH)),
                                                   (T.DXTC, T.RGBA, 4, T.DXT5, (BOTH,)), (T.ETC, T.RGB, 3, T.ETC1, (SRGB,))]:
        swap = 1 if fmt == T.BGRA else 0
        for h, w, pad in F.HOST_FORM_SHAPES:
            img = F.gpu_image(h, w, comps, h)
            for f in filters:
                got = pkg.compress_mips_host(compressor, fmt, _padded(img, pad), h, w, padding_bytes_per_row=pad, mip_filter=f)
                device = _fused(codec, img, comps, dev, swap_rb=bool(swap), mip_filter=f)[0][0].tobytes()
                assert got == device == F.oracle_chain(codec, img, comps, f, swap=swap), (compressor, fmt, f, h, w)
    assert pkg.compress_mips_host(T.ETC, T.RGBA, np.zeros(16 * 16 * 4, np.uint8), 16, 16, mip_filter=SRGB) is None


def test_cxx_compress_mip_chain_filtered(tmp_path):
    """Compressor::CompressMipChainFiltered through tests/cxx_mips/mip_filter_driver.cc (built here against the C++ classes):
    every chain it writes against the oracle's."""
    pkg_dir = os.path.join(T.ROOT, "image-compression_amd")
    exe = os.path.join(str(tmp_path), "mip_filter_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(pkg_dir, "cxx"), "-I" + os.path.join(T.ROOT, "include"),
                           "-o", exe, os.path.join(T.ROOT, "tests", "cxx_mips", "mip_filter_driver.cc"), "-L" + pkg_dir,
                           "-limagecompression_amd", "-Wl,-rpath," + pkg_dir])
    h, w, pad = 61, 130, 3
    img = F.gpu_image(h, w, 4, 6)
    src = os.path.join(str(tmp_path), "src.rgba")
    img.tofile(src)
    r = subprocess.run([exe, src, str(h), str(w), str(pad), str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0, out + r.stderr.decode()
    assert out.count("OK ") == 4 * 2 + 2 * 2 + 1, out
    for f in (0, 1, 2, 3):
        cases = [("dxtc_rgba", T.DXT5, 4, 0), ("dxtc_bgra", T.DXT5, 4, 1)] + ([("dxtc_rgb", T.DXT1, 3, 0), ("etc_rgb", T.ETC1, 3, 0)] if f <= 1 else [])
        for name, codec, comps, swap in cases:
            got = open(os.path.join(str(tmp_path), "%s_f%d.bin" % (name, f)), "rb").read()
            want = F.oracle_chain(codec, np.ascontiguousarray(img[..., :comps]), comps, f, swap=swap)
            assert got == want, (name, f)


@pytest.mark.parametrize("container,codec,comps,mip_filter", [(pkg.CONTAINER_KTX, T.ETC1, 3, SRGB), (pkg.CONTAINER_DDS, T.DXT5, 4, BOTH),
                                                              (pkg.CONTAINER_DDS, T.DXT1, 4, ALPHA)])
def test_filtered_chain_as_container(dev, container, codec, comps, mip_filter):
    h, w = 200, 136
    img = F.gpu_image(h, w, comps, 8)
    flat, views = _fused(codec, img, comps, dev, mip_filter=mip_filter)
    fused = pkg.container_write(container, codec, h, w, [v[0].tobytes() for v in views])
    separate = pkg.container_write(container, codec, h, w, [M.oracle_encode(codec, p, comps) for p in F.pyramid(img, mip_filter)])
    assert fused is not None and fused == separate


def test_filters_are_refused_where_they_do_not_apply(dev):
    import torch
    import bc45_oracle as B
    src = torch.zeros(64 * 64 * 4, dtype=torch.uint8, device=dev)
    for codec, comps, f in [(B.BC4, 4, SRGB), (B.BC5, 4, ALPHA), (T.DXT1, 3, ALPHA), (T.DXT1, 4, 4), (T.ETC1, 3, BOTH)]:
        with pytest.raises(pkg.BackendError):
            pkg.encode_mips_device(codec, src, 64, 64, comps, mip_filter=f)
    with pytest.raises(pkg.BackendError):
        pkg.mip_pyramid_device(src, 64, 64, 2, mip_filter=SRGB)
