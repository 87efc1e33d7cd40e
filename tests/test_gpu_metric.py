"""GPU tier for the quality metric (include/ic_amd.h, icamd_measure_error_device): the HIP kernels through the C ABI, the
Python wrappers and the C++ member.  Every comparison is == on integers against the definition computed with the oracle's
decoders (tests/metric_oracle.py)."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import bc45_oracle as B
import ic_testlib as T
import metric_oracle as M
import wrapper_cases as W

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


def _measure(codec, src, blocks, h, w, comps, dev, **kw):
    """(sse [n, 4], max_abs [n, 4]) as numpy int64; src / blocks: bytes-like or device tensors."""
    import torch
    launch = (max(kw.get("grid_height") or h, h), max(kw.get("grid_width") or w, w), kw.get("n_images", 1))
    assert launch in W.METRIC_GRIDS, "list %r in wrapper_cases.METRIC_GRIDS: fastdiv is probed at this file's divisors" % (launch,)
    s = src if hasattr(src, "is_cuda") else _to_dev(src, dev)
    b = blocks if hasattr(blocks, "is_cuda") else _to_dev(blocks, dev)
    got = pkg.measure_error_device(codec, s, b, h, w, comps, **kw)
    assert got is not None
    torch.cuda.synchronize()
    return got[0].cpu().numpy().astype(np.int64), got[1].cpu().numpy().astype(np.int64)


def _encode(codec, src, h, w, comps, swap, gh=None, gw=None):
    if codec in (M.BC4, M.BC5):
        return B.oracle_encode(codec, src, h, w, comps, swap, gh=gh, gw=gw)
    return T.oracle_encode(codec, src, h, w, comps, swap, strategy=T.HEURISTIC, gh=gh, gw=gw)


def _random(codec, gh, gw, seed):
    if codec in (M.BC4, M.BC5):
        return B.random_words(codec, gh, gw, seed)
    return T.random_blocks(codec, gh, gw, seed)[:M.grid_bytes(codec, gh, gw)]  # (PVRTC 2 bpp: 8 x 4-pixel blocks)


def _check(got, want, i=0, what=None):
    assert (got[0][i] == want[0]).all() and (got[1][i] == want[1]).all(), (what, got[0][i], got[1][i], want)


@pytest.mark.parametrize("gen", sorted(T.GENERATORS))
def test_every_codec_layout_and_content(dev, gen):
    h = w = 64
    img = B.image(gen, h, w, 4, index=3)
    for codec, comps, swap in M.BLOCK_LAYOUTS:
        src = np.ascontiguousarray(img[..., :comps])
        for blocks in (_encode(codec, src, h, w, comps, swap), _random(codec, h, w, 77)):
            got = _measure(codec, src.tobytes(), blocks, h, w, comps, dev, swap_rb=bool(swap))
            _check(got, M.measure(codec, src, blocks, h, w, comps, swap), what=(gen, codec, comps, swap))
    # PVRTC: 64^2 takes the raster kernels, 256^2 the tile kernels (block grids of at least 32 x 8)
    for size in (8, 64, 256):
        img = T.GENERATORS[gen](size, size, 4, 5)
        for codec, comps, swap in M.PVRTC_LAYOUTS:
            for blocks in (T.oracle_encode(codec, img, size, size, 4), _random(codec, size, size, 78 + size)):
                got = _measure(codec, img.tobytes(), blocks, size, size, 4, dev)
                _check(got, M.measure(codec, img, blocks, size, size, 4), what=(gen, codec, size))


def test_pvrtc4_random_words_include_punch_through_blocks():
    words = np.frombuffer(_random(M.PVRTC4, 256, 256, 78 + 256), np.uint32).reshape(-1, 2)
    assert (words[:, 1] & 1).any() and not (words[:, 1] & 1).all()


@pytest.mark.parametrize("h,w,pad", [(61, 59, 3), (5, 3, 0), (1, 1, 0), (257, 1023, 5)])
def test_ragged_shapes_row_padding_and_larger_grids(dev, h, w, pad):
    img = B.image("mixed", h, w, 4, index=h)
    gh, gw = h + 9, w + 13
    g = np.random.Generator(np.random.PCG64(h * w))
    for codec, comps, swap in M.BLOCK_LAYOUTS:
        src = np.ascontiguousarray(img[..., :comps])
        stride = w * comps + pad
        flat = T.with_row_padding(src, pad)
        for blocks in (_encode(codec, src, h, w, comps, swap, gh=gh, gw=gw), _random(codec, gh, gw, 31 + h)):
            want = M.measure(codec, src, blocks, h, w, comps, swap, gh=gh, gw=gw)
            got = _measure(codec, flat.tobytes(), blocks, h, w, comps, dev, swap_rb=bool(swap), grid_height=gh, grid_width=gw,
                           row_stride_bytes=stride)
            _check(got, want, what=(h, w, pad, codec, comps, swap))
            # garbage in the row padding and in every block outside the image: the same record
            rows = flat.reshape(h, stride).copy()
            rows[:, w * comps:] = g.integers(0, 256, size=(h, pad), dtype=np.uint8)
            bb = M.block_bytes(codec)
            grid = np.frombuffer(bytes(blocks), np.uint8).reshape((gh + 3) // 4, (gw + 3) // 4, bb).copy()
            junk = g.integers(0, 256, size=grid.shape, dtype=np.uint8)
            grid[(h + 3) // 4:] = junk[(h + 3) // 4:]
            grid[:, (w + 3) // 4:] = junk[:, (w + 3) // 4:]
            got = _measure(codec, rows.tobytes(), grid.tobytes(), h, w, comps, dev, swap_rb=bool(swap), grid_height=gh,
                           grid_width=gw, row_stride_bytes=stride)
            _check(got, want, what=("garbage", h, w, pad, codec, comps, swap))
        # the plain grid as well
        blocks = _encode(codec, src, h, w, comps, swap)
        got = _measure(codec, flat.tobytes(), blocks, h, w, comps, dev, swap_rb=bool(swap), row_stride_bytes=stride)
        _check(got, M.measure(codec, src, blocks, h, w, comps, swap), what=("plain", h, w, pad, codec, comps, swap))


def _batch_case(dev, codec, comps, swap, h, w, n, slack_src, slack_blk, lead):
    """n images with image strides larger than an image, both buffers starting `lead` bytes into their allocations."""
    import torch
    per_src, per_blk = h * w * comps, M.grid_bytes(codec, h, w)
    src_stride, blk_stride = per_src + slack_src, per_blk + slack_blk
    src_buf = np.full(lead + n * src_stride, 0x5A, np.uint8)
    blk_buf = np.full(lead + n * blk_stride, 0xC3, np.uint8)
    wants = []
    for i in range(n):
        img = B.image(("noise", "mixed", "smooth", "flat")[i % 4], h, w, 4, index=10 + i)
        src = np.ascontiguousarray(img[..., :comps])
        if codec in (M.PVRTC2, M.PVRTC4):
            blocks = T.oracle_encode(codec, src, h, w, 4) if i % 2 else _random(codec, h, w, 400 + i)
        else:
            blocks = _encode(codec, src, h, w, comps, swap) if i % 2 else _random(codec, h, w, 400 + i)
        src_buf[lead + i * src_stride: lead + i * src_stride + per_src] = src.reshape(-1)
        blk_buf[lead + i * blk_stride: lead + i * blk_stride + per_blk] = np.frombuffer(bytes(blocks), np.uint8)
        wants.append(M.measure(codec, src, blocks, h, w, comps, swap))
    d_src, d_blk = torch.from_numpy(src_buf).to(dev), torch.from_numpy(blk_buf).to(dev)
    got = _measure(codec, d_src[lead:], d_blk[lead:], h, w, comps, dev, swap_rb=bool(swap), n_images=n,
                   src_image_stride_bytes=src_stride, blocks_image_stride_bytes=blk_stride)
    for i in range(n):
        _check(got, wants[i], i, what=(codec, comps, swap, h, w, n, i))


def test_batches_with_strides_and_odd_starts(dev):
    for codec, comps, swap in M.BLOCK_LAYOUTS:
        _batch_case(dev, codec, comps, swap, 61, 59, 5, 37, 24, 1)
        _batch_case(dev, codec, comps, swap, 64, 128, 3, 0, 0, 0)     # 512 blocks an image: a workgroup spans two images
    for codec, comps, swap in M.PVRTC_LAYOUTS:
        _batch_case(dev, codec, 4, 0, 64, 64, 5, 48, 16, 1)
        _batch_case(dev, codec, 4, 0, 256, 256, 3, 16, 8, 3)


def test_a_workgroup_that_spans_many_small_images(dev):
    for codec, comps, swap in M.BLOCK_LAYOUTS + M.PVRTC_LAYOUTS:
        _batch_case(dev, codec, comps, swap, 8, 8, 37, 5, 8, 1)
    _batch_case(dev, M.DXT1, 4, 0, 12, 20, 300, 0, 0, 0)  # 15 blocks an image: waves that span five images


@pytest.mark.parametrize("codec,comps,size", [(M.DXT1, 4, 4096), (M.ETC1, 3, 4096), (M.PVRTC2, 4, 4096), (M.PVRTC4, 4, 2048)])
def test_one_full_size_image(dev, codec, comps, size):
    """Full-size launches (2^20 blocks and more: thousands of workgroups adding to one record).  The blocks come from the
    device encoders -- their bytes are pinned elsewhere; here only the metric of whatever they wrote is checked."""
    import torch
    img = T.s_mixed(size, size, comps, index=21)
    d_src = torch.from_numpy(img.reshape(-1)).to(dev)
    d_blocks = pkg.encode_device(codec, d_src, size, size, comps, etc_strategy=pkg.ETC_HEURISTIC)
    torch.cuda.synchronize()
    blocks = d_blocks.cpu().numpy().tobytes()
    got = _measure(codec, d_src, d_blocks.reshape(-1), size, size, comps, dev)
    want = M.measure(codec, img, blocks, size, size, comps)
    print("full size", codec, size, "sse", got[0][0], "max", got[1][0], "psnr",
          pkg.psnr_from_stats(got[0][0], size * size, 3 if comps == 3 or codec == M.DXT1 else 4))
    _check(got, want, what=(codec, size))


def test_a_solid_image_measures_zero(dev):
    import torch
    h, w = 61, 59
    for compressor, fmt, codec, comps, color in [(pkg.COMPRESSOR_DXTC, pkg.RGB, M.DXT1, 3, (8, 4, 8)),
                                                 (pkg.COMPRESSOR_DXTC, pkg.RGBA, M.DXT5, 4, (255, 0, 255, 77)),
                                                 (pkg.COMPRESSOR_ETC, pkg.RGB, M.ETC1, 3, (8, 16, 24))]:
        blocks = pkg.create_solid_device(compressor, fmt, h, w, bytes(color), device=dev)
        torch.cuda.synchronize()
        dec = M.decode(codec, blocks.cpu().numpy().tobytes(), h, w)
        src = np.ascontiguousarray(np.broadcast_to(dec[0, 0], (h, w, comps)))  # the colour the solid block decodes to
        assert (dec == src).all()
        got = _measure(codec, src.tobytes(), blocks.reshape(-1), h, w, comps, dev)
        assert not got[0].any() and not got[1].any(), (codec, got)


def test_measure_of_encode_equals_numpy_on_decode_device(dev):
    import torch
    h, w = 257, 1023
    for comps, swap in ((3, 0), (4, 1)):
        img = T.s_mixed(h, w, comps, index=33)
        d_src = torch.from_numpy(img.reshape(-1)).to(dev)
        d_blocks = pkg.encode_device(M.DXT1, d_src, h, w, comps, swap_rb=bool(swap))
        d_pix = pkg.decode_device(M.DXT1, d_blocks.reshape(-1), h, w, swap_rb=bool(swap))
        torch.cuda.synchronize()
        dec = d_pix.cpu().numpy().reshape(h, w, 3)
        got = _measure(M.DXT1, d_src, d_blocks.reshape(-1), h, w, comps, dev, swap_rb=bool(swap))
        _check(got, M.stats_of(img, dec, M.DXT1, comps, swap), what=(comps, swap))


def test_graph_capture_replays_to_the_same_records(dev):
    import torch
    h, w, n = 128, 128, 3
    imgs = np.stack([T.s_mixed(h, w, 4, index=40 + i) for i in range(n)])
    blocks = b"".join(T.oracle_encode(M.DXT5, imgs[i], h, w, 4) for i in range(n))
    d_src, d_blk = torch.from_numpy(imgs.reshape(-1)).to(dev), _to_dev(blocks, dev)
    out = torch.full((n, pkg.ERROR_STATS_BYTES), 0xEE, dtype=torch.uint8, device=dev)
    args = (M.DXT5, 4, 0, h, w, h, w, w * 4, n, h * w * 4, len(blocks) // n, d_src.data_ptr(), d_blk.data_ptr(), out.data_ptr())
    assert pkg.lib().icamd_measure_error_device(*args, None) == 0  # (the kernel's first launch loads its code: not under capture)
    torch.cuda.synchronize()
    out.fill_(0xEE)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            assert pkg.lib().icamd_measure_error_device(*args, torch.cuda.current_stream().cuda_stream) == 0
    records = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        records.append(out.cpu().numpy().copy())
    assert (records[0] == records[1]).all(), (records[0], records[1])
    for i in range(n):
        want = M.measure(M.DXT5, imgs[i], blocks[i * (len(blocks) // n):(i + 1) * (len(blocks) // n)], h, w, 4)
        assert (records[1][i, :32].view(np.uint64).astype(np.int64) == want[0]).all()
        assert (records[1][i, 32:].view(np.uint32).astype(np.int64) == want[1]).all()


def test_host_form_equals_the_device_form(dev):
    for compressor, fmt, codec, comps, swap, h, w, pad in [(pkg.COMPRESSOR_DXTC, pkg.RGB, M.DXT1, 3, 0, 61, 59, 3),
                                                           (pkg.COMPRESSOR_DXTC, pkg.BGRA, M.DXT5, 4, 1, 37, 130, 0),
                                                           (pkg.COMPRESSOR_ETC, pkg.RGB, M.ETC1, 3, 0, 64, 64, 5),
                                                           (pkg.COMPRESSOR_PVRTC, pkg.RGBA, M.PVRTC2, 4, 0, 256, 256, 0)]:
        img = T.s_mixed(h, w, comps, index=50)
        blocks = T.oracle_encode(codec, img, h, w, comps, swap, strategy=T.HEURISTIC)
        flat = T.with_row_padding(img, pad)
        sse, mx = pkg.measure_error_host(compressor, fmt, flat, blocks, h, w, padding_bytes_per_row=pad)
        got = _measure(codec, flat.tobytes(), blocks, h, w, comps, dev, swap_rb=bool(swap), row_stride_bytes=w * comps + pad)
        want = M.measure(codec, img, blocks, h, w, comps, swap)
        _check(got, want, what=(codec, h, w))
        assert (sse == want[0]).all() and (mx == want[1]).all(), (codec, sse, mx, want)
    assert pkg.measure_error_host(pkg.COMPRESSOR_ETC, pkg.RGBA, np.zeros(256, np.uint8), bytes(32), 8, 8) is None


def test_cxx_member_equals_the_c_abi(tmp_path):
    """MeasureErrorDevice of the C++ classes, the C ABI's device form and its host form leave the same record
    (tests/cxx_metric/measure_driver.cc, built here against the C++ classes and the HIP runtime API)."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    pkg_dir = os.path.join(T.ROOT, "image-compression_amd")
    exe = os.path.join(str(tmp_path), "measure_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                           "-I" + os.path.join(pkg_dir, "cxx"), "-I" + os.path.join(T.ROOT, "include"), "-o", exe,
                           os.path.join(T.ROOT, "tests", "cxx_metric", "measure_driver.cc"), "-L" + pkg_dir,
                           "-limagecompression_amd", "-lic_amd", "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                           "-Wl,-rpath," + pkg_dir, "-Wl,-rpath," + os.path.join(rocm, "lib")])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0, out + r.stderr.decode()
    assert out.count("OK ") == 7 and "BAD" not in out, out


def _extreme_pair(codec, comps, swap, h, w):
    """(source of zeros, the oracle's blocks for an all-255 image of the same shape, the definition's record)."""
    src = np.zeros((h, w, comps), np.uint8)
    white = np.full((h, w, comps), 255, np.uint8)
    blocks = T.oracle_encode(codec, white, h, w, 4) if codec in (M.PVRTC2, M.PVRTC4) else _encode(codec, white, h, w, comps, swap)
    want = M.measure(codec, src, blocks, h, w, comps, swap)
    for k, _, _ in M.channel_pairs(codec, comps, swap):  # a condition on the input alone: every difference is at the top
        assert want[1][k] >= 247, (codec, comps, swap, k, want[1])
    return src, blocks, want


def _extreme_batch(dev, codec, comps, swap, h, w, n):
    src, blocks, want = _extreme_pair(codec, comps, swap, h, w)
    got = _measure(codec, src.tobytes() * n, bytes(blocks) * n, h, w, comps, dev, swap_rb=bool(swap), n_images=n)
    for i in range(n):
        _check(got, want, i, what=("extremes", codec, comps, swap, h, w, n, i))


def test_partial_sums_at_the_top_of_their_range(dev):
    """metric_block.h budgets 256 * 4 * 32 * 65025 < 2^32 for a workgroup's 32-bit partial sums: every pixel of every block of a
    full workgroup differs by (nearly) 255 -- 128 x 128 is 1024 blocks -- and the same extremes through the per-wave flush of a
    workgroup that spans 37 small images."""
    for codec, comps, swap in M.BLOCK_LAYOUTS:
        _extreme_batch(dev, codec, comps, swap, 128, 128, 1)
        _extreme_batch(dev, codec, comps, swap, 8, 8, 37)


def test_pvrtc_partial_sums_at_the_top_of_their_range(dev):
    for codec, comps, swap in M.PVRTC_LAYOUTS:
        _extreme_batch(dev, codec, comps, swap, 256, 256, 1)
