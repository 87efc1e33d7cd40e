"""GPU tier of the normal-map mip filter (include/ic_amd.h, "normal-map mip filter"): icamd_encode_mips_filtered_device and
icamd_mip_pyramid_filtered_device with ICAMD_MIP_FILTER_NORMAL against the oracle pyramid (tests/normal_filter_oracle.py) fed
to the BC5 oracle and to icamd_encode_device; batches, padded rows and unaligned sources; the RG8 pixel pyramid; filter 0
through the same entry point against the unfiltered one."""
import importlib

import numpy as np
import pytest

import bc45_oracle as B
import mips_oracle as M
import normal_filter_oracle as N

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("image-compression_amd")
NORMAL = pkg.MIP_FILTER_NORMAL
GUARD = 0xa5


@pytest.fixture(scope="module")
def dev():
    import torch
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


def _dev(arr, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).reshape(-1).copy()).to(dev)


@pytest.mark.parametrize("h,w", N.SIZES)
def test_chain_equals_the_oracle_and_encode_device_of_every_level(dev, h, w):
    """1 x 1 and 5 x 3 (one tile, almost no quads), 8 x 8, 64 x 64 (7 levels), 129 x 65 (tile column 1 holds none of level
    1's columns), 131 x 257, and 256 x 256 with 9 levels: the second pass reads the hand-off image, in a workspace of exactly
    icamd_mip_workspace_size bytes with guard bytes behind it."""
    import torch
    levels = pkg.mip_max_levels(h, w)
    for k, (comps, swap) in enumerate(N.LAYOUTS):
        img = N.gpu_image(h, w, comps, swap, k)
        ws_bytes = pkg.mip_workspace_size(B.BC5, comps, h, w, levels)
        backing = torch.full((ws_bytes + 64,), GUARD, dtype=torch.uint8, device=dev)
        flat, views = pkg.encode_mips_device(B.BC5, _dev(img, dev), h, w, comps, swap_rb=bool(swap), mip_filter=NORMAL,
                                             workspace=backing[:ws_bytes] if ws_bytes else None)
        torch.cuda.synchronize()
        assert (backing[ws_bytes:] == GUARD).all()
        pyr = N.pyramid(img, swap)
        assert len(views) == len(pyr) == levels
        for l, p in enumerate(pyr):
            lh, lw = p.shape[:2]
            got = views[l][0].cpu().numpy().tobytes()
            assert got == M.oracle_encode(B.BC5, p, comps, swap), (h, w, comps, swap, l)
            per_level = pkg.encode_device(B.BC5, _dev(p, dev), lh, lw, comps, swap_rb=bool(swap))
            assert got == per_level[0].cpu().numpy().tobytes(), (h, w, comps, swap, l)
        if (h, w) == (256, 256):
            assert ws_bytes == 4 * 4 * comps
        if ws_bytes:  # the hand-off image is level 6 of the same pyramid, every byte of every pixel
            assert ws_bytes == pyr[6].size
            assert np.array_equal(backing[:ws_bytes].cpu().numpy().reshape(pyr[6].shape), pyr[6]), (h, w, comps, swap)


@pytest.mark.parametrize("comps,swap", [(2, 0), (3, 1)])
def test_batch_with_row_padding_unaligned_source_and_wide_image_strides(dev, comps, swap):
    import torch
    n, (h, w), pad = 3, N.BATCH_SHAPE, 7
    stride = w * comps + pad
    sis = h * stride + 101
    total, _ = pkg.mip_chain_size(B.BC5, h, w)
    dis = total + 48
    imgs = [N.gpu_image(h, w, comps, swap, 20 + i) for i in range(n)]
    buf = np.full(1 + n * sis, GUARD, np.uint8)  # one leading byte: every row starts at an odd address
    for i in range(n):
        rows = buf[1 + i * sis:1 + i * sis + h * stride].reshape(h, stride)
        rows[:, :w * comps] = imgs[i].reshape(h, w * comps)
    out = torch.full((n, dis), GUARD, dtype=torch.uint8, device=dev)
    src = torch.from_numpy(buf).to(dev)[1:]
    flat, _ = pkg.encode_mips_device(B.BC5, src, h, w, comps, swap_rb=bool(swap), n_images=n, row_stride_bytes=stride,
                                     src_image_stride_bytes=sis, dst_image_stride_bytes=dis, out=out, mip_filter=NORMAL)
    torch.cuda.synchronize()
    got = flat.cpu().numpy()
    assert got.shape == (n, dis)
    for i in range(n):
        assert got[i, :total].tobytes() == N.oracle_chain(imgs[i], comps, swap), (comps, swap, i)
        assert (got[i, total:] == GUARD).all()


@pytest.mark.parametrize("h,w", N.SIZES)
def test_rg8_pixel_pyramid_equals_the_oracle_and_writes_nothing_else(dev, h, w):
    import torch
    img = N.gpu_image(h, w, 2, 0, 10 + N.SIZES.index((h, w)))
    per, _ = pkg.mip_pyramid_size(2, h, w)
    out = torch.full((1, per + 32), GUARD, dtype=torch.uint8, device=dev)
    flat, views = pkg.mip_pyramid_device(_dev(img, dev), h, w, 2, dst_image_stride_bytes=per + 32, out=out, mip_filter=NORMAL)
    torch.cuda.synchronize()
    got = flat.cpu().numpy()[0]
    assert len(views) == M.max_levels(h, w) - 1
    assert got[:per].tobytes() == N.pyramid_bytes(img), (h, w)
    assert (got[per:] == GUARD).all()


def test_named_quads_as_exact_bytes(dev):
    """The quads of the header through the kernel: level 1 of a 4 x 4 image that holds four of them."""
    import torch
    quads = [[(218, 128), (218, 128), (128, 218), (128, 218)], [(255, 255)] * 4,
             [(255, 255), (0, 0), (255, 0), (0, 255)], [(200, 60), (10, 250), (128, 128), (90, 30)]]
    img = np.zeros((4, 4, 2), np.uint8)
    for i, q in enumerate(quads):
        img[2 * (i // 2):2 * (i // 2) + 2, 2 * (i % 2):2 * (i % 2) + 2] = N.rg_quad(q)
    _, views = pkg.mip_pyramid_device(_dev(img, dev), 4, 4, 2, levels=2, mip_filter=NORMAL)
    torch.cuda.synchronize()
    assert views[0].cpu().numpy()[0].tolist() == [[[180, 180], [218, 218]], [[127, 127], [92, 110]]]


def test_filter_zero_gives_the_bytes_of_the_unfiltered_entry_point(dev):
    import torch
    lib = pkg.lib()
    for (h, w), index in (((64, 64), 30), ((129, 65), 31)):
        for comps in (2, 3, 4):
            d = _dev(N.gpu_image(h, w, comps, 0, index), dev)
            levels = pkg.mip_max_levels(h, w)
            total, _ = pkg.mip_chain_size(B.BC5, h, w)
            old = torch.zeros((total,), dtype=torch.uint8, device=dev)
            new = torch.zeros((total,), dtype=torch.uint8, device=dev)
            ws_bytes = pkg.mip_workspace_size(B.BC5, comps, h, w)
            ws = torch.zeros((max(ws_bytes, 1),), dtype=torch.uint8, device=dev)
            args = (h, w, w * comps, levels, 1, 0, 0, d.data_ptr())
            assert lib.icamd_encode_mips_device(B.BC5, 2, comps, 0, *args, old.data_ptr(), ws.data_ptr(), ws_bytes, None) == 0
            assert lib.icamd_encode_mips_filtered_device(B.BC5, 2, comps, 0, 0, *args, new.data_ptr(), ws.data_ptr(), ws_bytes, None) == 0
            torch.cuda.synchronize()
            assert torch.equal(old, new), (h, w, comps)


def test_normal_filter_is_refused_where_it_does_not_apply(dev):
    import torch
    import ic_testlib as T
    src = torch.zeros(64 * 64 * 4, dtype=torch.uint8, device=dev)
    for codec, comps in [(T.DXT1, 4), (T.DXT5, 4), (T.ETC1, 3), (B.BC4, 2)]:
        with pytest.raises(pkg.BackendError):
            pkg.encode_mips_device(codec, src, 64, 64, comps, mip_filter=NORMAL)
    for comps in (1, 3, 4):
        with pytest.raises(pkg.BackendError):
            pkg.mip_pyramid_device(src, 64, 64, comps, mip_filter=NORMAL)
