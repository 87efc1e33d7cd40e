"""GPU tier of the mip-chain plan (image-compression_amd/csrc/mip_plan.h): the paths the plan decides and no other test runs --
pass boundaries on thin images (two and three passes, a last pass of one tile with eight local levels), and launches cut at 65 535
images and at 65 535 tile rows.  Expected bytes come from the oracles of the other mip tests (mips_oracle, mip_filter_oracle,
normal_filter_oracle).  The output is followed by guard bytes (0xa5), and the workspace is exactly icamd_mip_workspace_size bytes,
followed by a guard."""
import importlib

import numpy as np
import pytest

import bc45_oracle as B
import ic_testlib as T
import mip_filter_oracle as F
import mips_oracle as M
import normal_filter_oracle as N

pytestmark = pytest.mark.gpu
pkg = importlib.import_module("image-compression_amd")
GUARD, GUARD_BYTES = 0xA5, 256
NORMAL = 4
PYRAMID = None  # `codec` of the pixel-pyramid cases below
# (129, 1): the smallest two-pass chain; (1, 8192): a second pass of one tile with eight local levels; (1, 16384) and (16385, 3):
# three passes each
THIN = [(129, 1), (1, 8192), (1, 16384), (16385, 3)]
LEVELS = [6, 7, 8, 12, 13]
CONFIGS = [(T.DXT1, 4, 0), (T.DXT5, 4, 3), (B.BC4, 1, 0), (B.BC5, 2, NORMAL), (T.ETC1, 3, 1),
           (PYRAMID, 1, 0), (PYRAMID, 2, 0), (PYRAMID, 3, 0), (PYRAMID, 4, 0), (PYRAMID, 4, 3), (PYRAMID, 2, NORMAL)]


@pytest.fixture(scope="module")
def dev():
    import torch
    d = torch.device("cuda:0")
    torch.cuda.set_device(d)
    return d


def _pyramid(img, mip_filter):
    return N.pyramid(img) if mip_filter == NORMAL else F.pyramid(img, mip_filter) if mip_filter else M.pyramid(img)


def _expected_levels(codec, img, comps, mip_filter):
    """The bytes of every level of the full chain (or, codec PYRAMID, of levels 1 ..): a shorter chain is a prefix of them."""
    pyr = _pyramid(img, mip_filter)
    if codec is PYRAMID:
        return [p.tobytes() for p in pyr[1:]]
    return [M.oracle_encode(codec, p, comps) for p in pyr]


def _guarded(n_bytes, dev):
    import torch
    return torch.full((n_bytes + GUARD_BYTES,), GUARD, dtype=torch.uint8, device=dev)


def _run(codec, imgs, comps, mip_filter, levels, dev, pad=0, src_gap=0, dst_gap=0):
    """The call on the images (equal shapes) with rows padded by `pad` bytes and image strides `src_gap` / `dst_gap` bytes wider
    than an image: [n, per] output bytes, after the guards and the gaps were checked."""
    import torch
    n = len(imgs)
    h, w = imgs[0].shape[:2]
    stride = w * comps + pad
    sis = h * stride + src_gap
    src = np.full(n * sis, 0x5A, np.uint8)
    for i, img in enumerate(imgs):
        rows = src[i * sis:i * sis + h * stride].reshape(h, stride)
        rows[:, :w * comps] = img.reshape(h, w * comps)
    per = pkg.mip_pyramid_size(comps, h, w, levels)[0] if codec is PYRAMID else pkg.mip_chain_size(codec, h, w, levels)[0]
    dis = per + dst_gap
    out = _guarded(n * dis, dev)
    kw = dict(levels=levels, n_images=n, row_stride_bytes=stride, src_image_stride_bytes=sis, dst_image_stride_bytes=dis,
              out=out[:n * dis].view(n, dis), mip_filter=mip_filter)
    d_src = torch.from_numpy(src).to(dev)
    if codec is PYRAMID:
        assert pkg.mip_pyramid_device(d_src, h, w, comps, **kw) is not None
    else:
        need = pkg.mip_workspace_size(codec, comps, h, w, levels, n)
        ws = _guarded(need, dev)
        assert pkg.encode_mips_device(codec, d_src, h, w, comps, workspace=ws[:need] if need else None, **kw) is not None
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[n * dis:] == GUARD).all(), "wrote past the output"
    if codec is not PYRAMID:
        assert (ws.cpu().numpy()[need:] == GUARD).all(), "wrote past icamd_mip_workspace_size bytes of workspace"
    got = got[:n * dis].reshape(n, dis)
    assert (got[:, per:] == GUARD).all(), "wrote between the images"
    return got[:, :per]


@pytest.mark.parametrize("codec,comps,mip_filter", CONFIGS)
def test_pass_boundaries_on_thin_images(dev, codec, comps, mip_filter):
    rng = np.random.default_rng(1000 * comps + 10 * mip_filter + (0 if codec is PYRAMID else 1 + codec))
    for h, w in THIN:
        imgs = [rng.integers(0, 256, (h, w, comps), dtype=np.uint8) for _ in range(3)]
        want = [_expected_levels(codec, img, comps, mip_filter) for img in imgs]
        first = 1 if codec is PYRAMID else 0  # want[i][k] is level first + k
        top = M.max_levels(h, w)
        for levels in [l for l in LEVELS if l < top] + [top]:
            got = _run(codec, imgs[:1], comps, mip_filter, levels, dev)
            assert got[0].tobytes() == b"".join(want[0][:levels - first]), (codec, comps, mip_filter, h, w, levels)
        # three images, padded rows, image strides wider than an image: every handoff region holds three images
        got = _run(codec, imgs, comps, mip_filter, top, dev, pad=5, src_gap=40, dst_gap=24)
        for i in range(3):
            assert got[i].tobytes() == b"".join(want[i]), (codec, comps, mip_filter, h, w, i)


def test_more_than_65535_images(dev):
    """65 537 RGBA8 images of 4 x 4, tiled from eight distinct ones: grid.z takes 65 535 of them and then 2."""
    n, h, w, levels = 65537, 4, 4, 3
    rng = np.random.default_rng(65537)
    eight = [rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for _ in range(8)]
    imgs = [eight[i % 8] for i in range(n)]
    for codec in (T.DXT1, PYRAMID):
        want = [np.frombuffer(b"".join(_expected_levels(codec, img, 4, 0)), np.uint8) for img in eight]
        got = _run(codec, imgs, 4, 0, levels, dev)
        assert got.shape == (n, 24 if codec == T.DXT1 else 20)
        assert np.array_equal(got, np.stack([want[i % 8] for i in range(n)])), codec


def test_more_than_65535_tile_rows(dev):
    """One R8 image of 8 388 611 x 1: more than 65 535 tile rows, so grid.y is cut (MipParams::tile_row0), and four passes.  The
    pyramid against numpy; the BC4 chain against icamd_encode_device of each level of that pyramid (as test_4096_square)."""
    import torch
    h, w = 8388611, 1
    rng = np.random.default_rng(8388611)
    img = rng.integers(0, 256, (h, w, 1), dtype=np.uint8)
    levels = M.max_levels(h, w)
    assert levels == 24 and -(-h // 128) > 65535
    pyr = M.pyramid(img)
    got = _run(PYRAMID, [img], 1, 0, levels, dev)
    assert got[0].tobytes() == b"".join(p.tobytes() for p in pyr[1:])
    got = _run(B.BC4, [img], 1, 0, levels, dev)[0]
    offs = pkg.mip_chain_size(B.BC4, h, w, levels)[1]
    for l, p in enumerate(pyr):
        lh, lw = p.shape[:2]
        want = pkg.encode_device(B.BC4, torch.from_numpy(np.ascontiguousarray(p).reshape(-1)).to(dev), lh, lw, 1)
        assert np.array_equal(got[offs[l]:offs[l + 1]], want.cpu().numpy()[0]), l
