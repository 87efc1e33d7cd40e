"""GPU tier (-m gpu): DXT1 encodes whose blocks are written through to memory (icamd_dxt1_rgba8_kernel and
icamd_dxt1_rgb888_x2_kernel with an 8-byte aligned output) and their non-temporal twins (any other output pointer),
bit for bit against the oracle at the headline's launch shape and at the geometries the wide kernels cover."""
import numpy as np
import pytest

import ic_testlib as T

pytestmark = pytest.mark.gpu

GEN = {"noise": T.s_noise, "smooth": T.s_smooth, "flat": T.s_flat}


@pytest.fixture(scope="module")
def env():
    import torch
    import ic_amd_loader
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch, ic_amd_loader.load_package()


def _encode(env, flat, h, w, comps, n_images=1, stride=None, swap=False, out_offset=0, gh=None, gw=None):
    """One launch over n_images images packed in `flat` (bytes); out_offset > 0 moves the output off 8-byte alignment."""
    torch, pkg = env
    src = torch.from_numpy(np.ascontiguousarray(flat).reshape(-1)).cuda()
    per = pkg.encoded_size(T.DXT1, max(h, gh or h), max(w, gw or w))
    buf = torch.full((n_images * per + out_offset,), 0xEE, dtype=torch.uint8, device="cuda")
    out = buf[out_offset:]
    assert (out.data_ptr() % 8 == 0) == (out_offset % 8 == 0)
    res = pkg.encode_device(T.DXT1, src, h, w, comps, swap_rb=swap, row_stride_bytes=stride, n_images=n_images,
                            grid_height=gh, grid_width=gw, out=out)
    assert res is not None
    torch.cuda.synchronize()
    if out_offset:
        assert (buf[:out_offset].cpu().numpy() == 0xEE).all(), "bytes in front of the output were written"
    return out.cpu().numpy().reshape(n_images, per)


@pytest.mark.parametrize("content", ["noise", "smooth", "flat"])
def test_headline_batch(env, content):
    """16 x 4096^2 RGBA8 in one launch (the benchmark's shape); every image differs."""
    n, size = 16, 4096
    base = [GEN[content](size, size, 4, index=i) for i in range(4)]
    imgs = np.empty((n, size, size, 4), np.uint8)
    for j in range(n):
        imgs[j] = np.roll(base[j % 4], 4 * 37 * (j // 4) + 1, axis=1)
    got = _encode(env, imgs, size, size, 4, n_images=n)
    for j in range(n):
        want = T.oracle_encode(T.DXT1, imgs[j], size, size, 4, threads=8)
        assert got[j].tobytes() == want, "image %d (%s)" % (j, content)


def test_8192(env):
    img = T.s_mixed(8192, 8192, 4, index=11)
    got = _encode(env, img, 8192, 8192, 4)
    assert got[0].tobytes() == T.oracle_encode(T.DXT1, img, 8192, 8192, 4, threads=8)


# widths that are not a multiple of 1024 (a partial last tile) or of 4 (a partial last block column), heights whose last
# block row is partial, several images per launch
@pytest.mark.parametrize("comps", [4, 3])
@pytest.mark.parametrize("h,w,n", [(67, 1030, 3), (130, 4099, 2), (9, 2050, 5), (1025, 1025, 1), (4, 1024, 7)])
def test_widths_and_partial_rows(env, comps, h, w, n):
    imgs = np.stack([T.s_mixed(h, w, comps, index=20 + i) for i in range(n)])
    got = _encode(env, imgs, h, w, comps, n_images=n)
    for i in range(n):
        assert got[i].tobytes() == T.oracle_encode(T.DXT1, imgs[i], h, w, comps), "image %d" % i


@pytest.mark.parametrize("comps", [4, 3])
@pytest.mark.parametrize("pad", [4, 36, 4096])
def test_padded_rows(env, comps, pad):
    h, w, n = 70, 1284, 2
    imgs = [T.s_mixed(h, w, comps, index=40 + i) for i in range(n)]
    flat = np.concatenate([T.with_row_padding(im, pad) for im in imgs])
    stride = w * comps + pad
    got = _encode(env, flat, h, w, comps, n_images=n, stride=stride)
    for i in range(n):
        want = T.oracle_encode(T.DXT1, T.with_row_padding(imgs[i], pad), h, w, comps, stride=stride)
        assert got[i].tobytes() == want, "image %d" % i


@pytest.mark.parametrize("comps", [4, 3])
def test_swap_rb(env, comps):
    h, w, n = 132, 2052, 2
    imgs = np.stack([T.s_mixed(h, w, comps, index=60 + i) for i in range(n)])
    got = _encode(env, imgs, h, w, comps, n_images=n, swap=True)
    for i in range(n):
        assert got[i].tobytes() == T.oracle_encode(T.DXT1, imgs[i], h, w, comps, swap=1), "image %d" % i


@pytest.mark.parametrize("comps", [4, 3])
def test_padded_grid(env, comps):
    """A block grid larger than the image (CompressAndPad): the extra blocks are written through as well."""
    h, w, gh, gw = 61, 1030, 80, 1100
    img = T.s_mixed(h, w, comps, index=70)
    got = _encode(env, img, h, w, comps, gh=gh, gw=gw)
    assert got[0].tobytes() == T.oracle_encode(T.DXT1, img, h, w, comps, gh=gh, gw=gw)


@pytest.mark.parametrize("comps", [4, 3])
@pytest.mark.parametrize("offset", [1, 4])
def test_unaligned_output(env, comps, offset):
    """An output that is not 8-byte aligned takes the non-temporal kernels and gives the same bytes."""
    h, w, n = 68, 2048, 3
    imgs = np.stack([T.s_mixed(h, w, comps, index=80 + i) for i in range(n)])
    aligned = _encode(env, imgs, h, w, comps, n_images=n)
    shifted = _encode(env, imgs, h, w, comps, n_images=n, out_offset=offset)
    assert shifted.tobytes() == aligned.tobytes()
    for i in range(n):
        assert aligned[i].tobytes() == T.oracle_encode(T.DXT1, imgs[i], h, w, comps), "image %d" % i
