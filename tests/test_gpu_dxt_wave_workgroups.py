"""GPU tier (-m gpu): the wide DXT kernels launched one wave per workgroup (dxt_plan.h: grid.x = 4 x column tiles of 64 lanes,
a wave finds its 64 blocks from blockIdx.x), bit for bit against the oracle at the smallest geometries where that mapping can
go wrong: 129 block columns (the narrowest grid that takes the wide path: two full waves, a wave of one block, an empty
wave), one tile of four full waves, one block in a second tile, a partial block column, block rows that are partial or
single, several images per launch, padded rows, a block grid larger than the image, outputs off 8-byte alignment (the
non-temporal twins), and content on which single waves fall on either side of the wave-uniform shortcuts.
DXT1 from RGBA8 and RGB888 (two block rows per lane) and DXT5."""
import numpy as np
import pytest

import ic_testlib as T

pytestmark = pytest.mark.gpu

FORMS = [(T.DXT1, 4), (T.DXT1, 3), (T.DXT5, 4)]
FORM_IDS = ["dxt1-rgba8", "dxt1-rgb888", "dxt5"]
WIDTHS = [516, 1024, 1028, 1280, 1284, 2047, 4100]
HEIGHTS_AND_IMAGES = [(1, 1), (4, 2), (5, 3), (67, 2)]


@pytest.fixture(scope="module")
def env():
    import torch
    import ic_amd_loader
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch, ic_amd_loader.load_package()


def _encode(env, codec, flat, h, w, comps, n_images=1, stride=None, swap=False, out_offset=0, gh=None, gw=None):
    """One launch over n_images images packed in `flat` (bytes); out_offset > 0 moves the output off 8-byte alignment."""
    torch, pkg = env
    src = torch.from_numpy(np.ascontiguousarray(flat).reshape(-1)).cuda()
    per = pkg.encoded_size(codec, max(h, gh or h), max(w, gw or w))
    buf = torch.full((n_images * per + out_offset + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    out = buf[out_offset:out_offset + n_images * per]
    assert (out.data_ptr() % 8 == 0) == (out_offset % 8 == 0)
    res = pkg.encode_device(codec, src, h, w, comps, swap_rb=swap, row_stride_bytes=stride, n_images=n_images,
                            grid_height=gh, grid_width=gw, out=out)
    assert res is not None
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:out_offset] == 0xEE).all(), "bytes in front of the output were written"
    assert (host[out_offset + n_images * per:] == 0xEE).all(), "bytes behind the output were written"
    return host[out_offset:out_offset + n_images * per].reshape(n_images, per)


@pytest.mark.parametrize("codec,comps", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("w", WIDTHS)
def test_widths_heights_images(env, codec, comps, w):
    for h, n in HEIGHTS_AND_IMAGES:
        imgs = np.stack([T.s_mixed(h, w, comps, index=100 + 7 * h + i) for i in range(n)])
        got = _encode(env, codec, imgs, h, w, comps, n_images=n)
        for i in range(n):
            assert got[i].tobytes() == T.oracle_encode(codec, imgs[i], h, w, comps), "%d x %d, image %d" % (h, w, i)


@pytest.mark.parametrize("codec,comps", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("content", ["flat", "smooth"])
def test_content(env, codec, comps, content):
    """s_flat: waves of one-colour blocks beside waves with none (the constant-colour branch); s_smooth: the luminance range
    of the blocks differs from wave to wave, and every wave votes for itself."""
    h, w, n = 67, 1284, 2
    imgs = np.stack([T.GENERATORS[content](h, w, comps, index=120 + i) for i in range(n)])
    got = _encode(env, codec, imgs, h, w, comps, n_images=n)
    for i in range(n):
        assert got[i].tobytes() == T.oracle_encode(codec, imgs[i], h, w, comps), "image %d" % i


@pytest.mark.parametrize("codec,comps", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("pad", [4, 36, 4096])
def test_padded_rows(env, codec, comps, pad):
    h, w, n = 5, 1284, 2
    imgs = [T.s_mixed(h, w, comps, index=140 + i) for i in range(n)]
    flat = np.concatenate([T.with_row_padding(im, pad) for im in imgs])
    stride = w * comps + pad
    got = _encode(env, codec, flat, h, w, comps, n_images=n, stride=stride)
    for i in range(n):
        want = T.oracle_encode(codec, T.with_row_padding(imgs[i], pad), h, w, comps, stride=stride)
        assert got[i].tobytes() == want, "image %d" % i


def test_rows_of_4_mib(env):
    """Rows of 4 MiB take the wide kernels whatever the grid's width: 17 block columns are one wave of 17 blocks and three
    empty ones."""
    h, w, comps = 6, 68, 4
    pad = (1 << 22) - w * comps
    img = T.s_mixed(h, w, comps, index=150)
    flat = T.with_row_padding(img, pad)
    got = _encode(env, T.DXT1, flat, h, w, comps, stride=1 << 22)
    assert got[0].tobytes() == T.oracle_encode(T.DXT1, flat, h, w, comps, stride=1 << 22)


@pytest.mark.parametrize("codec,comps", FORMS, ids=FORM_IDS)
def test_swap_rb(env, codec, comps):
    h, w, n = 5, 1028, 2
    imgs = np.stack([T.s_mixed(h, w, comps, index=160 + i) for i in range(n)])
    got = _encode(env, codec, imgs, h, w, comps, n_images=n, swap=True)
    for i in range(n):
        assert got[i].tobytes() == T.oracle_encode(codec, imgs[i], h, w, comps, swap=1), "image %d" % i


@pytest.mark.parametrize("codec,comps", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("h,w,gh,gw", [(5, 516, 20, 1032), (67, 1020, 69, 1028), (4, 2047, 4, 2304)])
def test_padded_grid(env, codec, comps, h, w, gh, gw):
    """A block grid larger than the image: whole waves, and whole block rows, of blocks beyond the image."""
    img = T.s_mixed(h, w, comps, index=170)
    got = _encode(env, codec, img, h, w, comps, gh=gh, gw=gw)
    assert got[0].tobytes() == T.oracle_encode(codec, img, h, w, comps, gh=gh, gw=gw)


@pytest.mark.parametrize("comps", [4, 3])
@pytest.mark.parametrize("offset", [1, 4])
@pytest.mark.parametrize("h,w,n", [(5, 516, 3), (67, 1028, 2)])
def test_unaligned_output(env, comps, offset, h, w, n):
    """A DXT1 output that is not 8-byte aligned takes the non-temporal twins: the same bytes, nothing in front touched."""
    imgs = np.stack([T.s_mixed(h, w, comps, index=180 + i) for i in range(n)])
    shifted = _encode(env, T.DXT1, imgs, h, w, comps, n_images=n, out_offset=offset)
    for i in range(n):
        assert shifted[i].tobytes() == T.oracle_encode(T.DXT1, imgs[i], h, w, comps), "image %d" % i
