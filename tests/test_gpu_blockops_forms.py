"""GPU tier (-m gpu): the launch forms of the compressed-domain operations that the other GPU tests do not reach
(image-compression_amd/csrc/blockops_plan.h lists them): the row-tile Downsample kernels (grids of 256 output columns and
more), Pad with nothing to add, CopySubimage past 65 535 block rows, CreateSolid past the single fill's workgroup cap, and a
batched CreateSolid of more than one launch.  Everything is compared with the project's own oracle, or with a numpy restatement
where the operation is a copy."""
import numpy as np
import pytest

import ic_testlib as T

pytestmark = pytest.mark.gpu

CODECS = {"dxt1": (T.DXTC, T.RGB, T.DXT1, 8, T.SMALLER_ERROR), "dxt5": (T.DXTC, T.RGBA, T.DXT5, 16, T.SMALLER_ERROR),
          "etc1_heuristic": (T.ETC, T.RGB, T.ETC1, 8, T.HEURISTIC)}


@pytest.fixture(scope="module")
def pkg():
    import torch
    import ic_amd_loader
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return ic_amd_loader.load_package()


def to_device(array):
    import torch
    return torch.from_numpy(np.ascontiguousarray(array)).to("cuda:0")


def source_blocks(codec, block_bytes, h, w, index):
    """One h x w image's blocks: arbitrary block words for DXT, oracle-compressed mixed content for ETC1."""
    if codec == T.ETC1:
        return np.frombuffer(T.oracle_encode(T.ETC1, T.s_mixed(h, w, 3, index=index), h, w, 3), np.uint8).copy()
    rng = np.random.default_rng(1000 + index)
    return rng.integers(0, 256, (h // 4) * (w // 4) * block_bytes, dtype=np.uint8)


# 2 x 256 output blocks: exactly one column tile; 1 x 257: the second tile has one live lane; 1 x 255: the linear form
@pytest.mark.parametrize("h,w", [(16, 2048), (8, 2056), (8, 2040)])
@pytest.mark.parametrize("name", sorted(CODECS))
def test_downsample_across_the_row_tile_threshold(pkg, name, h, w):
    compressor, fmt, codec, block_bytes, strategy = CODECS[name]
    images = [source_blocks(codec, block_bytes, h, w, i) for i in range(3)]
    want = [T.oracle_downsample(compressor, fmt, im.tobytes(), h, w, strategy) for im in images]
    got = pkg.downsample_device(compressor, fmt, to_device(images[0]).view(1, -1), h, w, etc_strategy=strategy)
    assert got is not None and got.cpu().numpy().tobytes() == want[0]
    # three images on a padded image stride
    padded = np.full((3, images[0].size + 24), 0xa5, np.uint8)
    for i, im in enumerate(images):
        padded[i, :im.size] = im
    got = pkg.downsample_device(compressor, fmt, to_device(padded), h, w, etc_strategy=strategy, n_images=3)
    assert got is not None
    for i in range(3):
        assert got[i].cpu().numpy().tobytes() == want[i], "image %d" % i


@pytest.mark.parametrize("compressor,fmt,codec,strategy", [(T.DXTC, T.RGB, T.DXT1, T.SMALLER_ERROR), (T.ETC, T.RGB, T.ETC1, T.SPLIT_H),
                                                           (T.ETC, T.RGB, T.ETC1, T.SPLIT_V), (T.ETC, T.RGB, T.ETC1, T.SMALLER_ERROR),
                                                           (T.ETC, T.RGB, T.ETC1, T.HEURISTIC)])
def test_pad_with_nothing_to_add_is_the_copy(pkg, compressor, fmt, codec, strategy):
    h, w = 20, 36  # 5 x 9 blocks
    images = np.stack([source_blocks(codec, 8, h, w, 10 + i) for i in range(3)])
    for n in (1, 3):
        got = pkg.pad_batch_device(compressor, fmt, to_device(images[:n]), h, w, h, w, etc_strategy=strategy)
        assert got is not None and np.array_equal(got.cpu().numpy(), images[:n]), "%d images" % n
        assert images[0].tobytes() == T.oracle_pad(compressor, fmt, images[0].tobytes(), h, w, h, w, strategy)


def test_copy_subimage_past_65535_block_rows(pkg):
    rows, cols = 65538, 2
    grid = np.random.default_rng(7).integers(0, 256, (rows, cols, 8), dtype=np.uint8)
    got = pkg.copy_subimage_device(T.DXTC, T.RGB, to_device(grid.reshape(-1)), rows * 4, cols * 4, 4, 0, 65536 * 4, 4)
    assert got is not None and np.array_equal(got.cpu().numpy().reshape(65536, 8), grid[1:65537, 0])


def test_create_solid_past_the_fill_workgroup_cap(pkg):
    h, w, color = 8196, 8192, (200, 100, 50)  # 4 196 352 blocks: more than 16 384 workgroups of 256
    block = np.frombuffer(T.oracle_create_solid(T.DXTC, T.RGB, 4, 4, color), np.uint8)
    got = pkg.create_solid_device(T.DXTC, T.RGB, h, w, color)
    assert got is not None and got.numel() == 4196352 * 8
    assert np.array_equal(got.cpu().numpy().reshape(-1, 8), np.broadcast_to(block, (4196352, 8)))


def test_batched_create_solid_of_more_than_one_launch(pkg):
    h, w, n = 768, 772, 70  # 37 056 blocks per image: more than the 128 workgroups per image of a 64-image launch cover at once
    colors = [(3 * i, 255 - 2 * i, 7 * i % 256) for i in range(n)]
    got = pkg.create_solid_batch_device(T.DXTC, T.RGB, h, w, colors)
    assert got is not None
    got = got.cpu().numpy().reshape(n, -1, 8)
    assert got.shape[1] == 192 * 193
    for i, color in enumerate(colors):
        block = np.frombuffer(T.oracle_create_solid(T.DXTC, T.RGB, 4, 4, color), np.uint8)
        assert np.array_equal(got[i], np.broadcast_to(block, got[i].shape)), "image %d" % i
