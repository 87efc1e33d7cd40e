"""CPU tier of the DXT launch form (image-compression_amd/csrc/dxt_plan.h): which workgroup size and grid.x a DXT1 / DXT5 encode
gets -- 256-lane workgroups, or every wave of a 256-block tile as its own 64-lane workgroup -- is host-only arithmetic, so it is
pinned here, without a GPU.  tests/host_emul/dxt_plan_driver.cc, built with g++ against the header alone, prints the form for the
block grids of 128, 129, 256, 257 and 1024 columns: 128 is the widest grid of the narrow kernels, 129 the narrowest of the wide
ones (one tile: two full waves, a wave of one block, an empty wave), 257 puts one block into a second tile."""
import os
import subprocess

import pytest

import ic_testlib as T

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(T.ROOT, "image-compression_amd", "csrc")
COLS = [128, 129, 256, 257, 1024]
KEYS = "log2_tile_cols wide_rows wave_workgroups lanes grid_x".split()


@pytest.fixture(scope="module")
def form(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("dxt_plan")), "dxt_plan_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, "-I" + os.path.join(T.ROOT, "include"),
                           "-o", exe, os.path.join(HERE, "host_emul", "dxt_plan_driver.cc")])

    def run(codec, comps, block_cols, row_stride=None):
        stride = block_cols * 4 * comps if row_stride is None else row_stride
        out = subprocess.check_output([exe] + [str(v) for v in (codec, comps, block_cols, stride)]).decode()
        return dict(zip(KEYS, map(int, out.split())))
    return run


def test_the_header_needs_nothing_from_hip():
    text = open(os.path.join(CSRC, "dxt_plan.h")).read()
    includes = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
    assert sorted(includes) == ['"etc2_mip_plan.h"', "<cstdint>"]
    for word in ("hipGetDevice", "getenv", "hipError_t", "dim3", "hipLaunch"):
        assert word not in text


@pytest.mark.parametrize("block_cols,grid_x", zip(COLS, [1, 4, 4, 8, 16]))
def test_dxt1_rgba8_wide_grids_are_one_wave_workgroups(form, block_cols, grid_x):
    f = form(T.DXT1, 4, block_cols)
    wide = block_cols > 128
    assert f == dict(log2_tile_cols=8 if wide else 7, wide_rows=1, wave_workgroups=int(wide), lanes=64 if wide else 256, grid_x=grid_x)
    # whole tiles of 256 blocks either way: 64 lanes x grid.x covers what 256 lanes x column tiles covered
    if wide:
        assert f["lanes"] * f["grid_x"] == 256 * -(-block_cols // 256)


@pytest.mark.parametrize("codec,comps,wide_rows", [(T.DXT1, 3, 2), (T.DXT5, 4, 1)])
@pytest.mark.parametrize("block_cols,grid_x", zip(COLS, [1, 1, 1, 2, 4]))
def test_the_siblings_keep_256_lanes(form, codec, comps, wide_rows, block_cols, grid_x):
    f = form(codec, comps, block_cols)
    assert f == dict(log2_tile_cols=8 if block_cols > 128 else 7, wide_rows=wide_rows, wave_workgroups=0, lanes=256, grid_x=grid_x)


def test_rows_too_long_for_narrow_tiles(form):
    """Rows of 4 MiB and more take the wide kernels whatever the grid's width (encode_tile_shape): 16 block columns are one wave of
    16 blocks and three empty ones."""
    f = form(T.DXT1, 4, 16, row_stride=1 << 22)
    assert f == dict(log2_tile_cols=8, wide_rows=1, wave_workgroups=1, lanes=64, grid_x=4)
    assert form(T.DXT1, 4, 16)["lanes"] == 256 and form(T.DXT1, 4, 16)["log2_tile_cols"] == 4
