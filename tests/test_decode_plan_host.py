"""CPU tier of the cut of a decode or metric call into launches (image-compression_amd/csrc/decode_plan.h): whole images, as many
per launch as stay below 2^31 blocks, or bands of block rows of one image of 2^31 blocks or more.  The banded launches need 16 GiB
of blocks and more, so no GPU test reaches the bands (the whole-image groups of a call of more than 2^31 - 1 blocks run in
tests/test_gpu_walk_regimes.py, on images that overlap); the cut is host-only arithmetic and is pinned here.
tests/host_emul/decode_plan_driver.cc, built with g++ against the header alone, prints the pieces.  The expected lists are worked
out by hand from the rules (groups of max(1, limit // blocks_per_image) images; bands of limit // block_cols block rows, the last
one height - 4 * first_block_row pixel rows), not taken from a run.

The small limits (7 and 64 blocks) run over those shapes of the table whose block row fits the limit -- a band is whole block
rows, so no cut of a wider grid can hold every piece to the limit, and no entry point has such a grid: block_cols <= 2^30 -- and
over the table's large shapes scaled down to the same relations between blocks_per_image and the limit."""
import os
import subprocess

import pytest

import ic_testlib as T

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(T.ROOT, "image-compression_amd", "csrc")
LIMIT = 2 ** 31 - 1


def cols4(width):
    return (width + 3) // 4


# (name, height, block_cols, n_images, expected pieces (first_image, image_count, first_block_row, pixel_rows))
CASES = [
    ("small image", 4, cols4(4), 1, [(0, 1, 0, 4)]),
    ("partial blocks", 9, cols4(13), 3, [(0, 3, 0, 9)]),
    # 2^29 blocks per image: 3 images are 3 * 2^29 < 2^31, 4 are not
    ("2^29 blocks", 4 * 16384, 32768, 5, [(0, 3, 0, 65536), (3, 2, 0, 65536)]),
    ("2^30 blocks", 4 * 32768, 32768, 3, [(0, 1, 0, 131072), (1, 1, 0, 131072), (2, 1, 0, 131072)]),
    ("2^31 - 32768 blocks", 4 * 65535, 32768, 2, [(0, 1, 0, 262140), (1, 1, 0, 262140)]),
    # exactly 2^31 blocks, one more than a launch holds: (2^31 - 1) // 32768 = 65535 block rows, then the last one
    ("2^31 blocks", 4 * 65536, 32768, 1, [(0, 1, 0, 262140), (0, 1, 65535, 4)]),
    ("2^31 blocks, partial last row", 4 * 65536 - 1, 32768, 1, [(0, 1, 0, 262140), (0, 1, 65535, 3)]),
    ("2^31 blocks, two images", 4 * 65536, 32768, 2,
     [(0, 1, 0, 262140), (0, 1, 65535, 4), (1, 1, 0, 262140), (1, 1, 65535, 4)]),
    # the widest row: 2^30 block columns, one block row per band
    ("widest row", 9, cols4(2 ** 32 - 1), 1, [(0, 1, 0, 4), (0, 1, 1, 4), (0, 1, 2, 1)]),
    # PVRTC 2 bpp at 65536^2: 8 x 4-pixel blocks, 8192 x 16384 = 2^27 of them
    ("pvrtc 2 bpp pitch", 65536, 65536 // 8, 1, [(0, 1, 0, 65536)]),
]
# the large shapes at a limit of 64 blocks: (height, block_cols, n_images), blocks per image in the comment
SCALED = [
    (4 * 4, 4, 5),      # 16: groups of 4 and 1
    (4 * 8, 4, 3),      # 32: groups of 2 and 1
    (4 * 7, 8, 2),      # 56 = limit - block_cols: whole images, one per piece
    (4 * 8, 8, 2),      # 64 = limit: whole images, one per piece
    (4 * 8 + 1, 8, 2),  # 72: bands of 8 block rows, then one of 1 pixel row
    (4 * 9 - 1, 8, 1),  # 72: the last band has 3 pixel rows
    (9, 64, 1),         # a row is the limit: one block row per band
    (9, 33, 2),         # 99: bands of one block row, 31 blocks of the limit unused
]


@pytest.fixture(scope="module")
def pieces(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("decode_plan")), "decode_plan_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, "-o", exe,
                           os.path.join(HERE, "host_emul", "decode_plan_driver.cc")])

    def run(height, block_cols, n_images, limit=0, stop_after=0):
        lines = subprocess.check_output([exe] + [str(v) for v in (height, block_cols, n_images, limit, stop_after)]).decode().split("\n")
        assert lines[-1] == "" and lines[-2].startswith("rc ")
        return [tuple(map(int, l.split())) for l in lines[:-2]], int(lines[-2][3:])
    return run


def check_cover(got, height, block_cols, n_images, limit):
    """Every block row of every image exactly once and in order, at most `limit` blocks per piece, 32-bit block counts."""
    block_rows = (height + 3) // 4
    per_image = block_rows * block_cols
    image, row = 0, 0  # the next block row a piece must begin at
    for first_image, count, row0, pixel_rows in got:
        assert (first_image, row0) == (image, row) and count >= 1 and pixel_rows >= 1
        rows = (pixel_rows + 3) // 4
        assert count * rows * block_cols <= limit
        assert count * per_image < 2 ** 32
        if row0 == 0 and pixel_rows == height:  # whole images
            image += count
        else:  # a band: whole block rows, but for the image's last
            assert count == 1 and (pixel_rows % 4 == 0 or row0 * 4 + pixel_rows == height)
            row += rows
            if row == block_rows:
                image, row = image + 1, 0
            assert row0 * 4 + pixel_rows <= height
    assert (image, row) == (n_images, 0)


def test_the_header_needs_nothing_from_hip():
    text = open(os.path.join(CSRC, "decode_plan.h")).read()
    includes = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
    assert includes == ["<cstdint>"]
    for word in ("hipGetDevice", "getenv", "hipError_t", "dim3", "hipLaunch", "hipStream_t", "std::vector", "new "):
        assert word not in text


@pytest.mark.parametrize("name,height,block_cols,n_images,want", CASES, ids=[c[0] for c in CASES])
def test_the_pieces_of_a_call(pieces, name, height, block_cols, n_images, want):
    got, rc = pieces(height, block_cols, n_images)
    assert rc == 0 and got == want
    check_cover(got, height, block_cols, n_images, LIMIT)


@pytest.mark.parametrize("limit", [7, 64])
def test_small_limits_cover_the_same_shapes(pieces, limit):
    shapes = [(h, c, n) for _, h, c, n, _ in CASES if c <= limit] + [(h, c, n) for h, c, n in SCALED if c <= limit]
    assert len(shapes) >= (3 if limit == 7 else 10)
    for height, block_cols, n_images in shapes:
        got, rc = pieces(height, block_cols, n_images, limit)
        assert rc == 0
        check_cover(got, height, block_cols, n_images, limit)


def test_the_scaled_shapes_cut_as_the_large_ones(pieces):
    assert pieces(16, 4, 5, 64)[0] == [(0, 4, 0, 16), (4, 1, 0, 16)]
    assert pieces(28, 8, 2, 64)[0] == [(0, 1, 0, 28), (1, 1, 0, 28)]
    assert pieces(32, 8, 2, 64)[0] == [(0, 1, 0, 32), (1, 1, 0, 32)]
    assert pieces(33, 8, 2, 64)[0] == [(0, 1, 0, 32), (0, 1, 8, 1), (1, 1, 0, 32), (1, 1, 8, 1)]
    assert pieces(35, 8, 1, 64)[0] == [(0, 1, 0, 32), (0, 1, 8, 3)]
    with pytest.raises(subprocess.CalledProcessError):  # the driver refuses a block row wider than the limit
        pieces(9, 13, 3, 7)


def test_a_failed_launch_ends_the_walk(pieces):
    """The callback's first result other than 0 comes back and no later piece is visited: whole-image groups and bands."""
    assert pieces(4 * 32768, 32768, 3, 0, 2) == ([(0, 1, 0, 131072), (1, 1, 0, 131072)], 7)
    assert pieces(4 * 65536, 32768, 2, 0, 3) == ([(0, 1, 0, 262140), (0, 1, 65535, 4), (1, 1, 0, 262140)], 7)


def test_no_images_no_pieces(pieces):
    assert pieces(9, 4, 0) == ([], 0)
