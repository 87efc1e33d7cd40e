"""CPU tier of the block-walk cases (tests/walk_cases.py): the walk of the decode and metric kernels restated in numpy -- which
image each lane of each wave of each quarter of each workgroup holds, img_last in the lanes without a block -- and every regime
held to the properties it is named for, so that a shape edited out of its regime fails here.  Every family's definition is
computed once, and a few images of it through the oracle module's own call on the image alone.  The shapes of more than
2^31 - 1 blocks are held to their cut with tests/host_emul/decode_plan_driver.cc, and the additive shortcut their expected
records are built with to the oracle's metric of a whole image."""
import os
import subprocess

import numpy as np
import pytest

import ic_testlib as T
import walk_cases as K

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(T.ROOT, "image-compression_amd", "csrc")
METRIC = {r.name: r for r in K.METRIC_REGIMES}
DECODE = {r.name: r for r in K.DECODE_REGIMES}


def _metric(name):
    r = METRIC[name]
    return r, K.classify(r.rows * r.cols, r.n)


# ---- the table

def test_the_table_lists_every_kernel_of_the_three_launchers():
    """The (codec, components) pairs of kMetricKernels, ICAMD_EAC16_METRIC_KERNELS and ICAMD_BC6H_KERNELS, read from the sources:
    each has exactly one family (the PVRTC raster forms share theirs with the tile forms)."""
    import re
    import bc6h_oracle as B6
    import eac11_16_oracle as E16
    enum = {"DXT1": K.DXT1, "DXT5": K.DXT5, "ETC1": K.ETC1, "PVRTC2": K.PVRTC2, "PVRTC4": K.PVRTC4, "BC4": K.BC4, "BC5": K.BC5,
            "ETC2_RGBA8": K.ETC2_RGBA8, "ETC2_RGB8": K.ETC2_RGB8, "ETC2_RGB8A1": K.ETC2_RGB8A1, "EAC_R11": K.EAC_R11,
            "EAC_RG11": K.EAC_RG11, "BC7": K.BC7, "EAC_SIGNED_R11": E16.EAC_SIGNED_R11, "EAC_SIGNED_RG11": E16.EAC_SIGNED_RG11,
            "BC6H_UF16": B6.BC6H_UF16, "BC6H_SF16": B6.BC6H_SF16}

    def read(name):
        return open(os.path.join(CSRC, name)).read()
    listed = {}
    listed["measure_error_device"] = re.findall(r"ICAMD_METRIC_ENTRY\(ICAMD_(\w+), (\d), icamd_", read("metric_kernels.hip"))
    listed["measure_error_eac11_16_device"] = re.findall(r"X\(icamd_metric_\w+, ICAMD_(\w+), (\d)\)", read("eac11_16_kernels.hip"))
    listed["measure_error_bc6h_device"] = re.findall(r"X\(bc6h_\w+, ICAMD_(\w+), (\d), \w+\)", read("bc6h_kernels.hip"))
    assert [len(v) for v in listed.values()] == [27, 14, 4]
    for entry, pairs in listed.items():
        table = sorted((F.codec, F.comps) for F in K.METRIC_FAMILIES if F.entry == entry)
        assert table == sorted((enum[c], int(n)) for c, n in pairs), entry
    assert len({F.name for F in K.FAMILIES}) == len(K.FAMILIES)


def test_every_family_runs_in_every_regime():
    for F in K.FAMILIES:
        names = [r.name for r in K.regimes(F)]
        if K.is_pvrtc(F):
            assert names == ["pvrtc_8", "pvrtc_64", "pvrtc_128", "pvrtc_256"]
        else:
            assert names == [r.name for r in (K.METRIC_REGIMES if F.kind == "metric" else K.DECODE_REGIMES)]


# ---- the metric regimes: 1024 blocks a workgroup, four quarters of 256, waves of 64

def test_one_short_has_one_lane_without_a_block():
    r, c = _metric("one_short")
    assert r.rows * r.cols == 1023 and r.n == 1
    assert c["workgroups"] == 1 and c["one_image_workgroups"] == [0] and c["last_wave_with_blocks"] == (1, 1)


def test_exact_fills_one_workgroup():
    r, c = _metric("exact")
    assert c["workgroups"] == 1 and c["blocks_in_last_workgroup"] == 1024 and c["one_image_workgroups"] == [0]


def test_one_over_leaves_one_block_to_the_second_workgroup():
    r, c = _metric("one_over")
    assert r.n == 1 and c["workgroups"] == 2 and c["one_image_workgroups"] == [0, 1]
    assert c["blocks_in_last_workgroup"] == 1 and c["quarters_without_a_block_in_last_workgroup"] == 3
    assert c["last_wave_with_blocks"] == (1, 63)  # and the quarter's other three waves are empty: 255 lanes bring nothing


def test_image_per_workgroup_commits_to_images_other_than_the_first():
    r, c = _metric("image_per_workgroup")
    assert c["one_image_workgroups"] == [0, 1, 2] and c["one_image_workgroup_images"] == [0, 1, 2]
    assert c["blocks_in_last_workgroup"] == 1024


def test_waves_agree_in_workgroups_that_span_images():
    r, c = _metric("waves_agree")
    assert c["workgroups"] == 2 and c["one_image_workgroups"] == []
    assert c["waves_that_agree"] == 32 and c["waves_that_disagree"] == 0
    assert c["waves_that_agree_on_another_image_than_img_last"] == 17 and c["empty_waves"] == 11


def test_waves_split_between_the_wave_and_the_lane_commit():
    r, c = _metric("waves_split")
    assert c["workgroups"] == 2 and c["one_image_workgroups"] == [1] and c["one_image_workgroup_images"] == [r.n - 1]
    assert c["waves_that_agree"] == 11 and c["waves_that_disagree"] == 5 and c["most_images_in_a_wave"] == 2
    assert c["blocks_in_last_workgroup"] == 32


def test_straddle_has_a_spanning_workgroup_between_two_one_image_ones():
    r, c = _metric("straddle")
    assert c["workgroups"] == 3 and c["one_image_workgroups"] == [0, 2] and c["one_image_workgroup_images"] == [0, 1]
    assert c["waves_that_agree"] == 16 and c["waves_that_disagree"] == 0
    assert c["waves_that_agree_on_another_image_than_img_last"] == 8


def test_lanes_disagree_in_every_wave_that_holds_blocks():
    r, c = _metric("lanes_disagree")
    assert c["one_image_workgroups"] == [] and c["waves_with_blocks"] == 71 and c["waves_that_disagree"] == 71
    assert c["most_images_in_a_wave"] == 6 and c["last_wave_with_blocks"] == (2, 44)


def test_image_per_lane_has_64_images_a_wave_in_two_workgroups():
    r, c = _metric("image_per_lane")
    assert r.rows * r.cols == 1 and c["workgroups"] == 2 and c["one_image_workgroups"] == []
    assert c["most_images_in_a_wave"] == 64 and c["waves_that_disagree"] == 18
    assert K.image_shape(K.BY_NAME["metric_dxt1_rgba8"], r) == (3, 2)


def test_the_padded_regimes_are_the_ones_with_waves_that_span_images():
    assert {r.name for r in K.METRIC_REGIMES if r.padded} == {"waves_agree", "waves_split", "lanes_disagree"}
    for F in (K.BY_NAME["metric_bc7_rgb888"], K.BY_NAME["metric_eac16_signed_rg11_rgb16"]):
        for r in K.regimes(F):
            L = K.layout(F, r)
            px = F.comps * F.sample_bytes
            assert L.h == 4 * r.rows - 1 and L.w == 4 * r.cols - 2
            if r.padded:
                assert (L.gh + 3) // 4 > r.rows and (L.gw + 3) // 4 > r.cols and L.stride > L.w * px
                assert L.pixel_image_stride > L.h * L.stride
                assert L.blocks_image_stride > ((L.gh + 3) // 4) * ((L.gw + 3) // 4) * K.block_bytes(F)
                assert (L.pixel_lead, L.blocks_lead) == (F.sample_bytes, 1)
                assert F.sample_bytes == 1 or (L.stride % 2 == 0 and L.pixel_image_stride % 2 == 0)


# ---- the decode regimes: 256 blocks a workgroup

def test_the_decode_regimes():
    blocks = {name: (r.rows * r.cols, r.n) for name, r in DECODE.items()}
    assert blocks["one_short"] == (255, 1) and blocks["exact"] == (256, 1) and blocks["one_over"] == (257, 1)
    assert blocks["image_per_workgroup"] == (256, 3)
    img, have = K.walk(15, 300, K.DECODE_BLOCKS_PER_WORKGROUP)  # lanes_disagree
    assert (DECODE["lanes_disagree"].rows * DECODE["lanes_disagree"].cols, DECODE["lanes_disagree"].n) == (15, 300)
    assert img.shape[0] == 18 and max(len(set(w[h].tolist())) for w, h in zip(img.reshape(-1, 64), have.reshape(-1, 64)) if h.any()) == 6
    img, have = K.walk(1, 1100, K.DECODE_BLOCKS_PER_WORKGROUP)  # image_per_lane
    assert blocks["image_per_lane"] == (1, 1100) and img.shape[0] == 5 and int(have[-1].sum()) == 76


def test_the_pvrtc_shapes_reach_both_forms():
    p2, p4 = K.BY_NAME["metric_pvrtc2_rgba8"], K.BY_NAME["metric_pvrtc4_rgba8"]
    assert [(s, n) for s, n, _ in K.PVRTC_SHAPES] == [(8, 300), (64, 5), (128, 3), (256, 3)]
    assert [K.pvrtc_takes_tiles(p2, s) for s, _, _ in K.PVRTC_SHAPES] == [False, False, False, True]
    assert [K.pvrtc_takes_tiles(p4, s) for s, _, _ in K.PVRTC_SHAPES] == [False, False, True, True]
    assert K.pvrtc_grid(p2, 128) == (32, 16)  # 512 blocks in the raster form: a metric workgroup spans two images
    c = K.classify(512, 3)
    assert c["workgroups"] == 2 and c["one_image_workgroups"] == [1] and c["waves_that_agree"] == 16
    c = K.classify(2, 300)  # 8^2 at 2 bpp: 32 images a wave
    assert c["most_images_in_a_wave"] == 32 and c["one_image_workgroups"] == []


# ---- the definitions

@pytest.mark.parametrize("F", K.METRIC_FAMILIES, ids=[F.name for F in K.METRIC_FAMILIES])
def test_metric_definition_at_the_smallest_regime(F):
    """The shared route (one decode of the batch, every image clipped out of it) against the oracle module's own call on the
    image alone, at the first, the second and the last image; the extremes reach the top of the range."""
    regime = K.regimes(F)[0] if K.is_pvrtc(F) else METRIC["lanes_disagree"]
    sse, mx = K.want_metric(F, regime)
    assert sse.shape == (regime.n, 4) and mx.shape == (regime.n, 4)
    k = K.compared_channels(F)
    assert not sse[:, k:].any() and not mx[:, k:].any() and (sse[:, :k] > 0).all()
    for i in (0, 1, regime.n - 1):
        one_sse, one_mx = K.want_metric_as_the_oracle_measures(F, regime, i)
        assert sse[i].tolist() == one_sse.tolist() and mx[i].tolist() == one_mx.tolist(), (F.name, i)
    top = {"rgba8": 255, "u16": 65535, "s16": 65535, "half": 0x7BFF}[K.DEFINITIONS[F.definition][3]]
    assert mx[:, :k].max() >= top - top // 32, (F.name, mx.max())


@pytest.mark.parametrize("F", K.DECODE_FAMILIES, ids=[F.name for F in K.DECODE_FAMILIES])
def test_decode_definition_at_the_smallest_regime(F):
    regime = K.regimes(F)[0] if K.is_pvrtc(F) else DECODE["lanes_disagree"]
    L = K.layout(F, regime)
    rows = K.want_rows(F, regime)
    assert rows.shape == (regime.n, L.h, L.w * F.pixel_bytes)
    stream = K.blocks(F.definition, regime.rows, regime.cols, regime.n)
    for i in (0, 1, regime.n - 1):
        one = np.ascontiguousarray(K.oracle_decode(F.definition, stream[i].tobytes(), L.h, L.w)).reshape(L.h, -1).view(np.uint8)
        assert (rows[i] == one).all(), (F.name, i)
    start, want = K.decode_output(F, regime)
    assert start.shape == want.shape and (start == K.CANARY).all() and (want[-K.TAIL:] == K.CANARY).all()
    assert K.image_of_byte(F, regime, 0) == 0 and K.image_of_byte(F, regime, want.size - 1) == regime.n - 1


def test_buffers_hold_the_images_where_the_layout_says():
    F, regime = K.BY_NAME["metric_bc5_rgb888"], METRIC["waves_split"]
    L = K.layout(F, regime)
    src, blk = K.source_buffer(F, regime), K.blocks_buffer(F, regime)
    i = regime.n - 1
    at = L.pixel_lead + i * L.pixel_image_stride + (L.h - 1) * L.stride
    assert src[at:at + L.w * 3].tobytes() == K.source(F, regime)[i, -1].tobytes() and src.size == at + L.stride
    grid_cols = (L.gw + 3) // 4
    at = L.blocks_lead + i * L.blocks_image_stride + ((regime.rows - 1) * grid_cols + regime.cols - 1) * 16
    assert blk[at:at + 16].tobytes() == K.blocks("bc5", regime.rows, regime.cols, regime.n)[i, -16:].tobytes()


# ---- more than 2^31 - 1 blocks in one call

@pytest.fixture(scope="module")
def pieces(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("walk_plan")), "decode_plan_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, "-o", exe,
                           os.path.join(HERE, "host_emul", "decode_plan_driver.cc")])

    def run(height, block_cols, n_images):
        lines = subprocess.check_output([exe] + [str(v) for v in (height, block_cols, n_images, 0, 0)]).decode().split("\n")
        assert lines[-2] == "rc 0"
        return [tuple(map(int, l.split())) for l in lines[:-2]]
    return run


def test_the_strip_is_cut_into_two_launches_out_of_step_with_its_period(pieces):
    assert K.STRIP_BLOCKS_PER_IMAGE == 64512 and K.STRIP_H == 4095 and K.STRIP_COLS == 63
    got = pieces(K.STRIP_H, K.STRIP_COLS, K.STRIP_IMAGES)
    assert got == [(0, K.STRIP_FIRST_LAUNCH_IMAGES, 0, K.STRIP_H),
                   (K.STRIP_FIRST_LAUNCH_IMAGES, K.STRIP_IMAGES - K.STRIP_FIRST_LAUNCH_IMAGES, 0, K.STRIP_H)]
    assert len(got) >= 2 and got[1][0] % K.STRIP_PERIOD != 0
    assert K.STRIP_FIRST_LAUNCH_IMAGES == 33288 and K.STRIP_IMAGES * K.STRIP_BLOCKS_PER_IMAGE > 2 ** 31 - 1
    # the first launch ends less than one image below the top of fastdiv's domain
    assert K.STRIP_FIRST_LAUNCH_IMAGES * K.STRIP_BLOCKS_PER_IMAGE - 1 >= 2 ** 31 - 1 - K.STRIP_BLOCKS_PER_IMAGE
    # what the 16-bit and BC6H entry points refuse: more than 2^31 pixels in one image
    assert K.STRIP_H * K.STRIP_W <= 2 ** 31


@pytest.mark.parametrize("name", K.STRIP_METRICS)
def test_the_strip_records_add_up_to_the_oracles_metric_of_a_whole_image(name):
    F = K.BY_NAME[name]
    table = K.strip_record_table(F)
    for i in (1, K.STRIP_FIRST_LAUNCH_IMAGES):
        sse, mx = K.strip_image_as_the_oracle_measures(F, i)
        got_sse, got_mx = K.strip_record(F, i)
        assert got_sse.tolist() == sse.tolist() and got_mx.tolist() == mx.tolist(), (name, i)
        row = table[i % K.STRIP_PERIOD]
        assert row[:32].view("<u8").tolist() == sse.tolist() and row[32:].view("<u4").tolist() == mx.tolist()
    assert len({table[r].tobytes() for r in range(K.STRIP_PERIOD)}) == K.STRIP_PERIOD  # every residue tells itself apart


@pytest.mark.parametrize("name", K.STRIP_DECODERS)
def test_the_strip_decodes_to_a_period_with_rows_that_differ(name):
    F = K.BY_NAME[name]
    rows = K.strip_period_decoded_rows(F)
    assert rows.shape == (4 * K.STRIP_PERIOD, K.STRIP_W * F.pixel_bytes + K.STRIP_ROW_PADDING)
    assert (rows[:, K.STRIP_W * F.pixel_bytes:] == K.CANARY).all()
    assert len({rows[4 * p:4 * p + 4].tobytes() for p in range(K.STRIP_PERIOD)}) == K.STRIP_PERIOD


def test_the_fastdiv_probe_covers_the_walk_tables_grids():
    import wrapper_cases as W
    d = set(W.fastdiv_divisors())
    assert K.fastdiv_grids() <= d
    assert {64512, 33288 * 64512, 63, 1023, 1025, 1536, 3072, 15, 4500, 1100, 96, 192, 255, 257} <= d
