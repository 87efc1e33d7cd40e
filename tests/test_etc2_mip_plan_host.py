"""CPU tier of the ETC2-family mip chains (image-compression_amd/csrc/etc2_mip_plan.h, icamd_encode_etc2_mips_device): the plan of a
call -- the pyramid passes, the level table of the one encode launch, its grid -- is host-only arithmetic, and every argument check
of the entry points returns before a device is needed, so both are stated here without a GPU.

tests/host_emul/etc2_mip_plan_driver.cc, built with g++ against the header alone, prints every field of every plan over a grid of
codecs, layouts, filters, shapes (1 x 1, 1 x 37, 37 x 21, 516 x 8, 8 x 516, 4096^2, 16384 x 4, ...), level counts, image counts (0,
1, 3 with padded strides, 65 537) and both level orders, and locates every workgroup of grid.x with etc2_mip_locate -- the function
the kernels call -- to count how often each block of each level is encoded."""
import ctypes
import os
import subprocess

import pytest

import eac11_oracle as E11
import ic_testlib as T
import mips_oracle as M

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(T.ROOT, "image-compression_amd", "csrc")
REFUSED, NOTHING, LAUNCH = range(3)
SOURCE, WORKSPACE, OUTPUT = range(3)
OK, FALSE, ERR_NO_DEVICE, ERR_ARG = 0, 1, -1, -4
ETC2_RGBA8, ETC2_RGB8, ETC2_RGB8A1 = 16, 18, 21
R11, RG11 = E11.EAC_R11, E11.EAC_RG11
FAMILY = (ETC2_RGBA8, ETC2_RGB8, ETC2_RGB8A1, R11, RG11)
BLOCK_BYTES = {ETC2_RGBA8: 16, ETC2_RGB8: 8, ETC2_RGB8A1: 8, R11: 8, RG11: 16}
COMPONENTS = {ETC2_RGBA8: (4,), ETC2_RGB8A1: (4,), ETC2_RGB8: (3, 4), R11: (1, 2, 3, 4), RG11: (2, 3, 4)}
SRGB, ALPHA, NORMAL = 1, 2, 4
IN_KEYS = "codec comps filter modes h w levels n_images row_stride src_image_stride dst_image_stride order".split()
PLAN_KEYS = "form workspace pyramid_image_stride chain_bytes grid_x n_images th n_passes".split()
LEVEL_KEYS = ("k level pix_offset dst_offset row_stride h w block_rows block_cols log2_tile_cols force_gather tiles_per_row n_tiles "
              "first_wg").split()


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("etc2_mip_plan")), "etc2_mip_plan_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, "-I" + os.path.join(T.ROOT, "include"),
                           "-o", exe, os.path.join(HERE, "host_emul", "etc2_mip_plan_driver.cc")])
    out = []
    for line in subprocess.check_output([exe]).decode().splitlines():
        w = line.split()
        if w[0] == "#":
            out.append(dict(zip(IN_KEYS, map(int, w[1:])), passes=[], ref=[], table=[], y=[], cover=None))
        elif w[0] == "=":
            out[-1].update(zip(PLAN_KEYS, map(int, w[1:])))
        elif w[0] in "PR":
            out[-1]["passes" if w[0] == "P" else "ref"].append(list(map(int, w[1:])))
        elif w[0] == "L":
            out[-1]["table"].append(dict(zip(LEVEL_KEYS, map(int, w[1:]))))
        elif w[0] == "Y":
            out[-1]["y"] = [tuple(map(int, x.split("+"))) for x in w[1:]]
        else:
            assert w[0] == "C", line
            out[-1]["cover"] = tuple(map(int, w[1:]))
    return out


@pytest.fixture(scope="module")
def pkg():
    import ic_amd_loader
    return ic_amd_loader.load_package()


def test_the_header_needs_nothing_from_hip():
    text = open(os.path.join(CSRC, "etc2_mip_plan.h")).read()
    includes = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
    assert sorted(includes) == ['"codec_info.h"', '"mip_plan.h"', "<cstddef>", "<cstdint>"]
    for word in ("hipGetDevice", "getenv", "hipError_t", "hipStream_t", "std::vector", "std::atomic", "dim3", "malloc", "new "):
        assert word not in text, word


def test_the_grid_of_cases_reaches_every_form(cases):
    assert {c["form"] for c in cases} == {REFUSED, NOTHING, LAUNCH}
    shapes = {(c["h"], c["w"]) for c in cases}
    assert {(1, 1), (1, 37), (37, 21), (516, 8), (8, 516), (4096, 4096), (16384, 4)} <= shapes
    assert {c["n_images"] for c in cases} == {0, 1, 3, 65537} and {c["order"] for c in cases} == {0, 1}
    for c in cases:
        ok = c["codec"] in FAMILY and c["comps"] in COMPONENTS[c["codec"]] and 1 <= c["levels"] <= M.max_levels(c["h"], c["w"]) \
            and (c["modes"] == 0 or c["codec"] == ETC2_RGB8)
        assert c["form"] == (REFUSED if not ok else NOTHING if c["n_images"] == 0 else LAUNCH), c
        assert c["th"] == (1 if c["modes"] else 0) or not ok
        if c["form"] != LAUNCH:
            assert not c["passes"] and not c["table"]
    assert any(c["form"] == LAUNCH and c["cover"] is None for c in cases)  # (the shapes too large to count are planned all the same)


def test_level_offsets_are_the_prefix_sums_of_encoded_size(cases, pkg):
    for c in cases:
        if c["form"] != LAUNCH:
            continue
        sizes = [pkg.encoded_size(c["codec"], *M.level_shape(c["h"], c["w"], l)) for l in range(c["levels"])]
        offsets = [sum(sizes[:l]) for l in range(c["levels"] + 1)]
        assert c["chain_bytes"] == offsets[-1], c
        assert {L["level"]: L["dst_offset"] for L in c["table"]} == dict(enumerate(offsets[:-1])), c
        total, offs = pkg.etc2_mip_chain_size(c["codec"], c["h"], c["w"], c["levels"])
        assert (total, offs) == (offsets[-1], offsets), c


def test_workspace_is_the_pixel_pyramid_of_every_image(cases, pkg):
    for c in cases:
        if c["form"] == REFUSED:
            continue
        pyramid = sum(lh * lw * c["comps"] for lh, lw in (M.level_shape(c["h"], c["w"], l) for l in range(1, c["levels"])))
        assert c["pyramid_image_stride"] == pyramid and c["workspace"] == pyramid * c["n_images"], c
        assert (c["workspace"] == 0) == (c["levels"] == 1 or c["n_images"] == 0), c
        assert pkg.etc2_mip_workspace_size(c["codec"], c["comps"], c["h"], c["w"], c["levels"], c["n_images"]) == c["workspace"], c


def test_the_pyramid_passes_are_those_of_the_etc1_chain(cases):
    two_pass = 0
    for c in cases:
        if c["form"] != LAUNCH:
            continue
        assert c["n_passes"] == len(c["passes"]) == len(c["ref"]) and (c["n_passes"] == 0) == (c["levels"] == 1), c
        for p, r in zip(c["passes"], c["ref"]):
            if c["comps"] >= 3:  # ICAMD_ETC1 of the same geometry: field for field
                assert p == r, c
            else:  # ETC1 takes 3 or 4 components: the pixel pyramid's passes, which write to the output where these write to the workspace
                moved = [WORKSPACE if k in (3, 11) and v == OUTPUT else v for k, v in enumerate(r)]
                assert p[11] == WORKSPACE and r[11] == OUTPUT and p == moved, c
        two_pass += c["n_passes"] == 2
    assert two_pass


def test_levels_tile_grid_x_without_gap_or_overlap_in_the_stated_order(cases):
    for c in cases:
        if c["form"] != LAUNCH:
            continue
        order = [L["level"] for L in c["table"]]
        assert order == (list(range(c["levels"])) if c["order"] else list(range(c["levels"] - 1, -1, -1))), c
        at = 0
        for L in c["table"]:
            assert L["first_wg"] == at and L["n_tiles"] > 0, c
            at += L["n_tiles"]
        assert at == c["grid_x"] < 1 << 31, c


def _tile_shape(block_cols, row_stride):  # launch_tiled with max_log2_cols = 4: what icamd_encode_device uses for the family
    log2 = min(max(block_cols - 1, 0).bit_length(), 4)
    if row_stride * 1024 >= 1 << 32 or block_cols * 4096 >= 1 << 32:
        log2 = 8
    return log2, int(row_stride * 3 + 8192 >= 1 << 32)


def test_every_level_is_the_view_icamd_encode_device_would_get(cases):
    wide = 0
    for c in cases:
        if c["form"] != LAUNCH:
            continue
        offs = [0, 0]
        for l in range(1, c["levels"]):
            lh, lw = M.level_shape(c["h"], c["w"], l)
            offs.append(offs[-1] + lh * lw * c["comps"])
        for L in c["table"]:
            l = L["level"]
            lh, lw = M.level_shape(c["h"], c["w"], l)
            assert (L["h"], L["w"], L["block_rows"], L["block_cols"]) == (lh, lw, -(-lh // 4), -(-lw // 4)), c
            assert L["row_stride"] == (c["row_stride"] if l == 0 else lw * c["comps"] % (1 << 32)), c
            assert L["pix_offset"] == (0 if l == 0 else offs[l]), c
            log2, gather = _tile_shape(L["block_cols"], L["row_stride"])
            assert (L["log2_tile_cols"], L["force_gather"]) == (log2, gather), c
            cols, rows = 1 << log2, 256 >> log2
            assert L["tiles_per_row"] == -(-L["block_cols"] // cols) and L["n_tiles"] == L["tiles_per_row"] * -(-L["block_rows"] // rows), c
            wide += log2 == 8
    assert wide  # (rows of 4 MiB and more: 256 x 1 tiles)


def test_every_block_of_every_level_is_encoded_exactly_once(cases):
    counted = 0
    for c in cases:
        if c["form"] != LAUNCH or c["cover"] is None:
            continue
        blocks = sum(L["block_rows"] * L["block_cols"] for L in c["table"])
        assert c["cover"] == (blocks, blocks, 1), c
        counted += 1
    assert counted > 1000
    assert any(c["cover"] is not None and (c["h"], c["w"]) == (4096, 4096) for c in cases)


def test_the_python_restatement_of_the_lookup_agrees_on_small_shapes(cases):
    """The same count from the printed table alone: a linear search of first_wg, then row-major tiles."""
    for c in cases:
        if c["form"] != LAUNCH or c["grid_x"] > 64 or c["n_images"] != 1:
            continue
        hits = {}
        for wg in range(c["grid_x"]):
            L = [L for L in c["table"] if L["first_wg"] <= wg][-1]
            t = wg - L["first_wg"]
            tr, tc = divmod(t, L["tiles_per_row"])
            cols, rows = 1 << L["log2_tile_cols"], 256 >> L["log2_tile_cols"]
            for tid in range(256):
                bc, br = tc * cols + (tid & (cols - 1)), tr * rows + (tid >> L["log2_tile_cols"])
                if bc < L["block_cols"] and br < L["block_rows"]:
                    hits[(L["level"], br, bc)] = hits.get((L["level"], br, bc), 0) + 1
        want = {(L["level"], br, bc): 1 for L in c["table"] for br in range(L["block_rows"]) for bc in range(L["block_cols"])}
        assert hits == want, c


def test_images_go_into_grid_y_in_pieces_of_at_most_65535(cases):
    seen = set()
    for c in cases:
        if c["form"] != LAUNCH:
            continue
        at = 0
        for first, count in c["y"]:
            assert first == at and 0 < count <= 65535, c
            at += count
        assert at == c["n_images"] and len(c["y"]) == -(-c["n_images"] // 65535), c
        seen.add(len(c["y"]))
    assert seen == {1, 2}


# ---- the C ABI: every check below returns before a device is touched ----
DUMMY = ctypes.c_void_p(16)


def _call(lib, codec, comps, *, strategy=2, modes=0, swap=0, f=0, h=64, w=64, stride=None, levels=7, n=1, src_stride=0, dst_stride=0,
          src=DUMMY, dst=DUMMY, ws=DUMMY, ws_bytes=1 << 30):
    return lib.icamd_encode_etc2_mips_device(codec, strategy, modes, comps, swap, f, h, w, w * comps if stride is None else stride, levels, n,
                                             src_stride, dst_stride, src, dst, ws, ws_bytes, None)


def _filter_ok(codec, comps, f):
    if f == 0:
        return True
    if f == NORMAL:
        return codec == RG11 and comps == 2
    if f < 0 or f > 3 or codec in (R11, RG11):
        return False
    return comps == 4 or not f & ALPHA


def test_codec_component_swap_mode_and_filter_rules(pkg):
    lib = pkg.lib()
    accepted = OK if lib.icamd_device_count() else ERR_NO_DEVICE  # with a device an accepted call would run on the dummy pointers
    for codec in list(range(-1, 24)):
        for comps in range(0, 6):
            for f in range(-1, 9):
                for modes in (0, 1, 2):
                    for swap in (0, 1):
                        ok = codec in FAMILY and comps in COMPONENTS[codec] and not (swap and comps < 3) and _filter_ok(codec, comps, f) \
                            and (modes == 0 or (modes == 1 and codec == ETC2_RGB8))
                        if ok and accepted == OK:
                            continue
                        assert _call(lib, codec, comps, modes=modes, swap=swap, f=f) == (accepted if ok else ERR_ARG), (codec, comps, f, modes, swap)
                        # (n_images == 0 is ICAMD_OK only once the rules are met)
                        assert _call(lib, codec, comps, modes=modes, swap=swap, f=f, n=0) == (OK if ok else ERR_ARG), (codec, comps, f, modes, swap)
    assert _call(lib, T.ETC1, 3) == ERR_ARG  # ETC1 keeps its chain in icamd_encode_mips_device


def test_status_order_and_geometry(pkg):
    lib = pkg.lib()
    # null pointers and empty images come first, whatever else is wrong
    assert _call(lib, 99, 9, src=None) == FALSE and _call(lib, 99, 9, dst=None) == FALSE
    assert _call(lib, 99, 9, h=0) == FALSE and _call(lib, ETC2_RGB8, 3, w=0, levels=0) == FALSE
    # then the rules, then the geometry -- all before n_images == 0 is ICAMD_OK
    assert _call(lib, ETC2_RGB8, 5, levels=0, n=0) == ERR_ARG
    for levels in (0, 8, 33):
        assert _call(lib, ETC2_RGB8, 3, levels=levels, n=0) == ERR_ARG
    assert _call(lib, ETC2_RGB8, 3, levels=7, n=0) == OK
    assert _call(lib, ETC2_RGB8, 3, stride=64 * 3 - 1, n=0) == ERR_ARG
    assert _call(lib, R11, 1, stride=63, n=0) == ERR_ARG and _call(lib, R11, 1, stride=64, n=0) == OK
    chain = pkg.etc2_mip_chain_size(ETC2_RGB8, 64, 64, 7)[0]
    src_bytes = 63 * 200 + 64 * 3
    assert _call(lib, ETC2_RGB8, 3, stride=200, n=2, src_stride=src_bytes - 1, dst_stride=chain) == ERR_ARG
    assert _call(lib, ETC2_RGB8, 3, stride=200, n=2, src_stride=src_bytes, dst_stride=chain - 1) == ERR_ARG
    need = pkg.etc2_mip_workspace_size(ETC2_RGB8, 3, 64, 64, 7, 2)
    assert need == 2 * 3 * sum((64 >> l) ** 2 for l in range(1, 7))
    assert _call(lib, ETC2_RGB8, 3, n=2, src_stride=64 * 64 * 3, dst_stride=chain, ws_bytes=need - 1) == ERR_ARG
    assert _call(lib, ETC2_RGB8, 3, n=2, src_stride=64 * 64 * 3, dst_stride=chain, ws=None, ws_bytes=need) == ERR_ARG
    # a chain of level 0 alone needs no workspace; short image strides are refused before n_images == 0 returns only for n > 1
    assert pkg.etc2_mip_workspace_size(ETC2_RGB8, 3, 64, 64, 1, 5) == 0
    assert _call(lib, ETC2_RGB8, 3, levels=1, n=0, ws=None, ws_bytes=0) == OK
    if lib.icamd_device_count() == 0:
        assert _call(lib, ETC2_RGB8, 3, levels=1, ws=None, ws_bytes=0) == ERR_NO_DEVICE
        assert _call(lib, RG11, 2, f=NORMAL) == ERR_NO_DEVICE
        assert b"no HIP device" in lib.icamd_last_error()


def test_sizes_answer_zero_outside_the_family(pkg):
    lib = pkg.lib()
    for codec in range(-1, 24):
        total, offs = pkg.etc2_mip_chain_size(codec, 37, 21, 6)
        if codec in FAMILY:
            want = [0]
            for l in range(6):
                lh, lw = M.level_shape(37, 21, l)
                want.append(want[-1] + -(-lh // 4) * -(-lw // 4) * BLOCK_BYTES[codec])
            assert (total, offs) == (want[-1], want), codec
            assert pkg.etc2_mip_chain_size(codec, 37, 21, 7) == (0, None) and pkg.etc2_mip_chain_size(codec, 37, 21, 0) == (0, None)
            assert pkg.etc2_mip_chain_size(codec, 0, 21, 1) == (0, None)
        else:
            assert (total, offs) == (0, None), codec
        for comps in range(0, 6):
            size = lib.icamd_etc2_mip_workspace_size(codec, comps, 37, 21, 6, 3)
            ok = codec in FAMILY and comps in COMPONENTS[codec]
            assert size == (3 * comps * sum(lh * lw for lh, lw in (M.level_shape(37, 21, l) for l in range(1, 6))) if ok else 0), (codec, comps)
    assert lib.icamd_etc2_mip_workspace_size(ETC2_RGB8, 3, 37, 21, 7, 1) == 0


def test_kernel_names(pkg):
    per_level = {ETC2_RGBA8: "icamd_etc2_rgba8", ETC2_RGB8A1: "icamd_etc2_rgb8a1"}
    suffix = {0: "_split_h", 1: "_split_v", 2: "", 3: "_heuristic"}
    layout = {1: "r8", 2: "rg8", 3: "rgb888", 4: "rgba8"}
    names = set()
    for codec in range(-1, 24):
        for comps in range(0, 6):
            for strategy in (-1, 0, 1, 2, 3, 4):
                for modes in (0, 1, 2):
                    got = pkg.etc2_mip_kernel_name(codec, comps, strategy, modes)
                    ok = codec in FAMILY and comps in COMPONENTS[codec] and (modes == 0 or (modes == 1 and codec == ETC2_RGB8))
                    s = suffix.get(strategy, "")
                    if not ok:
                        want = ""
                    elif modes == 1:
                        want = "icamd_etc2_mip_th_%s_kernel" % layout[comps]
                    elif codec == ETC2_RGB8:
                        want = "icamd_etc2_mip_rgb8_%s%s_kernel" % (layout[comps], s)
                    elif codec in per_level:
                        want = per_level[codec].replace("icamd_etc2_", "icamd_etc2_mip_") + s + "_kernel"
                    else:
                        want = "icamd_etc2_mip_%s_%s_kernel" % ("r11" if codec == R11 else "rg11", layout[comps])
                    assert got == want, (codec, comps, strategy, modes)
                    names.add(got)
    assert len(names - {""}) == 8 + 2 + 4 + 4 + 4 + 3  # one chain form per per-level encode kernel of the family
    # the per-level twin of a chain kernel is the name without "mip_" (EAC: icamd_eac_...), which the existing entry points answer
    assert pkg.kernel_name(ETC2_RGB8, 3) == "icamd_etc2_rgb8_rgb888_kernel" and pkg.kernel_name(R11, 1) == "icamd_eac_r11_r8_kernel"


def test_the_old_mip_entry_points_still_refuse_the_family(pkg):
    lib = pkg.lib()
    for codec in FAMILY:
        assert pkg.mip_chain_size(codec, 64, 64, 3) == (0, None)
        assert pkg.mip_kernel_name(codec, 4) == ""
        for comps in range(1, 5):
            assert lib.icamd_mip_workspace_size(codec, comps, 64, 64, 3, 1) == 0
        assert lib.icamd_encode_mips_device(codec, 2, 4, 0, 8, 8, 32, 1, 1, 0, 0, DUMMY, DUMMY, None, 0, None) == ERR_ARG
        assert b"ETC2 has no fused mip chain: icamd_mip_pyramid_device, then icamd_encode_device per level" in lib.icamd_last_error()
        assert lib.icamd_encode_mips_filtered_device(codec, 2, 4, 0, 0, 8, 8, 32, 1, 1, 0, 0, DUMMY, DUMMY, None, 0, None) == ERR_ARG


def test_the_level_order_knob_takes_two_values(pkg):
    lib = pkg.lib()
    assert lib.icamd_etc2_mip_tune(2) == ERR_ARG and lib.icamd_etc2_mip_tune(-1) == ERR_ARG
    assert lib.icamd_etc2_mip_tune(0) == OK and lib.icamd_etc2_mip_tune(1) == OK  # (1, largest first, is the default: put back)
