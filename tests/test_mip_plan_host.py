"""CPU tier of the mip-chain plan (image-compression_amd/csrc/mip_plan.h): which passes a mip call runs, where each reads and
writes, the workspace, the grid pieces of every launch and which (mode, components, filter) has a kernel is host-only arithmetic,
so it is pinned here, without a GPU.

tests/host_emul/mip_plan_driver.cc, built with g++ against the header alone, prints the kernel list, one image's chain and pyramid
offsets, and every field of every plan over
* the five codecs and the pixel pyramid x components 1..4 x filters 0..4,
* the shapes SHAPES x levels {1, 6, 7, 8, 12, 13, 14, full chain} where legal x {0, 1, 3, 65 535, 65 536, 70 000} images (with three
  images the rows are padded and the image strides wider than an image).
tests/golden/mip_plan.txt records them one line per label (mode / components / filter): in the clear, the number of passes of the
full chain of one image per shape (R where the combination is refused), and the SHA-256 (first 16 digits) of the driver's lines.
It was recorded in the first step of the move, with the arithmetic in the header verbatim: mip_plan's loop, encode_mips's and
mip_pyramid's running pointers and poff[] and the ETC1 walk as they stood in ic_capi.hip, the 65 535 loops as they stood in
mip_pass.h's launch_mip_kernel.  The one pass builder that replaced them must reproduce it byte for byte.  A mismatch prints the
driver's lines of that label; `python tests/test_mip_plan_host.py` prints the file anew.

Every plan is also checked against the independent Python restatement of the pass rule (_model_plan, _workspace_formula, which
tests/test_mips_host.py checks against the numpy pyramid tile by tile), and the properties below are stated on the parsed table."""
import hashlib
import os
import subprocess

import pytest

import bc45_oracle as B
import ic_testlib as T
import mips_oracle as M
from test_mips_host import _model_plan, _workspace_formula

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(T.ROOT, "image-compression_amd", "csrc")
GOLDEN = os.path.join(HERE, "golden", "mip_plan.txt")
REFUSED, NOTHING, LAUNCH = range(3)
SOURCE, WORKSPACE, OUTPUT = range(3)
PYRAMID = -1
ERR_NO_DEVICE, ERR_ARG = -1, -4
MODES = [T.DXT1, T.DXT5, T.ETC1, B.BC4, B.BC5, PYRAMID]
SHAPES = [(1, 1), (1, 7), (2, 3), (61, 59), (128, 128), (129, 127), (129, 1), (256, 256), (257, 255), (1, 8192), (1, 16384), (16385, 3),
          (4096, 4096), (16384, 16384), (65536, 65536), (8388481, 1), (8388480, 1), (1, 1 << 31)]
LEVELS = [1, 6, 7, 8, 12, 13, 14]
IMAGES = [0, 1, 3, 65535, 65536, 70000]
INPUT_KEYS = "mode comps filter h w levels n_images row_stride src_image_stride dst_image_stride".split()
PASS_KEYS = ("l0 n handoff in_base in_offset in_row_stride in_image_stride h w enc_mask pix_mask pix_base pix_offset pix_image_stride "
             "dst_image_stride").split()
ENCODE_KEYS = "h w in_base in_offset in_row_stride in_image_stride out_offset".split()


def run_driver(tmp_dir):
    exe = os.path.join(str(tmp_dir), "mip_plan_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, "-I" + os.path.join(T.ROOT, "include"),
                           "-o", exe, os.path.join(HERE, "host_emul", "mip_plan_driver.cc")])
    return subprocess.check_output([exe]).decode()


def _pieces(words):
    return [tuple(map(int, x.split("+"))) for x in words]


def parse(table):
    """(kernel rows [(name, mode, comps, filter)], {(mode, comps, filter): name or None}, chain sizes, pyramid sizes,
    [(label, inputs, plan)])"""
    rows, forms, chains, pyramids, cases = [], {}, [], [], []
    for line in table.splitlines():
        w = line.split()
        if w[0] == "K":
            rows.append((w[1],) + tuple(map(int, w[2:])))
        elif w[0] == "k":
            forms[tuple(map(int, w[1:4]))] = w[5] if w[4] == "1" else None
            assert (w[4] == "1") == (w[5] != "-")
        elif w[0] in "SQ":
            (chains if w[0] == "S" else pyramids).append((tuple(map(int, w[1:5])), int(w[6]), list(map(int, w[8:]))))
        elif w[0] == "#":
            cases.append((w[1], dict(zip(INPUT_KEYS, map(int, w[2:]))), None))
        elif w[0] == "=":
            plan = dict(zip("form workspace n_passes n_encodes".split(), map(int, w[1:])), passes=[], encodes=[])
            cases[-1] = cases[-1][:2] + (plan,)
        elif w[0] == "P":
            p = dict(zip(PASS_KEYS, map(int, w[1:16])))
            assert (w[16], w[25], w[34], w[38]) == ("L", "X", "G", "Y")
            p["level_off"], p["pix_off"] = list(map(int, w[17:25])), list(map(int, w[26:34]))
            p["grid_x"], p["tile_rows"], p["n_images"] = map(int, w[35:38])
            z = w.index("Z")
            p["y"], p["z"] = _pieces(w[39:z]), _pieces(w[z + 1:])
            cases[-1][2]["passes"].append(p)
        else:
            assert w[0] == "E", line
            cases[-1][2]["encodes"].append(dict(zip(ENCODE_KEYS, map(int, w[1:]))))
    return rows, forms, chains, pyramids, cases


def test_the_header_needs_nothing_from_hip():
    text = open(os.path.join(CSRC, "mip_plan.h")).read()
    includes = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
    assert sorted(includes) == ['"codec_info.h"', "<cstddef>", "<cstdint>"]
    info = open(os.path.join(CSRC, "codec_info.h")).read()
    assert sorted(l.split()[1] for l in info.splitlines() if l.startswith("#include")) == ['"ic_amd.h"', "<stdint.h>"]
    for word in ("hipGetDevice", "getenv", "hipError_t", "hipStream_t", "std::vector", "std::atomic", "dim3", "malloc", "new "):
        assert word not in text, word


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return run_driver(tmp_path_factory.mktemp("mip_plan"))


@pytest.fixture(scope="module")
def parsed(table):
    return parse(table)


@pytest.fixture(scope="module")
def cases(parsed):
    return parsed[4]


@pytest.fixture(scope="module")
def pkg():
    import ic_amd_loader
    return ic_amd_loader.load_package()


def golden_lines(table, cases):
    """{golden line: the driver's lines it stands for}, in the driver's order."""
    texts, clear = {}, {}
    head, _, body = table.partition("# ")
    for line in head.splitlines(True):
        texts.setdefault({"K": "kernels", "k": "kernels", "S": "sizes/chain", "Q": "sizes/pyramid"}[line[0]], []).append(line)
    for block in body.split("# "):
        texts.setdefault(block.split()[0], []).append("# " + block)
    for label, i, plan in cases:
        if i["n_images"] == 1 and i["levels"] == M.max_levels(i["h"], i["w"]):
            clear.setdefault(label, []).append("R" if plan["form"] == REFUSED else str(plan["n_passes"]))
    return {" ".join([label, "".join(clear.get(label, ["."])), hashlib.sha256("".join(blocks).encode()).hexdigest()[:16]]): "".join(blocks)
            for label, blocks in texts.items()}


def test_plan_table_is_the_recorded_one(table, cases):
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    got = golden_lines(table, cases)
    assert len(got) == len(want), "the grid itself changed: %d labels, recorded %d" % (len(got), len(want))
    for g, w in zip(got, want):
        assert g == w, "plans differ from the recorded ones (%s):\n%s" % (w, got[g][:20000])


def _legal_levels(h, w):
    top = M.max_levels(h, w)
    return [l for l in LEVELS if l < top] + [top]


def test_the_grid_is_the_one_the_table_claims(cases):
    want = [(mode, comps, f, h, w, levels, n) for mode in MODES for comps in (1, 2, 3, 4) for f in range(5) for h, w in SHAPES
            for levels in _legal_levels(h, w) for n in IMAGES]
    assert [tuple(i[k] for k in "mode comps filter h w levels n_images".split()) for _, i, _ in cases] == want
    for _, i, _ in cases:
        pad = i["n_images"] == 3
        assert i["row_stride"] == (i["w"] * i["comps"] + 5 * pad) % (1 << 32)
        out = M.chain_offsets(i["mode"], i["h"], i["w"], i["levels"])[-1] if i["mode"] != PYRAMID else \
            sum(lh * lw * i["comps"] for lh, lw in (M.level_shape(i["h"], i["w"], l) for l in range(1, i["levels"])))
        assert i["dst_image_stride"] == out + 24 * pad
        assert i["src_image_stride"] == (i["w"] * i["comps"] + 5 * pad) * i["h"] + 40 * pad


def test_sizes_and_offsets_match_the_oracle_and_the_package(parsed, pkg):
    _, _, chains, pyramids, _ = parsed
    assert len(chains) == 5 * sum(len(_legal_levels(h, w)) for h, w in SHAPES) and len(pyramids) == len(chains) // 5 * 4
    for (codec, h, w, levels), total, offsets in chains:
        assert offsets == M.chain_offsets(codec, h, w, levels) and total == offsets[-1], (codec, h, w, levels)
    for (comps, h, w, levels), total, offsets in pyramids:
        assert (total, offsets) == pkg.mip_pyramid_size(comps, h, w, levels), (comps, h, w, levels)


def test_every_plan_agrees_with_the_python_restatement(parsed):
    _, forms, _, _, cases = parsed
    launched = set()
    for _, i, plan in cases:
        mode, comps, h, w, levels, n = (i[k] for k in "mode comps h w levels n_images".split())
        key = (mode, comps, i["filter"], h, w, levels, n)
        kernel = forms[(PYRAMID if mode == T.ETC1 else mode, comps, i["filter"])] is not None and not (mode == T.ETC1 and comps < 3)
        nothing = n == 0 or (mode == PYRAMID and levels == 1)
        assert plan["form"] == (REFUSED if not kernel else NOTHING if nothing else LAUNCH), key
        pyramid_bytes = sum(lh * lw * comps for lh, lw in (M.level_shape(h, w, l) for l in range(1, levels)))
        # the workspace does not depend on the filter, and is stated whenever the chain exists
        assert plan["workspace"] == (0 if mode == PYRAMID else pyramid_bytes * n if mode == T.ETC1
                                     else _workspace_formula(h, w, levels, comps, n)), key
        if plan["form"] != LAUNCH:
            assert not plan["passes"] and not plan["encodes"], key
            continue
        launched.add(mode)
        fused = mode not in (PYRAMID, T.ETC1)
        model = _model_plan(h, w, levels, not fused) if fused or levels > 1 else []
        assert [(p["l0"], p["n"], p["h"], p["w"], bool(p["handoff"])) for p in plan["passes"]] == model, key
        assert plan["n_passes"] == len(model) <= 6 and plan["n_encodes"] == len(plan["encodes"]) == (levels if mode == T.ETC1 else 0), key
        for p in plan["passes"]:
            assert p["enc_mask"] == ((1 << p["n"]) - 1 if fused else 0), key
            assert p["pix_mask"] == (((1 << 6) if p["handoff"] else 0) if fused else ((1 << p["n"]) - 1) & ~1), key
            assert p["n_images"] == n and p["dst_image_stride"] == (i["dst_image_stride"] if fused else 0), key
    assert launched == set(MODES)


def _written(i, plan):
    """{level: (base, offset, row stride, image stride)} of the pixel levels the passes write"""
    out = {}
    for p in plan["passes"]:
        for j in range(1, 8):
            if p["pix_mask"] >> j & 1:
                level = p["l0"] + j
                assert level not in out
                # (tight rows; a 32-bit field as the source's row stride is: 1 x 2^31 with 4 components, whose own rows no caller
                # can state, wraps at level 1)
                out[level] = (p["pix_base"], p["pix_offset"] + p["pix_off"][j],
                              M.level_shape(i["h"], i["w"], level)[1] * i["comps"] % (1 << 32), p["pix_image_stride"])
    return out


def test_every_level_is_produced_once_and_read_where_it_was_written(cases):
    for _, i, plan in cases:
        if plan["form"] != LAUNCH:
            continue
        mode, levels = i["mode"], i["levels"]
        written = _written(i, plan)
        chain = M.chain_offsets(mode, i["h"], i["w"], levels) if mode != PYRAMID else None
        if mode in (PYRAMID, T.ETC1):
            assert sorted(written) == list(range(1, levels)), i
        if mode == PYRAMID:
            assert all(v[0] == OUTPUT and v[3] == i["dst_image_stride"] for v in written.values()), i
        elif mode == T.ETC1:
            assert [e["out_offset"] for e in plan["encodes"]] == chain[:-1], i
            first = plan["encodes"][0]
            assert (first["in_base"], first["in_offset"], first["in_row_stride"], first["in_image_stride"]) == \
                (SOURCE, 0, i["row_stride"], i["src_image_stride"]) and (first["h"], first["w"]) == (i["h"], i["w"]), i
            for l, e in enumerate(plan["encodes"][1:], 1):
                assert (e["h"], e["w"]) == M.level_shape(i["h"], i["w"], l), i
                assert (e["in_base"], e["in_offset"], e["in_row_stride"], e["in_image_stride"]) == written[l], (i, l)
        else:
            encoded = [(p["l0"] + j, p["level_off"][j]) for p in plan["passes"] for j in range(8) if p["enc_mask"] >> j & 1]
            assert encoded == list(zip(range(levels), chain)), i
        done = set()
        for k, p in enumerate(plan["passes"]):
            got = (p["in_base"], p["in_offset"], p["in_row_stride"], p["in_image_stride"])
            if k == 0:
                assert p["l0"] == 0 and got == (SOURCE, 0, i["row_stride"], i["src_image_stride"]), i
            else:  # ... what an EARLIER pass wrote
                assert p["l0"] in done and got == written[p["l0"]], (i, k)
            done |= {p["l0"] + j for j in range(1, 8) if p["pix_mask"] >> j & 1}


def test_workspace_regions_do_not_overlap_and_end_at_workspace_bytes(cases):
    for _, i, plan in cases:
        if plan["form"] != LAUNCH:
            continue
        groups = {}  # (offset, image stride) -> [(start, end) within an image]
        for p in plan["passes"]:
            if p["pix_base"] != WORKSPACE or not p["pix_mask"]:
                continue
            for j in range(1, 8):
                if p["pix_mask"] >> j & 1:
                    lh, lw = M.level_shape(i["h"], i["w"], p["l0"] + j)
                    groups.setdefault((p["pix_offset"], p["pix_image_stride"]), []).append((p["pix_off"][j], p["pix_off"][j] + lh * lw * i["comps"]))
        spans = []
        for (offset, stride), levels in sorted(groups.items()):
            levels.sort()
            assert all(a[1] <= b[0] for a, b in zip(levels, levels[1:])) and levels[-1][1] <= stride, i
            spans.append((offset, offset + stride * i["n_images"]))
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), i
        assert (spans[-1][1] if spans else 0) == plan["workspace"], i
        assert (i["mode"] == PYRAMID) <= (not spans), i


def test_no_pass_builds_more_levels_than_its_tiles_hold(cases):
    seen = set()
    for _, i, plan in cases:
        for p in plan["passes"]:
            single = p["h"] <= 128 and p["w"] <= 128
            assert p["enc_mask"] < (1 << 8 if single else 1 << 6) and p["pix_mask"] < (1 << 8 if single else 1 << 7), i
            assert not p["pix_mask"] & 1, i
            seen.add((single, max(p["enc_mask"], p["pix_mask"]).bit_length()))
    assert {(True, 8), (False, 6), (False, 7)} <= seen


def test_the_launches_tile_every_tile_row_and_image_once_within_the_grid_limits(cases):
    y_counts, z_counts = set(), set()
    for _, i, plan in cases:
        for p in plan["passes"]:
            assert p["grid_x"] == -(-p["w"] // 128) and p["tile_rows"] == -(-p["h"] // 128), i
            for pieces, total in ((p["y"], p["tile_rows"]), (p["z"], i["n_images"])):
                at = 0
                for first, count in pieces:
                    assert first == at and 0 < count <= 65535, i
                    at += count
                assert at == total and len(pieces) == -(-total // 65535), i
            y_counts.add(len(p["y"]))
            z_counts.add(len(p["z"]))
    assert {1, 2} <= y_counts and {1, 2} <= z_counts


def _enc(lib, codec, comps, f):  # (a workspace for ETC1's pyramid: its size is checked before the device is asked for)
    return lib.icamd_encode_mips_filtered_device(codec, 2, comps, 0, f, 64, 64, 64 * comps, 7, 1, 0, 0, 16, 16, 16, 1 << 20, None)


def _pyr(lib, comps, f):
    return lib.icamd_mip_pyramid_filtered_device(comps, f, 8, 8, 8 * comps, 2, 1, 0, 0, 16, 16, None)


def test_the_kernel_list_is_what_the_c_abi_answers(parsed, pkg):
    rows, forms, _, _, _ = parsed
    assert len(rows) == 29 == len({r[0] for r in rows}) == len({r[1:] for r in rows})
    assert [sum(r[0].startswith(p) for r in rows) for p in ("icamd_mip_", "icamd_fmip_", "icamd_nmip_")] == [14, 11, 4]
    assert {k: v for k, v in forms.items() if v} == {r[1:]: r[0] for r in rows}
    lib = pkg.lib()
    no_device = lib.icamd_device_count() == 0  # with a device an accepted call would run on the dummy pointers: refusals only
    for codec in MODES:
        for comps in (1, 2, 3, 4):
            for f in range(5):
                mode = PYRAMID if codec == T.ETC1 else codec
                name = forms[(mode, comps, f)] if not (codec == T.ETC1 and comps < 3) else None
                assert pkg.mip_kernel_name(pkg.MIP_PYRAMID if codec == PYRAMID else codec, comps, f) == (name or ""), (codec, comps, f)
                if name is None:
                    assert (_pyr(lib, comps, f) if codec == PYRAMID else _enc(lib, codec, comps, f)) == ERR_ARG, (codec, comps, f)
                elif no_device:
                    assert (_pyr(lib, comps, f) if codec == PYRAMID else _enc(lib, codec, comps, f)) == ERR_NO_DEVICE, (codec, comps, f)


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        text = run_driver(tmp)
    print("\n".join(golden_lines(text, parse(text)[4])))
