"""CPU tier of the mip filters (include/ic_amd.h, "mip filters"; ICAMD_MIP_FILTER_SRGB / ICAMD_MIP_FILTER_ALPHA_WEIGHTED):
* the numpy restatement (tests/mip_filter_oracle.py) against literal per-pixel loops, filter 0 against tests/mips_oracle.py;
* the sRGB table: regenerating csrc/srgb_table.inc gives no diff, its SHA-256, monotony, inv(T[s]) == s;
* the filter math of csrc/mip_filter.h compiled for the host (tests/host_emul/mip_filter_emul.cc) against that oracle;
* every refusal of the filtered entry points, answered before a device is needed, and a loud error without a GPU;
* the eleven filtered kernels compile for gfx950 with zero scratch and the planned LDS size."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import bc45_oracle as B
import ic_testlib as T
import mip_filter_oracle as F
import mips_oracle as M

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(T.ROOT, "image-compression_amd", "csrc")
OK, FALSE, ERR_NO_DEVICE, ERR_ARG = 0, 1, -1, -4
FILTERS_BY_COMPS = {3: (0, 1), 4: (0, 1, 2, 3)}


@pytest.fixture(scope="module")
def pkg():
    import ic_amd_loader
    return ic_amd_loader.load_package()


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("mip_filter") / "libmip_filter_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DICAMD_HOST_EMULATION", "-I" + CSRC, "-o", so,
                           os.path.join(HERE, "host_emul", "mip_filter_emul.cc")])
    L = ctypes.CDLL(so)
    L.mip_filter_emul_table.restype = None
    L.mip_filter_emul_table.argtypes = [T.vp]
    L.mip_filter_emul_inverse.restype = None
    L.mip_filter_emul_inverse.argtypes = [T.vp, T.u32, T.vp]
    L.mip_filter_emul_quotient.restype = None
    L.mip_filter_emul_quotient.argtypes = [T.vp, T.vp, T.u32, T.vp]
    L.mip_filter_emul_quads.restype = ctypes.c_int
    L.mip_filter_emul_quads.argtypes = [T.ci, T.ci, T.vp, T.u32, T.vp]
    yield L
    T.assert_no_emul_violations(L, "test_mip_filters_host")


# ---- the oracle

@pytest.mark.parametrize("h,w", [(1, 1), (1, 9), (9, 1), (2, 3), (3, 5), (5, 5), (7, 13), (13, 7), (17, 2), (33, 31)])
def test_numpy_filters_match_the_literal_rule(h, w):
    """The odd and thin shapes of tests/test_mips_host.py; filter 0 is mips_oracle.next_level."""
    for c in (3, 4):
        p = F.mixed_image(h, w, c, index=h * 100 + w) if (h + w) % 2 else \
            np.random.default_rng(h * 100 + w).integers(0, 256, (h, w, c), dtype=np.uint8)
        for f in FILTERS_BY_COMPS[c]:
            levels = F.pyramid(p, f)
            assert len(levels) == M.max_levels(h, w)
            for l in range(1, len(levels)):
                assert levels[l].shape[:2] == M.level_shape(h, w, l)
                assert np.array_equal(levels[l], F.next_level_literal(levels[l - 1], f)), (h, w, c, f, l)
        assert np.array_equal(F.next_level(p, 0), M.next_level(p))
    for c in (1, 2):
        p = np.random.default_rng(w).integers(0, 256, (h, w, c), dtype=np.uint8)
        assert np.array_equal(F.next_level(p, 0), M.next_level(p))


def test_named_properties_of_the_definition():
    flat = np.zeros((4, 4, 4), np.uint8)
    for s in range(256):
        flat[...] = s
        for f in (1, 2, 3):
            assert (F.next_level(flat, f) == s).all(), (s, f)
    cb = np.zeros((2, 2, 3), np.uint8)
    cb[0, 0] = cb[1, 1] = 255
    assert F.next_level(cb, 1).tolist() == [[[188, 188, 188]]] and F.next_level(cb, 0).tolist() == [[[127, 127, 127]]]
    q = np.array([[[255, 0, 0, 0], [255, 0, 0, 0]], [[255, 0, 0, 0], [0, 0, 255, 255]]], np.uint8)
    assert F.next_level(q, 2).tolist() == [[[0, 0, 255, 63]]] and F.next_level(q, 3).tolist() == [[[0, 0, 255, 63]]]
    q[1, 1, 3] = 0  # all transparent: the unweighted value of the same filter
    assert np.array_equal(F.next_level(q, 2), F.next_level(q, 0)) and np.array_equal(F.next_level(q, 3), F.next_level(q, 1))


def test_every_gpu_test_image_holds_the_three_alpha_cases():
    """A == 0, A == 1020 and 0 < A < 1020 occur among the level-1 quads of every image the GPU tier uses (F.GPU_TEST_IMAGES,
    the list F.gpu_image serves it from).  1 x 1 and 5 x 3 have one and two quads: they hold as many cases as quads, and the
    three cases together over their indices."""
    small = {}
    for h, w, index in sorted(set(F.GPU_TEST_IMAGES)):
        cases = F.alpha_cases(F.mixed_image(h, w, 4, index=index))
        quads = max(1, h >> 1) * max(1, w >> 1)
        if quads >= 3:
            assert all(cases), (h, w, index, cases)
        else:
            assert sum(1 for c in cases if c) == quads, (h, w, index, cases)
            small[(h, w)] = small.get((h, w), np.zeros(3, np.int64)) + np.array(cases)
    assert small and all((seen > 0).all() for seen in small.values()), small


# ---- the table

def _inc_values():
    text = open(os.path.join(CSRC, "srgb_table.inc")).read()
    return [int(v) for v in re.findall(r"\d+", re.sub(r"/\*.*?\*/", "", text, flags=re.S))]


def test_srgb_table_is_the_generated_one_and_is_pinned(tmp_path):
    sys.path.insert(0, os.path.join(T.ROOT, "scripts"))
    try:
        import gen_srgb_table as G
    finally:
        sys.path.pop(0)
    table, margin = G.build()
    assert G.render(table, G.sha256_of(table)) == open(os.path.join(CSRC, "srgb_table.inc")).read()  # regenerating: no diff
    assert margin > 1.6e-3
    values = _inc_values()
    assert values == table == [int(v) for v in F.TABLE] and len(values) == 256
    assert F.table_sha256(values).startswith(F.TABLE_SHA256_PREFIX)
    steps = np.diff(values)
    assert steps.min() == 19 and steps.max() == 583  # strictly increasing
    assert F.inv(np.array(values)).tolist() == list(range(256))


# ---- csrc/mip_filter.h on the host

def test_emulated_table_and_inverse(emul):
    t = np.zeros(256, np.uint16)
    emul.mip_filter_emul_table(t.ctypes.data)
    assert t.tolist() == F.TABLE.tolist()
    v = np.arange(65536, dtype=np.uint32)
    out = np.zeros(65536, np.uint8)
    emul.mip_filter_emul_inverse(v.ctypes.data, v.size, out.ctypes.data)
    assert np.array_equal(out, F.inv(v).astype(np.uint8))
    assert out[F.TABLE].tolist() == list(range(256))


def test_emulated_weighted_quotient(emul):
    """(n + (A >> 1)) // A for every A in 1..1020 at n = 0, A - 1, A, the largest numerator 65535 A, and random ones."""
    rng = np.random.default_rng(5)
    A = np.repeat(np.arange(1, 1021, dtype=np.uint32), 8)
    n = np.zeros(A.size, np.uint32)
    n[1::8] = A[1::8] - 1
    n[2::8] = A[2::8]
    n[3::8] = A[3::8] * 65535
    for k in range(4, 8):
        n[k::8] = (rng.integers(0, 65536, A[k::8].size) * A[k::8]).astype(np.uint32) + rng.integers(0, 1021, A[k::8].size) % A[k::8]
    n = np.minimum(n, A * 65535)
    out = np.zeros(A.size, np.uint32)
    emul.mip_filter_emul_quotient(n.ctypes.data, A.ctypes.data, A.size, out.ctypes.data)
    want = (n.astype(np.int64) + (A >> 1)) // A
    assert np.array_equal(out, want)


def _pack(p):
    p = np.asarray(p, np.uint32)
    v = p[..., 0] | p[..., 1] << 8 | p[..., 2] << 16
    return (v | p[..., 3] << 24) if p.shape[-1] == 4 else v


@pytest.mark.parametrize("comps,mip_filter", [(3, 0), (4, 0), (3, 1), (4, 1), (4, 2), (4, 3)])
def test_emulated_four_pixel_rule(emul, comps, mip_filter):
    rng = np.random.default_rng(10 * comps + mip_filter)
    n = 40000
    quads = rng.integers(0, 256, (n, 4, comps), dtype=np.uint8)
    if comps == 4:
        quads[:5000, :, 3] = 0                                     # A == 0
        quads[5000:10000, :, 3] = 0
        quads[np.arange(5000, 10000), rng.integers(0, 4, 5000), 3] = rng.integers(1, 256, 5000)  # a single a_i != 0
        quads[10000:15000, :, 3] = 255                             # all a_i = 255
        quads[15000:20000, :, :3] = rng.choice([0, 255], (5000, 4, 3))  # extreme colours under any alpha
    packed = np.ascontiguousarray(_pack(quads), np.uint32)
    if comps == 3:  # byte 3 of a 3-byte pixel is undefined on input: the result must not depend on it
        packed |= rng.integers(0, 256, packed.shape).astype(np.uint32) << 24
    out = np.zeros(n, np.uint32)
    assert emul.mip_filter_emul_quads(mip_filter, comps, packed.ctypes.data, n, out.ctypes.data) == 1
    want = F.filter_quads(quads[:, 0], quads[:, 1], quads[:, 2], quads[:, 3], mip_filter)
    mask = np.uint32(0xffffffff if comps == 4 else 0x00ffffff)
    assert np.array_equal(out & mask, _pack(want))
    assert emul.mip_filter_emul_quads(2, 3, packed.ctypes.data, 1, out.ctypes.data) == 0


# ---- refusals (argument checks come before any device work)

def _enc(lib, codec=T.DXT1, comps=4, swap=0, mip_filter=1, h=64, w=64, levels=7, src=16, dst=16):
    return lib.icamd_encode_mips_filtered_device(codec, 2, comps, swap, mip_filter, h, w, w * comps, levels, 1, 0, 0, src, dst,
                                                 None, 0, None)


def _pyr(lib, comps=4, mip_filter=1, h=8, w=8, levels=2, src=16, dst=16):
    return lib.icamd_mip_pyramid_filtered_device(comps, mip_filter, h, w, w * comps, levels, 1, 0, 0, src, dst, None)


def test_filtered_entry_points_refuse_before_a_device_is_needed(pkg):
    lib = pkg.lib()
    for f in (1, 2, 3):
        for codec in (B.BC4, B.BC5, T.PVRTC2, T.PVRTC4):
            assert _enc(lib, codec=codec, mip_filter=f) == ERR_ARG, (codec, f)
        for comps in (1, 2):
            assert _pyr(lib, comps=comps, mip_filter=f) == ERR_ARG
            assert _enc(lib, codec=T.DXT1, comps=comps, mip_filter=f) == ERR_ARG
    for f in (4, -1, 7, 256):
        assert _enc(lib, mip_filter=f) == ERR_ARG
        assert _pyr(lib, mip_filter=f) == ERR_ARG
    for f in (2, 3):  # ALPHA_WEIGHTED needs an alpha byte
        assert _enc(lib, codec=T.DXT1, comps=3, mip_filter=f) == ERR_ARG
        assert _enc(lib, codec=T.ETC1, comps=3, mip_filter=f) == ERR_ARG
        assert _pyr(lib, comps=3, mip_filter=f) == ERR_ARG
    assert b"ALPHA_WEIGHTED" in lib.icamd_last_error()
    # the rules of the unfiltered entry points still hold
    assert _enc(lib, codec=T.DXT5, comps=3) == ERR_ARG
    assert _enc(lib, levels=8) == ERR_ARG and _enc(lib, levels=0) == ERR_ARG
    assert _enc(lib, h=256, w=256, levels=9) == ERR_ARG  # needs a workspace, whatever the filter
    # null pointers / empty images: ICAMD_FALSE, as the old entry points
    for f in (0, 1, 3):
        assert _enc(lib, mip_filter=f, src=None) == FALSE and _enc(lib, mip_filter=f, dst=None) == FALSE
        assert _enc(lib, mip_filter=f, h=0) == FALSE
        assert _pyr(lib, mip_filter=f, src=None) == FALSE and _pyr(lib, mip_filter=f, w=0) == FALSE
    # the host form
    buf = np.zeros(64 * 64 * 4, np.uint8)
    out = np.zeros(1 << 16, np.uint8)
    cm = lib.icamd_compress_mips_filtered
    chain5 = M.chain_offsets(T.DXT5, 64, 64, 7)[-1]
    chain1 = M.chain_offsets(T.DXT1, 64, 64, 7)[-1]
    assert cm(T.PVRTC, 2, T.RGBA, 1, 64, 64, 0, 7, buf.ctypes.data, out.ctypes.data, chain5) == ERR_ARG
    assert cm(T.DXTC, 2, T.RGBA, 4, 64, 64, 0, 7, buf.ctypes.data, out.ctypes.data, chain5) == ERR_ARG
    assert cm(T.DXTC, 2, T.RGBA, -1, 64, 64, 0, 7, buf.ctypes.data, out.ctypes.data, chain5) == ERR_ARG
    assert cm(T.DXTC, 2, T.RGB, 2, 64, 64, 0, 7, buf.ctypes.data, out.ctypes.data, chain1) == ERR_ARG
    assert cm(T.ETC, 2, T.RGB, 3, 64, 64, 0, 7, buf.ctypes.data, out.ctypes.data, chain1) == ERR_ARG
    assert cm(T.ETC, 2, T.RGBA, 1, 64, 64, 0, 7, buf.ctypes.data, out.ctypes.data, chain1) == FALSE  # ETC takes kRGB only
    assert cm(T.DXTC, 2, T.RGBA, 3, 64, 64, 0, 7, buf.ctypes.data, out.ctypes.data, chain5 - 1) == FALSE
    assert cm(T.DXTC, 2, T.RGBA, 3, 64, 64, 0, 7, None, out.ctypes.data, chain5) == FALSE
    assert cm(T.DXTC, 2, T.RGBA, 3, 64, 64, 0, 8, buf.ctypes.data, out.ctypes.data, chain5) == ERR_ARG


def test_workspace_size_does_not_depend_on_the_filter_and_kernel_names(pkg):
    # one size query serves every filter: a chain that needs a workspace is refused without one and accepted (up to the
    # device check) with the unfiltered size, under every filter
    lib = pkg.lib()
    need = lib.icamd_mip_workspace_size(T.DXT1, 4, 256, 256, 9, 1)
    for f in (0, 1, 2, 3):
        rc = lib.icamd_encode_mips_filtered_device(T.DXT1, 2, 4, 0, f, 256, 256, 1024, 9, 1, 0, 0, 16, 16, 64, need - 1, None)
        assert rc == ERR_ARG
    names = set()
    for codec, comps, filters in [(T.DXT1, 3, (1,)), (T.DXT1, 4, (1, 2, 3)), (T.DXT5, 4, (1, 2, 3)), (pkg.MIP_PYRAMID, 3, (1,)),
                                  (pkg.MIP_PYRAMID, 4, (1, 2, 3))]:
        for f in filters:
            name = pkg.mip_kernel_name(codec, comps, f)
            assert name.startswith("icamd_fmip_") and name.endswith("_kernel"), (codec, comps, f, name)
            names.add(name)
    assert len(names) == 11
    assert pkg.mip_kernel_name(T.DXT1, 4, 0) == "icamd_mip_dxt1_rgba8_kernel"
    assert pkg.mip_kernel_name(B.BC4, 1, 0) == "icamd_mip_bc4_r8_kernel"
    assert pkg.mip_kernel_name(pkg.MIP_PYRAMID, 2, 0) == "icamd_mip_pyramid_rg8_kernel"
    assert pkg.mip_kernel_name(T.ETC1, 4, 3) == pkg.mip_kernel_name(pkg.MIP_PYRAMID, 4, 3)  # ETC1: pyramid + ETC1 kernels
    for codec, comps, f in [(B.BC4, 4, 1), (T.DXT1, 3, 2), (T.DXT5, 3, 1), (T.DXT1, 4, 4), (T.DXT1, 4, -1), (T.PVRTC2, 4, 0),
                            (pkg.MIP_PYRAMID, 2, 1), (T.ETC1, 2, 0)]:
        assert pkg.mip_kernel_name(codec, comps, f) == "", (codec, comps, f)
    assert (pkg.MIP_FILTER_BOX, pkg.MIP_FILTER_SRGB, pkg.MIP_FILTER_ALPHA_WEIGHTED) == (0, 1, 2)


def test_no_gpu_means_a_loud_error_not_a_cpu_result(pkg):
    if pkg.lib().icamd_device_count() > 0:
        pytest.skip("a HIP device is present: the GPU tier covers this path")
    lib = pkg.lib()
    for f in (0, 1, 2, 3):
        assert _enc(lib, mip_filter=f) == ERR_NO_DEVICE
        assert lib.icamd_last_error().decode()
        assert _pyr(lib, mip_filter=f) == ERR_NO_DEVICE
    buf = np.zeros(64 * 64 * 4, np.uint8)
    out = np.zeros(1 << 16, np.uint8)
    chain = M.chain_offsets(T.DXT5, 64, 64, 7)[-1]
    assert lib.icamd_compress_mips_filtered(T.DXTC, 2, T.RGBA, 3, 64, 64, 0, 7, buf.ctypes.data, out.ctypes.data, chain) == ERR_NO_DEVICE
    with pytest.raises(pkg.BackendError):
        pkg.compress_mips_host(T.DXTC, T.RGBA, buf, 64, 64, mip_filter=pkg.MIP_FILTER_SRGB)


# ---- build check: zero scratch, the planned LDS

def test_filtered_mip_kernels_use_no_scratch_and_the_planned_lds(tmp_path):
    if not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    out = os.path.join(str(tmp_path), "k.s")
    subprocess.check_call(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(T.ROOT, "include"),
                           "-I" + CSRC, "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "mip_filter_kernels.hip")],
                          stderr=subprocess.DEVNULL)
    text = open(out).read()
    metas = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", text, re.S):
        blk = m.group(0)
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        metas[name] = (int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)),
                       int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1)))
    assert not [n for n in metas if n.startswith("icamd_mip_")]  # the box kernels stay in mip_kernels.hip
    names = sorted(n for n in metas if n.startswith("icamd_fmip_"))
    assert len(names) == 11, sorted(metas)  # SRGB: DXT1 x 2, DXT5, pyramid x 2; ALPHA_WEIGHTED and both: DXT1, DXT5, pyramid
    # the box twin's plan (tests/test_mips_host.py): levels 1..7 of a 128 x 128 tile as pixel dwords, rounded up to the 16-byte
    # alignment of what follows it, + the DXT colour search's per-lane 64-byte stash; then the filter's tables:
    # T and M (256 16-bit entries each, 1 KiB) for SRGB, the reciprocals of A = 0..1023 (32-bit, 4 KiB) for ALPHA_WEIGHTED
    pyramid_lds = -(-5461 * 4 // 16) * 16
    for n in names:
        scratch, lds = metas[n]
        assert scratch == 0, "%s uses %d bytes of scratch" % (n, scratch)
        tables = (4096 if "_alpha_" in n else 0) + (1024 if "_srgb_" in n else 0)
        want = pyramid_lds + (256 * 64 if ("dxt1" in n or "dxt5" in n) else 0) + tables
        assert lds == want, (n, lds, want)
    # no inline assembly beyond the empty optimisation barrier of ic_device.h, and the tables are read from LDS
    assert "flat_load" not in text and "ds_read_u16" in text
