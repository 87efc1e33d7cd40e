"""CPU tier of the half-float pixel pyramid (include/ic_amd.h icamd_mip_pyramid_f16_device; image-compression_amd/csrc/mip_f16.h).

Three statements of one filter are held together: the float64 restatement (mip_f16_oracle.average, the independent oracle: the
float64 sum of four halves is exact), the header's integer definition written out in numpy (average_integer), and the routine
the kernels run, compiled for the host with g++ (tests/host_emul/mip_f16_emul.cc).  The geometry -- cascade, odd sizes, sides of
1 -- is checked on small images, and the entry point's argument checks, which all return before a device is needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ic_testlib as T
import mip_f16_oracle as F
import mips_oracle as M

CSRC = os.path.join(T.ROOT, "image-compression_amd", "csrc")
EMUL_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_emul")
OK, FALSE, ERR_NO_DEVICE, ERR_ARG = 0, 1, -1, -4


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("mip_f16") / "libmip_f16_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-DICAMD_HOST_EMULATION",
                           "-I" + CSRC, "-I" + os.path.join(T.ROOT, "include"), "-o", so, os.path.join(EMUL_DIR, "mip_f16_emul.cc")])
    L = ctypes.CDLL(so)
    L.mip_f16_emul_avg.restype = None
    L.mip_f16_emul_avg.argtypes = [T.vp, ctypes.c_uint64, T.vp]
    L.mip_f16_emul_avg2.restype = None
    L.mip_f16_emul_avg2.argtypes = [T.vp, ctypes.c_uint64, T.vp]
    L.mip_f16_emul_next_level.restype = None
    L.mip_f16_emul_next_level.argtypes = [T.vp, T.u32, T.u32, T.u32, T.vp]
    return L


@pytest.fixture(scope="module")
def pkg():
    import ic_amd_loader
    return ic_amd_loader.load_package()


@pytest.fixture(scope="module")
def quads():
    """(n, 4) uint16: the stated quads, every permutation-free variant of them with the signs flipped, and 1.2 million random ones"""
    special = np.array([q[:4] for q in F.SPECIAL_QUADS], np.uint16)
    return np.concatenate([special, special ^ 0x8000, F.random_quads(1_200_000, seed=5)])


def emul_avg(emul, q):
    q = np.ascontiguousarray(q, np.uint16)
    out = np.empty(len(q), np.uint16)
    emul.mip_f16_emul_avg(q.ctypes.data, len(q), out.ctypes.data)
    return out


def test_the_stated_quads_give_the_stated_halves(emul):
    q = np.array([s[:4] for s in F.SPECIAL_QUADS], np.uint16)
    want = np.array([s[4] for s in F.SPECIAL_QUADS], np.uint16)
    for name, got in (("float64", F.average(*q.T)), ("integer", F.average_integer(*q.T)), ("kernel routine", emul_avg(emul, q))):
        assert got.tolist() == want.tolist(), name
    # the cases the definition names, one by one
    one = lambda *p: int(F.average(*[np.array([v], np.uint16) for v in p])[0])  # noqa: E731
    assert one(0x7E00, 0x7E00, 0x7E00, 0x7E00) == 0 and one(0xFFFF, 0x7C01, 0x7FFF, 0xFE00) == 0  # NaN -> 0
    assert one(*[0x7C00] * 4) == 0x7BFF and one(*[0xFC00] * 4) == 0xFBFF  # +-Inf -> +-65504
    assert one(0x3C00, 0x3C00, 0x3C01, 0x3C01) == 0x3C00 and one(0x3C01, 0x3C01, 0x3C02, 0x3C02) == 0x3C02  # ties to even
    assert one(0x1234, 0x9234, 0xABCD, 0x2BCD) == 0x0000  # +x, -x pairs: +0, never 0x8000


def test_integer_definition_and_kernel_routine_equal_the_float64_oracle(emul, quads):
    assert len(quads) >= 1_000_000
    want = F.average(*quads.T)
    assert not (want == 0x8000).any() and (want & 0x7FFF).max() <= 0x7BFF  # never -0, never an infinity or NaN
    integer = F.average_integer(*quads.T)
    bad = np.nonzero(integer != want)[0]
    assert bad.size == 0, (quads[bad[:4]].tolist(), integer[bad[:4]].tolist(), want[bad[:4]].tolist())
    got = emul_avg(emul, quads)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (quads[bad[:4]].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist())
    # the classes the grid must hold: subnormal results, results at the top, cancellations, exact ties
    s = F.fixed(quads[:, 0]) + F.fixed(quads[:, 1]) + F.fixed(quads[:, 2]) + F.fixed(quads[:, 3])
    assert ((want & 0x7C00) == 0).sum() > 1000 and (s == 0).sum() > 100 and ((want & 0x7FFF) >= 0x7800).sum() > 1000
    a = np.abs(s)
    n = np.floor(np.log2(np.maximum(a, 1).astype(np.float64))).astype(np.int64) + 1
    sh = np.maximum(2, n - 11)
    assert ((a & ((1 << sh) - 1)) == (1 << (sh - 1))).sum() > 1000  # ties


def test_the_packed_form_is_the_routine_on_each_half(emul, quads):
    q = quads[:200_000].astype(np.uint32)
    packed = np.ascontiguousarray(q[:100_000] | q[100_000:] << 16)
    out = np.empty(100_000, np.uint32)
    emul.mip_f16_emul_avg2(packed.ctypes.data, 100_000, out.ctypes.data)
    want = F.average(*quads[:100_000].T).astype(np.uint32) | F.average(*quads[100_000:200_000].T).astype(np.uint32) << 16
    assert (out == want).all()


def next_level_loops(p):
    """the geometry as plain loops, one pixel at a time"""
    h, w, c = p.shape
    nh, nw = max(1, h >> 1), max(1, w >> 1)
    out = np.zeros((nh, nw, c), np.uint16)
    for y in range(nh):
        for x in range(nw):
            ya, yb, xa, xb = 2 * y, min(2 * y + 1, h - 1), 2 * x, min(2 * x + 1, w - 1)
            out[y, x] = F.average(p[ya, xa], p[ya, xb], p[yb, xa], p[yb, xb])
    return out


@pytest.mark.parametrize("h,w", [(5, 3), (1, 7), (37, 21)])
@pytest.mark.parametrize("chans", [3, 4])
def test_geometry_cascade_odd_sizes_and_sides_of_one(emul, h, w, chans):
    img = F.image(h, w, chans, seed=h * 100 + w)
    levels = F.pyramid(img)
    assert len(levels) == M.max_levels(h, w) and levels[-1].shape == (1, 1, chans)
    for l in range(1, len(levels)):
        assert levels[l].shape == M.level_shape(h, w, l) + (chans,)
        assert (levels[l] == next_level_loops(levels[l - 1])).all(), l  # each level from the ROUNDED level above
        assert (levels[l] == F.next_level(levels[l - 1], F.average_integer)).all(), l
        above = np.ascontiguousarray(levels[l - 1])
        got = np.empty(levels[l].shape, np.uint16)
        emul.mip_f16_emul_next_level(above.ctypes.data, above.shape[0], above.shape[1], chans, got.ctypes.data)
        assert (got == levels[l]).all(), l
    total = sum(lh * lw * chans * 2 for lh, lw in (M.level_shape(h, w, l) for l in range(1, len(levels))))
    assert len(F.pyramid_bytes(img)) == total
    assert F.pyramid_bytes(img, 2) == np.ascontiguousarray(levels[1]).tobytes() and F.pyramid_bytes(img, 1) == b""


def test_the_image_generator_places_every_special_quad_off_the_block_grid():
    img = F.image(37, 21, 3, seed=1)
    placed = set()
    for y in range(36):
        for x in range(20):
            quad = (int(img[y, x, 0]), int(img[y, x + 1, 0]), int(img[y + 1, x, 0]), int(img[y + 1, x + 1, 0]))
            if quad in {q[:4] for q in F.SPECIAL_QUADS}:
                placed.add((quad, y % 2, x % 2))
    assert {q for q, _, _ in placed} == {q[:4] for q in F.SPECIAL_QUADS}
    assert {(a, b) for _, a, b in placed} == {(0, 0), (0, 1), (1, 0), (1, 1)}


# ---- the C ABI: every check below returns before a device is touched ----
DUMMY = ctypes.c_void_p(16)


def _call(lib, chans, *, h=64, w=64, stride=None, levels=7, n=1, src_stride=0, dst_stride=0, src=DUMMY, dst=DUMMY):
    return lib.icamd_mip_pyramid_f16_device(chans, h, w, w * chans * 2 if stride is None else stride, levels, n, src_stride, dst_stride,
                                            src, dst, None)


def test_statuses_of_the_entry_point(pkg):
    lib = pkg.lib()
    for chans in (-1, 0, 1, 2, 5):
        assert _call(lib, chans, src=None) == ERR_ARG
    assert _call(lib, 3, src=None) == FALSE and _call(lib, 4, dst=None) == FALSE and _call(lib, 3, h=0) == FALSE and _call(lib, 3, w=0) == FALSE
    for levels in (0, 8, 33):
        assert _call(lib, 3, levels=levels, n=0) == ERR_ARG
    assert _call(lib, 3, stride=64 * 6 - 2, n=0) == ERR_ARG and _call(lib, 4, stride=64 * 8 - 2, n=0) == ERR_ARG
    pyramid = 6 * sum((64 >> l) ** 2 for l in range(1, 7))
    src_bytes = 63 * 400 + 64 * 6
    assert _call(lib, 3, stride=400, n=2, src_stride=src_bytes - 2, dst_stride=pyramid) == ERR_ARG
    assert _call(lib, 3, stride=400, n=2, src_stride=src_bytes, dst_stride=pyramid - 2) == ERR_ARG
    assert _call(lib, 3, stride=400, n=0, src_stride=src_bytes, dst_stride=pyramid) == OK
    # samples are 2-byte aligned: odd pointers and strides are refused
    assert _call(lib, 3, src=ctypes.c_void_p(17), n=0) == ERR_ARG and _call(lib, 3, dst=ctypes.c_void_p(17), n=0) == ERR_ARG
    assert _call(lib, 3, stride=64 * 6 + 1, n=0) == ERR_ARG
    assert _call(lib, 3, n=0, src_stride=64 * 64 * 6 + 1, dst_stride=pyramid) == ERR_ARG
    assert _call(lib, 3, n=0, src_stride=64 * 64 * 6, dst_stride=pyramid + 1) == ERR_ARG
    assert _call(lib, 3, src=ctypes.c_void_p(18), dst=ctypes.c_void_p(22), stride=64 * 6 + 2, n=0) == OK  # no wider alignment is asked
    if lib.icamd_device_count() == 0:
        assert _call(lib, 3) == ERR_NO_DEVICE and _call(lib, 4, levels=1) == ERR_NO_DEVICE
        assert b"no HIP device" in lib.icamd_last_error()


def test_kernel_names(pkg):
    assert [pkg.mip_f16_kernel_name(c) for c in range(0, 6)] == ["", "", "", "icamd_mip_pyramid_rgb16f_kernel",
                                                                 "icamd_mip_pyramid_rgba16f_kernel", ""]
    # the 8-bit pyramid's list is as it was: these kernels are not rows of it
    assert pkg.mip_kernel_name(pkg.MIP_PYRAMID, 6) == "" and pkg.mip_kernel_name(pkg.MIP_PYRAMID, 8) == ""
