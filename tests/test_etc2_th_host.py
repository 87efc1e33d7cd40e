"""CPU tier for the T / H encoder of ETC2 RGB8 (include/ic_amd.h icamd_encode_etc2_device, ICAMD_ETC2_MODES_TH).

* The fixtures have the properties the definition gives them, asserted on the numpy definition (tests/etc2_th_oracle.py).
* The block math of image-compression_amd/csrc/etc2_th_block.h compiled for the host (tests/host_emul/etc2_th_emul.cc,
  -DICAMD_HOST_EMULATION), bit-exact against the definition: fixtures, random blocks, constructed corner blocks.
* The definition's output checked through etc2_colour_oracle alone (modes, decode, error).
* The C ABI's host-side surface of icamd_encode_etc2_device / icamd_etc2_kernel_name, and the Python keyword.

The fixture tests, test_output_of_the_definition_checked_independently and
test_packing_lands_in_the_intended_mode_with_the_intended_paints run no product code: they pin the DEFINITION (the numpy oracle
every other test here and in the GPU tier compares against), so they pass whatever the library does.  The host-twin, ABI,
keyword and build tests are the ones that fail without the feature."""
import ctypes
import functools
import importlib
import os
import subprocess

import numpy as np
import pytest

import etc2_colour_oracle as C
import etc2_th_oracle as H
import ic_testlib as T

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, "host_emul")
CSRC = os.path.join(T.ROOT, "image-compression_amd", "csrc")
pkg = importlib.import_module("image-compression_amd")
OK, FALSE, ERR_NO_DEVICE, ERR_ARG = 0, 1, -1, -4
COMBOS = {(p, k) for p in (H.PART_L, H.PART_C) for k in (H.KIND_T_AB, H.KIND_T_BA, H.KIND_H)}


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("etc2th") / "libetc2_th_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DICAMD_HOST_EMULATION", "-I" + CSRC,
                           "-I" + os.path.join(T.ROOT, "include"), "-o", so, os.path.join(EMUL_DIR, "etc2_th_emul.cc")])
    L = ctypes.CDLL(so)
    L.etc2th_emul_encode.restype = ctypes.c_int
    L.etc2th_emul_encode.argtypes = [T.ci, T.ci, T.ci, T.u32, T.u32, T.u32, T.u32, T.u32, T.vp, T.vp]
    L.etc2th_emul_search.restype = None
    L.etc2th_emul_search.argtypes = [T.u32, T.vp, T.vp]
    L.etc2th_emul_quantise.restype = T.u32
    L.etc2th_emul_quantise.argtypes = [T.u32, T.u32]
    yield L
    T.assert_no_emul_violations(L, "test_etc2_th_host")


def emul_encode(L, flat, h, w, comps, strategy=2, modes=1, gh=None, gw=None, stride=None):
    gh = h if gh is None else max(gh, h)
    gw = w if gw is None else max(gw, w)
    out = np.zeros(C.encoded_size(gh, gw), np.uint8)
    src = np.ascontiguousarray(flat, dtype=np.uint8).reshape(-1)
    assert L.etc2th_emul_encode(strategy, modes, comps, h, w, gh, gw, w * comps if stride is None else stride, src.ctypes.data,
                                out.ctypes.data)
    return out.tobytes()


def strip(tex):
    """[n, 4(y), 4(x), 3] blocks -> the 4 x 4n RGB image that holds them side by side."""
    tex = np.asarray(tex, np.uint8)
    return np.ascontiguousarray(tex.transpose(1, 0, 2, 3).reshape(4, 4 * tex.shape[0], 3))


@functools.lru_cache(maxsize=None)
def fixture_image(name):
    return {"edges0": lambda: H.edges(0), "edges6": lambda: H.edges(6), "equiluminant": H.equiluminant,
            "gradient": lambda: C.gradient(64, 64), "mixed": H.mixed}[name]()


@functools.lru_cache(maxsize=None)
def want(name, strategy=T.SMALLER_ERROR):
    """(bytes, choice) of the definition for a 64 x 64 fixture; computed once, never written to."""
    out, choice = H.oracle_encode(fixture_image(name), 64, 64, 3, 0, strategy, return_choice=True)
    choice.setflags(write=False)
    return out, choice


def psnr(img, blocks):
    dec = C.oracle_decode(blocks, 64, 64).reshape(64, 64, 3).astype(np.int64)
    return 10 * np.log10(255.0 ** 2 / ((img[..., :3].astype(np.int64) - dec) ** 2).mean())


# ---- the fixtures, on the definition

def test_edges_fixture_takes_every_partition_and_kind():
    out, choice = want("edges6")
    th = H.changed(choice)
    assert th.mean() >= 0.5
    assert {tuple(c) for c in choice[th][:, :2].tolist()} == COMBOS
    img = fixture_image("edges6")
    assert psnr(img, out) > psnr(img, C.oracle_encode(img, 64, 64, 3)) + 10  # (the issue's prototype: 17.0 -> 34.6 dB)


def test_equiluminant_fixture_is_h_from_partition_c_everywhere():
    out, choice = want("equiluminant")
    assert (choice[:, 0] == H.PART_C).all() and (choice[:, 1] == H.KIND_H).all()
    assert (C.modes(out) == C.H_MODE).all()
    tex = C.block_texels(fixture_image("equiluminant"), 64, 64, 64, 64)
    assert not H.cluster_colours(tex, H.partitions(tex)[H.PART_L])[2].any()  # partition L is dropped in every block


def test_gradient_fixture_is_unchanged():
    out, choice = want("gradient")
    assert not H.changed(choice).any()
    assert out == C.oracle_encode(fixture_image("gradient"), 64, 64, 3)


@pytest.mark.parametrize("strategy", C.STRATEGIES)
def test_mixed_fixture_holds_all_three_kinds_in_every_wave(strategy):
    kinds = H.wave_kinds(fixture_image("mixed"), strategy=strategy)
    assert len(kinds) == 4 and all(min(k) >= 4 for k in kinds), kinds


# ---- host twin against the definition

@pytest.mark.parametrize("name", ["edges0", "edges6", "equiluminant", "gradient", "mixed"])
def test_host_twin_on_the_fixtures(emul, name):
    img = fixture_image(name)
    for strategy in C.STRATEGIES + (7,):  # (out of range: kSmallerError)
        st = strategy if strategy < 4 else T.SMALLER_ERROR
        assert emul_encode(emul, img, 64, 64, 3, strategy) == want(name, st)[0], (name, strategy)
        assert emul_encode(emul, img, 64, 64, 3, strategy, modes=0) == C.oracle_encode(img, 64, 64, 3, 0, st)
    rgba = np.full((64, 64, 4), 77, np.uint8)
    rgba[..., :3] = img
    assert emul_encode(emul, rgba, 64, 64, 4) == want(name)[0]


def test_host_twin_padded_grid_and_row_padding(emul):
    img = H.edges(6, 61, 59)
    assert emul_encode(emul, img, 61, 59, 3, gh=64, gw=64) == H.oracle_encode(img, 61, 59, 3, gh=64, gw=64)
    flat = T.with_row_padding(img, 5)
    assert emul_encode(emul, flat, 61, 59, 3, stride=59 * 3 + 5) == H.oracle_encode(img, 61, 59, 3)


def random_blocks():
    """20 480 blocks: noise, two noisy colours under a random mask, two close colours, low-contrast noise."""
    g = np.random.Generator(np.random.PCG64(T.SEED0 + 9710))
    n = 5120
    noise = g.integers(0, 256, (n, 4, 4, 3))
    mask = g.integers(0, 2, (2 * n, 4, 4, 1)).astype(bool)
    c1, c2 = g.integers(0, 256, (2 * n, 1, 1, 3)), g.integers(0, 256, (2 * n, 1, 1, 3))
    c2[n:] = c1[n:] + g.integers(-20, 21, (n, 1, 1, 3))  # close colours: codes that collide, partitions that coincide
    two = np.where(mask, c1, c2) + g.integers(-4, 5, (2 * n, 4, 4, 3))
    low = g.integers(0, 256, (n, 1, 1, 3)) + g.integers(-9, 10, (n, 4, 4, 3))
    return np.clip(np.concatenate([noise, two, low]), 0, 255).astype(np.uint8)


def corner_blocks():
    """Constructed blocks: one-texel clusters (n = 1 and n = 15), clusters with equal codes, paints that clamp at 0 and 255,
    exact ties between paints and between candidates."""
    blocks = []

    def block(fill, **texels):
        b = np.empty((4, 4, 3), np.int64)
        b[:] = fill
        for key, colour in texels.items():
            b[int(key[1]), int(key[2])] = colour
        blocks.append(b)

    block((20, 30, 40), t00=(250, 240, 230))      # n_B = 1
    block((250, 240, 230), t33=(20, 30, 40))      # n_B = 15
    block((20, 30, 40), t12=(250, 30, 40))        # one texel apart in R only
    block((100, 100, 100), t00=(104, 104, 104))   # both clusters quantise to code 6: dropped
    block((100, 100, 100), t00=(108, 100, 100), t11=(108, 100, 100))  # codes differ in R alone
    block((0, 0, 0), t00=(255, 255, 255), t01=(255, 255, 255))        # paints clamp at both ends
    block((5, 5, 5), t00=(250, 250, 250), t01=(0, 0, 0), t10=(255, 255, 255))
    block((255, 255, 255), t30=(0, 0, 0))
    # texels midway between two paints: C1 = 0, C2 = 136 (codes 0 and 8); 136 +- d and the midpoints of neighbours
    for d in C.DIST:
        b = np.zeros((4, 4, 3), np.int64)
        b[:, 2:] = 136
        b[0, 2] = 136 + d
        b[1, 2] = 136 - d
        b[2, 2] = 136 + d // 2      # between C2 and C2 + d
        b[3, 2] = 136 - (d + 1) // 2
        b[0, 0] = 68                # between C1 and C2
        blocks.append(b)
    # two flat halves: T(a, b) and T(b, a) and H tie at several distances; the earliest must win
    for a, b2 in (((17, 17, 17), (238, 238, 238)), ((0, 0, 0), (255, 255, 255)), ((51, 102, 153), (153, 102, 51)),
                  ((34, 34, 34), (40, 34, 34)), ((3, 3, 3), (20, 20, 20))):
        for split in (1, 2, 3):
            blk = np.empty((4, 4, 3), np.int64)
            blk[:, :split], blk[:, split:] = a, b2
            blocks.append(blk)
            blocks.append(blk.transpose(1, 0, 2).copy())
    # equal luminance (partition L dropped) and equal ranges (the channel tie goes to R, then G)
    block((200, 50, 100), t00=(100, 100, 100), t22=(100, 100, 100))
    block((10, 10, 10), t00=(60, 60, 60))
    block((10, 10, 10), t00=(10, 60, 60))
    block((10, 10, 10), t00=(10, 10, 60), t01=(10, 60, 10))
    return np.clip(np.stack(blocks), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def block_cases():
    tex = np.concatenate([corner_blocks(), random_blocks()])
    img = strip(tex)
    n = tex.shape[0]
    out, choice = H.oracle_encode(img, 4, 4 * n, 3, return_choice=True)
    return tex, img, out, choice


def test_host_twin_on_random_and_corner_blocks(emul):
    tex, img, out, choice = block_cases()
    n = tex.shape[0]
    assert n >= 20000
    assert (C.block_texels(img, 4, 4 * n, 4, 4 * n) == tex).all()
    th = H.changed(choice)
    assert 0.2 < th.mean() < 0.98  # both outcomes in numbers
    got = emul_encode(emul, img, 4, 4 * n, 3)
    bad = np.flatnonzero((np.frombuffer(got, np.uint8).reshape(-1, 8) != np.frombuffer(out, np.uint8).reshape(-1, 8)).any(axis=1))
    assert bad.size == 0, (bad[:8], choice[bad[:8]])


def test_search_key_is_the_definitions_error_and_order(emul):
    tex, _, _, _ = block_cases()
    n = tex.shape[0]
    _, err, choice = H.search(tex)
    keys = np.zeros(n, np.uint32)
    flat = np.ascontiguousarray(tex.reshape(n, 48))
    emul.etc2th_emul_search(n, flat.ctypes.data, keys.ctypes.data)
    none = err == H.NO_ERROR
    assert none.any() and (keys[none] == 0xffffffff).all()
    order = 24 * choice[:, 0] + 8 * choice[:, 1] + choice[:, 2]
    assert (keys[~none].astype(np.int64) == (err[~none] << 6 | order[~none])).all()


def test_cluster_code_division(emul):
    for n in range(1, 16):
        for s in range(0, 255 * n + 1, 7):
            assert emul.etc2th_emul_quantise(s, n) == (30 * s + 255 * n) // (510 * n)
        assert emul.etc2th_emul_quantise(255 * n, n) == 15


# ---- the definition's output, through etc2_colour_oracle alone

def test_output_of_the_definition_checked_independently():
    tex, img, out, choice = block_cases()
    n = tex.shape[0]
    base = np.frombuffer(C.oracle_encode(img, 4, 4 * n, 3), np.uint8).reshape(-1, 8)
    words = np.frombuffer(out, np.uint8).reshape(-1, 8)
    th = H.changed(choice)
    assert ((words != base).any(axis=1) == th).all()       # unchanged blocks are W byte for byte
    m = C.modes(words[th])
    assert (m == np.where(choice[th][:, 1] == H.KIND_H, C.H_MODE, C.T_MODE)).all()
    err_base, err_out = C.sse(tex, C.decode_blocks(base)), C.sse(tex, C.decode_blocks(words))
    assert (err_out[th] < err_base[th]).all() and (err_out[~th] == err_base[~th]).all()
    _, claimed, _ = H.search(tex)
    assert (err_out[th] == claimed[th]).all()              # the decoder renders what the search counted
    assert (claimed[~th] >= err_base[~th]).all()


def _paints_of(kind, a, b, di):
    out = np.zeros((a.shape[0], 4, 3), np.int64)
    for d in range(8):
        out[di == d] = H.paints(kind, a[di == d], b[di == d], d)
    return out


def test_packing_lands_in_the_intended_mode_with_the_intended_paints():
    g = np.random.Generator(np.random.PCG64(T.SEED0 + 9720))
    n = 20000
    a, b = g.integers(0, 16, (n, 3)), g.integers(0, 16, (n, 3))
    b[(a == b).all(axis=1), 0] ^= 1
    di, k = g.integers(0, 8, n), g.integers(0, 4, (n, 4, 4))
    rows = np.arange(n)[:, None, None]
    t = H.pack_t(a, b, di, k)
    assert (C.modes(t) == C.T_MODE).all()
    assert (C.decode_blocks(t) == _paints_of(H.KIND_T_AB, a, b, di)[rows, k]).all()
    h = H.pack_h(a, b, di, k)
    assert (C.modes(h) == C.H_MODE).all()
    assert (C.decode_blocks(h) == _paints_of(H.KIND_H, a, b, di)[rows, k]).all()


# ---- the C ABI's host-side surface (every check below returns before the GPU is touched)

def _call(lib, codec=18, strategy=2, modes=1, comps=3, swap=0, h=8, w=8, gh=8, gw=8, stride=None, n=1, src=16, dst=16):
    stride = w * comps if stride is None else stride
    return lib.icamd_encode_etc2_device(codec, strategy, modes, comps, swap, h, w, gh, gw, stride, n, 0, 0,
                                        ctypes.c_void_p(src) if src else None, ctypes.c_void_p(dst) if dst else None, None)


def test_argument_errors():
    lib = pkg.lib()  # (the pointers are never dereferenced: the arguments are refused first)
    for codec in list(range(-1, 18)) + list(range(19, 24)):
        assert _call(lib, codec=codec, comps=4) == ERR_ARG, codec
    for modes in (-1, 2):
        assert _call(lib, modes=modes) == ERR_ARG, modes
    for comps in (1, 2, 5):
        for modes in (0, 1):
            assert _call(lib, comps=comps, modes=modes) == ERR_ARG, comps
    for comps in (3, 4):
        for modes in (0, 1):
            assert _call(lib, comps=comps, modes=modes, stride=8 * comps - 1) == ERR_ARG
    for modes in (0, 1):
        assert _call(lib, modes=modes, src=0) == FALSE and _call(lib, modes=modes, dst=0) == FALSE
        assert _call(lib, modes=modes, h=0) == FALSE and _call(lib, modes=modes, w=0) == FALSE
        assert _call(lib, modes=modes, n=0) == OK
        assert _call(lib, modes=modes, n=0, stride=23) == OK  # an empty batch comes before the stride, as in icamd_encode_device
        assert lib.icamd_encode_device(18, 2, 3, 0, 8, 8, 8, 8, 23, 0, 0, 0, ctypes.c_void_p(16), ctypes.c_void_p(16), None) == OK
        assert _call(lib, modes=modes, n=0, comps=5) == ERR_ARG and _call(lib, modes=modes, n=0, codec=16, comps=4) == ERR_ARG


def test_valid_arguments_fail_loudly_without_a_device():
    if pkg.lib().icamd_device_count() > 0:
        pytest.skip("a device is present: the GPU tier runs this call")
    for modes in (0, 1):
        assert _call(pkg.lib(), modes=modes) == ERR_NO_DEVICE


def test_kernel_names_and_constants():
    assert (pkg.ETC2_MODES_DEFAULT, pkg.ETC2_MODES_TH) == (0, 1) == (H.MODES_DEFAULT, H.MODES_TH)
    assert pkg.etc2_kernel_name(18, 3, 1) == "icamd_etc2_th_rgb888_kernel"
    assert pkg.etc2_kernel_name(18, 4, 1) == "icamd_etc2_th_rgba8_kernel"
    for comps in (3, 4):
        assert pkg.etc2_kernel_name(18, comps, 0) == pkg.kernel_name(18, comps) != ""
    for codec, comps, modes in ((18, 2, 1), (18, 5, 1), (18, 3, 2), (18, 3, -1), (16, 4, 1), (21, 4, 1), (2, 3, 1), (17, 3, 1)):
        assert pkg.etc2_kernel_name(codec, comps, modes) == "", (codec, comps, modes)
    assert pkg.etc2_kernel_name(16, 4, 0) == pkg.kernel_name(16, 4)
    assert "icamd_encode_etc2_device" in pkg.EXPORTS and "icamd_etc2_kernel_name" in pkg.EXPORTS


def test_python_keyword_reaches_the_new_entry_point(monkeypatch):
    calls = []
    real = pkg.lib()

    class Tensor:  # what encode_device touches of a tensor, without a device
        is_cuda, dtype, device = True, pkg.torch.uint8, "cpu"

        def is_contiguous(self):
            return True

        def data_ptr(self):
            return 16

    class Lib:
        def icamd_encode_device(self, *a):
            calls.append(("encode", a))
            return 0

        def icamd_encode_etc2_device(self, *a):
            calls.append(("etc2", a))
            return 0

        def icamd_encoded_size(self, codec, gh, gw):
            return real.icamd_encoded_size(codec, gh, gw)

    monkeypatch.setattr(pkg, "lib", lambda: Lib())
    monkeypatch.setattr(pkg, "_stream_handle", lambda stream=None: None)
    out = pkg.torch.empty((1, 32), dtype=pkg.torch.uint8)
    pkg.encode_device(18, Tensor(), 8, 8, 3, out=out)
    pkg.encode_device(18, Tensor(), 8, 8, 3, out=out, etc2_modes=0)
    pkg.encode_device(18, Tensor(), 8, 8, 3, out=out, etc2_modes=pkg.ETC2_MODES_TH, etc_strategy=1)
    assert [c[0] for c in calls] == ["encode", "encode", "etc2"]
    assert calls[0][1] == calls[1][1]
    assert calls[2][1][:4] == (18, 1, 1, 3) and calls[2][1][4:] == calls[0][1][3:]


# ---- build check: the T / H kernels keep everything in registers

def test_th_kernels_use_no_scratch(tmp_path):
    import re
    import shutil
    if not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    out = os.path.join(str(tmp_path), "etc2_th_kernels.s")
    cc = subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(T.ROOT, "include"),
                         "-I" + CSRC, "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "etc2_th_kernels.hip")],
                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert cc.returncode == 0, "hipcc failed:\n" + cc.stdout
    metas = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", open(out).read(), re.S):
        blk = m.group(0)
        metas[re.search(r"\.name:\s+(\S+)", blk).group(1)] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
    assert metas == {"icamd_etc2_th_rgb888_kernel": 0, "icamd_etc2_th_rgba8_kernel": 0}
