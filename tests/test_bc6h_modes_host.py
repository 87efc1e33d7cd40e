"""CPU tier for BC6H's opt-in two-subset candidate (include/ic_amd.h ICAMD_BC6H_MODES_EXTENDED).

* The definition's numpy restatement (tests/bc6h_modes_oracle.py) through PINNED code: what it writes, decoded by bc6h_oracle's
  decode_blocks (held bit by bit to an independent decoder in tests/test_bc6h_host.py), has exactly the sse it claims.
* The host twin of csrc/bc6h_modes_block.h (tests/host_emul/bc6h_modes_emul.cc, -DICAMD_HOST_EMULATION) byte for byte against the
  restatement on every shape, layout, channel count, format and content.
* The fixture's adequacy, asserted on the oracle alone: every ladder field written, kept blocks, every refit outcome, both anchor
  exchanges, negative endpoints in the signed format.
* Block-level promises, the closed form of Q_b against the definition for every T and b, the C ABI's host-side surface, the
  header's worked example, and the new kernels' scratch size (0)."""
import ctypes
import functools
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bc6h_modes_oracle as M
import bc6h_oracle as B
import ic_testlib as T

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, "host_emul")
CSRC = os.path.join(T.ROOT, "image-compression_amd", "csrc")
pkg = importlib.import_module("image-compression_amd")
UF16, SF16 = B.BC6H_UF16, B.BC6H_SF16
CODECS = (UF16, SF16)
SHAPES = [(1, 1), (4, 4), (5, 3), (9, 2), (61, 59)]
PAD = 6  # bytes of row padding
PADDED = [(5, 3, 16, 16), (30, 30, 40, 48)]
SCRATCH_BYTES = 0  # what DESIGN.md 3.24 states for the new kernels
i32 = ctypes.c_int32


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("bc6h_modes") / "libbc6h_modes_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-DICAMD_HOST_EMULATION", "-I" + CSRC,
                           "-I" + os.path.join(T.ROOT, "include"), "-o", so, os.path.join(EMUL_DIR, "bc6h_modes_emul.cc")])
    L = ctypes.CDLL(so)
    L.bc6h_modes_emul_encode.restype = ctypes.c_int
    L.bc6h_modes_emul_encode.argtypes = [T.ci, T.ci, T.ci, T.u32, T.u32, T.u32, T.u32, T.u32, T.vp, T.vp]
    L.bc6h_modes_emul_quantise.restype = None
    L.bc6h_modes_emul_quantise.argtypes = [T.ci, T.u32, i32, i32, T.vp]
    L.bc6h_modes_emul_endpoint_value.restype = i32
    L.bc6h_modes_emul_endpoint_value.argtypes = [T.ci, T.u32, i32]
    yield L
    T.assert_no_emul_violations(L, "test_bc6h_modes_host")


def emul_encode(L, img, signed, gh=None, gw=None, pad=0, modes=M.MODES_EXTENDED):
    h, w, chans = img.shape
    out = np.zeros(B.encoded_size(max(h, gh or h), max(w, gw or w)), np.uint8)
    rows = np.zeros((h, w * chans + pad // 2), np.uint16)
    rows[:, :w * chans] = img.reshape(h, w * chans)
    assert L.bc6h_modes_emul_encode(modes, int(signed), chans, h, w, gh or h, gw or w, w * chans * 2 + pad, rows.ctypes.data,
                                    out.ctypes.data)
    return out.tobytes()


@functools.lru_cache(maxsize=None)
def _image(name, h, w, chans):
    img = M.content(name, h, w, chans)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _want(name, h, w, chans, signed, gh=None, gw=None):
    return M.oracle_encode(_image(name, h, w, chans), signed, gh, gw)


def green_probe_blocks():
    """[n, 16, 3] half bits (all positive, t = the bits): two ramps per block over partition 0 (columns 0-1 | columns 2-3) whose
    gap is 16-31 eight-bit steps in G and under 16 in R and B, in either format's steps: the blocks the rung 10110 is for."""
    out = []
    for base in (3000, 9000, 14000):
        for gr, gg in ((1000, 3000), (1500, 3700), (2000, 5500), (2600, 7000)):
            blk = np.zeros((16, 3), np.int64)
            for i in range(16):
                side, y = (i % 4) >= 2, i // 4
                blk[i] = (base + 40 * y + side * gr, base + 500 + 30 * y + side * gg, base + 900 + 50 * y + side * gr)
            out.append(blk)
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def _fixture(signed):
    """(t [N, 16, 3], blocks [N, 16], stages): every content at 32 x 32, the edge content at 64 x 64, the 10110 probes."""
    t = [B.block_texels(_image(name, 32, 32, 3), signed) for name in B.CONTENTS]
    t.append(B.block_texels(_image("edge", 64, 64, 3), signed))
    t.append(B.target(green_probe_blocks(), signed))
    t = np.concatenate(t)
    blocks, st = M.encode_texels(t, signed, stages=True)
    return t, blocks, st


# ---- the definition through pinned code

@pytest.mark.parametrize("signed", [False, True])
def test_claimed_sse_is_what_the_pinned_decoder_makes_of_every_block(signed):
    t, blocks, st = _fixture(signed)
    dec = B.target(B.decode_blocks(blocks, signed), signed)
    real = ((dec - t) ** 2).sum(axis=(1, 2))
    assert (real == st["claimed"]).all()
    assert (st["claimed"] == np.where(st["chosen"], st["sse2"], st["sse1"])).all()
    assert (st["sse2"] == st["final"].sum(axis=0)).all() and (st["final"] <= st["first"]).all()
    fields = M.block_fields(blocks)
    assert ((fields == M.ONE_SUBSET_FIELD) == ~st["chosen"]).all()
    assert (fields[st["chosen"]] == np.array(M.LADDER_FIELDS)[st["ladder"][st["chosen"]]]).all()


# ---- twin against oracle

@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("chans", [3, 4])
def test_twin_matches_definition_on_every_shape(emul, signed, chans):
    for h, w in SHAPES:
        img = _image("edge", h, w, chans)
        want = _want("edge", h, w, chans, signed)
        assert emul_encode(emul, img, signed) == want, (h, w)
        assert emul_encode(emul, img, signed, pad=PAD) == want, (h, w, "padded rows")


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("name", M.CONTENTS)
def test_twin_matches_definition_on_every_content(emul, signed, name):
    for chans in (3, 4):
        assert emul_encode(emul, _image(name, 61, 59, chans), signed) == _want(name, 61, 59, chans, signed), chans


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("h,w,gh,gw", PADDED)
def test_twin_padded_grid(emul, signed, h, w, gh, gw):
    for chans, name in ((3, "edge"), (4, "noise")):
        want = _want(name, h, w, chans, signed, gh, gw)
        assert len(want) == B.encoded_size(gh, gw)
        assert emul_encode(emul, _image(name, h, w, chans), signed, gh, gw) == want, (chans, name)


@pytest.mark.parametrize("signed", [False, True])
def test_twin_on_the_fixture_and_the_wave_image(emul, signed):
    t, blocks, _ = _fixture(signed)
    probes = green_probe_blocks().astype(np.uint16)
    img = np.ascontiguousarray(probes.reshape(-1, 4, 4, 3).transpose(1, 0, 2, 3).reshape(4, -1, 3))
    assert emul_encode(emul, img, signed) == blocks[-len(probes):].tobytes()
    wave, _ = M.wave_image(signed)
    assert emul_encode(emul, wave, signed) == M.oracle_encode(wave, signed)


def test_default_through_the_twin_is_the_one_subset_definition(emul):
    for signed in (False, True):
        for name in ("edge", "noise"):
            img = _image(name, 61, 59, 4)
            assert emul_encode(emul, img, signed, pad=PAD, modes=M.MODES_DEFAULT) == B.oracle_encode(img, signed), (signed, name)
            assert M.oracle_encode(img, signed, modes=M.MODES_DEFAULT) == B.oracle_encode(img, signed)


# ---- the fixture is adequate (conditions on the oracle alone)

@pytest.mark.parametrize("signed", [False, True])
def test_fixture_reaches_every_branch_of_the_definition(signed):
    t, blocks, st = _fixture(signed)
    chosen = st["chosen"]
    fields = M.block_fields(blocks)
    for f in M.LADDER_FIELDS:
        assert (fields == f).any(), bin(f)
    assert (fields == M.ONE_SUBSET_FIELD).any()
    for outcome in (M.TAKEN, M.NOT_BETTER, M.INFEASIBLE):
        assert ((st["refit"] == outcome) & chosen[None, :]).any(), outcome
    for j in (0, 1):
        assert (st["flips"][j] & chosen).any() and (~st["flips"][j] & chosen).any(), j
    negative = (st["E"] < 0).any(axis=(1, 2))
    if signed:
        assert (negative & chosen).any()
        assert (st["ladder"][negative] == len(M.LADDER) - 1).all()
        assert (fields[negative & chosen] == M.LADDER_FIELDS[-1]).all()
    else:
        assert not negative.any()
    # the wave image: every flag it can show is true in some lanes and false in others
    _, flags = M.wave_image(signed)
    for name, f in flags.items():
        if name == "negative endpoint" and not signed:
            assert not f.any()
        else:
            assert f.any() and not f.all(), name


# ---- block-level properties

@pytest.mark.parametrize("signed", [False, True])
def test_no_block_is_worse_than_default_and_flat_blocks_are_kept(signed):
    t, blocks, st = _fixture(signed)
    assert (st["claimed"] <= st["sse1"]).all() and (st["claimed"][st["chosen"]] < st["sse1"][st["chosen"]]).all()
    for name in ("flat", "two_valued"):
        img = _image(name, 32, 32, 3)
        assert M.oracle_encode(img, signed) == B.oracle_encode(img, signed), name
    ratio = {}
    for name, hw in (("edge", 64), ("ldr", 32)):
        _, s = M.encode_texels(B.block_texels(_image(name, hw, hw, 3), signed), signed, stages=True)
        ratio[name] = s["claimed"].sum() / s["sse1"].sum()
    print("sse EXTENDED / DEFAULT:", ratio)
    assert ratio["edge"] < 1 and ratio["ldr"] < 1


@pytest.mark.parametrize("signed", [False, True])
def test_stored_deltas_are_within_range_without_wrap_around(signed):
    t, blocks, st = _fixture(signed)
    sel = np.flatnonzero(st["chosen"])
    for n, (m, e0, d) in zip(sel, M.stored_endpoints(blocks[sel], signed)):
        _, _, ep, delta, transformed, ns, _ = B.MODES[m]
        assert ns == 2 and m == M.LADDER[st["ladder"][n]]
        lo, hi = M.q_range(ep, signed)
        E = st["E"][n]  # [endpoint, channel], after the anchor exchanges
        for c in range(3):
            assert e0[c] == E[0, c]
            for k in (1, 2, 3):
                if transformed:
                    assert -(1 << (delta[c] - 1)) <= d[c][k - 1] < (1 << (delta[c] - 1))
                    assert lo <= e0[c] + d[c][k - 1] <= hi and e0[c] + d[c][k - 1] == E[k, c], (n, c, k)  # no wrap
                    assert not signed or E[k, c] >= 0
                else:  # 11110: the endpoints themselves, six bits each
                    assert (d[c][k - 1] & 63) == (int(E[k, c]) & 63) and lo <= E[k, c] <= hi


# ---- Q_b

@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("b", [6, 7, 8, 9, 10])
def test_quantiser_closed_form_equals_the_definition_for_every_target(emul, signed, b):
    lo, hi = (-B.T_MAX, B.T_MAX) if signed else (0, B.T_MAX)
    T_all = np.arange(lo, hi + 1)
    got = np.zeros(len(T_all), np.int32)
    emul.bc6h_modes_emul_quantise(int(signed), b, lo, hi, got.ctypes.data)
    want = np.concatenate([M.quantise(T_all[i:i + 4096], b, signed) for i in range(0, len(T_all), 4096)])
    assert (got == want).all()
    qlo, qhi = M.q_range(b, signed)
    q = np.arange(qlo, qhi + 1)
    d = np.array([emul.bc6h_modes_emul_endpoint_value(int(signed), b, int(x)) for x in q])
    assert (d == M.D(q, b, signed)).all() and (np.diff(d) > 0).all()
    assert d[-1] == B.T_MAX and d[0] == (-B.T_MAX if signed else 0)
    assert want.min() == qlo and want.max() == qhi
    if b == 10:  # the one-subset definition's grid
        assert (want[::7] == B.quantise(T_all[::7], signed)).all()


# ---- the C ABI's host-side surface (no device work: every check below returns before the GPU is touched)

def _name(codec, chans, modes):
    if codec not in CODECS or chans not in (3, 4) or modes not in (0, 1):
        return ""
    return "icamd_bc6h_%s%s_%s_kernel" % ("modes_" if modes else "", "uf16" if codec == UF16 else "sf16",
                                           "rgb16f" if chans == 3 else "rgba16f")


def test_kernel_names_and_constants():
    assert (pkg.BC6H_MODES_DEFAULT, pkg.BC6H_MODES_EXTENDED) == (0, 1) == (M.MODES_DEFAULT, M.MODES_EXTENDED)
    for codec in list(CODECS) + [0, 32, 33, 36]:
        for chans in range(0, 6):
            for modes in (-1, 0, 1, 2, 32):
                assert pkg.bc6h_modes_kernel_name(codec, chans, modes) == _name(codec, chans, modes), (codec, chans, modes)
            assert pkg.bc6h_modes_kernel_name(codec, chans, 0) == pkg.bc6h_kernel_name(codec, chans)
    assert pkg.bc6h_modes_kernel_name(UF16, 4, 1) == "icamd_bc6h_modes_uf16_rgba16f_kernel"
    assert "icamd_encode_bc6h_modes_device" in pkg.EXPORTS and "icamd_bc6h_modes_kernel_name" in pkg.EXPORTS


def test_statuses_in_their_order():
    lib = pkg.lib()
    enc = lib.icamd_encode_bc6h_modes_device
    d = ctypes.c_void_p(16)  # never dereferenced: the arguments are refused first
    odd = ctypes.c_void_p(17)
    # 1. a null pointer or an empty image is ICAMD_FALSE, whatever else is wrong
    for codec, modes, chans in ((UF16, 0, 3), (SF16, 1, 4), (7, 9, 9)):
        assert enc(codec, modes, chans, 0, 8, 8, 8, 1, 1, 0, 0, d, d, None) == 1
        assert enc(codec, modes, chans, 8, 0, 8, 8, 1, 1, 0, 0, d, d, None) == 1
        assert enc(codec, modes, chans, 8, 8, 8, 8, 1, 1, 0, 0, None, d, None) == 1
        assert enc(codec, modes, chans, 8, 8, 8, 8, 1, 1, 0, 0, d, None, None) == 1
    # 2. the domain, before the empty batch
    for codec in (-1, 0, 5, 32, 33, 36):
        for modes in (0, 1):
            assert enc(codec, modes, 3, 8, 8, 8, 8, 48, 0, 0, 0, d, d, None) == -4, codec
    for codec in CODECS:
        for modes in (-1, 2, 6):
            assert enc(codec, modes, 4, 8, 8, 8, 8, 64, 0, 0, 0, d, d, None) == -4
            assert b"bc6h_modes" in lib.icamd_last_error()
        for modes in (0, 1):
            for chans in (0, 1, 2, 5):
                assert enc(codec, modes, chans, 8, 8, 8, 8, 64, 0, 0, 0, d, d, None) == -4
                assert b"channels" in lib.icamd_last_error()
            for n in (0, 1):  # 2-byte alignment is a rule: refused whatever the count
                assert enc(codec, modes, 3, 8, 8, 8, 8, 48, n, 0, 0, odd, d, None) == -4
                assert b"even" in lib.icamd_last_error()
                assert enc(codec, modes, 3, 8, 8, 8, 8, 49, n, 0, 0, d, d, None) == -4
                assert enc(codec, modes, 3, 8, 8, 8, 8, 48, n, 1001, 0, d, d, None) == -4
            for chans in (3, 4):
                # 3. the empty batch, before the stride
                assert enc(codec, modes, chans, 8, 8, 8, 8, 2, 0, 0, 0, d, d, None) == 0
                assert enc(codec, modes, chans, 8, 8, 8, 8, 16 * chans, 0, 0, 0, d, odd, None) == 0  # the output: any alignment
                # 4. the stride
                assert enc(codec, modes, chans, 8, 8, 8, 8, 16 * chans - 2, 1, 0, 0, d, d, None) == -4
                assert b"row stride" in lib.icamd_last_error()
                # 5. everything in order, and no device here
                if lib.icamd_device_count() == 0:
                    assert enc(codec, modes, chans, 8, 8, 8, 8, 16 * chans, 1, 0, 0, d, d, None) == -1  # ICAMD_ERR_NO_DEVICE


def test_prototype_table_matches_the_header():
    import test_abi_exports as X
    header = X.header_prototypes()
    new = ["icamd_encode_bc6h_modes_device", "icamd_bc6h_modes_kernel_name"]
    assert all(n in header for n in new)
    assert X.prototype_mismatches(header, pkg.abi.PROTOTYPES) == []
    names = [n for n, _, _ in pkg.abi.PROTOTYPES]
    assert names[names.index("icamd_bc6h_metric_kernel_name") + 1:][:2] == new  # header order
    entry = dict((n, (r, a)) for n, r, a in pkg.abi.PROTOTYPES)["icamd_encode_bc6h_modes_device"]
    assert entry[0] is ctypes.c_int and len(entry[1]) == 14
    lib = ctypes.CDLL(pkg.LIB_PATH)
    assert all(hasattr(lib, n) for n in new)


def test_header_example_blocks(emul):
    img = np.zeros((4, 4, 3), np.uint16)
    img[0], img[1] = (0x3C00, 0x3800, 0x3400), (0x3C40, 0x3800, 0x3400)
    img[2], img[3] = (0x3D00, 0x3700, 0x3480), (0x3D00, 0x3740, 0x3480)
    header = open(os.path.join(T.ROOT, "include", "ic_amd.h")).read()
    for signed, text, sse in ((False, "e4 3d e7 5a 13 15 40 80 50 a4 01 e0 ff ff 3f 49", (16024, 940)),
                              (True, "e4 9e 73 ac 09 1b 60 50 08 a2 29 e9 ff ff 7f db", (23840, 13944))):
        want = bytes.fromhex(text)
        assert text in header
        assert M.oracle_encode(img, signed) == want and emul_encode(emul, img, signed) == want
        _, st = M.encode_texels(B.block_texels(img, signed), signed, stages=True)
        assert (int(st["sse1"][0]), int(st["sse2"][0])) == sse and st["partition"][0] == 13 and st["ladder"][0] == 0
        assert [bool(f[0]) for f in st["flips"]] == [False, True] and (st["refit"][:, 0] == M.NOT_BETTER).all()
        if not signed:
            assert st["E"][0].tolist() == [[495, 462, 429], [497, 462, 429], [503, 456, 433], [503, 454, 433]]
            assert st["first"][:, 0].tolist() == [56, 884]


# ---- build check: the new kernels' scratch size is what DESIGN.md states

def test_bc6h_modes_kernels_scratch_size(tmp_path):
    if not shutil.which("hipcc"):
        pytest.skip("hipcc not available")
    out = str(tmp_path / "bc6h_modes_kernels.s")
    subprocess.check_call(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(T.ROOT, "include"),
                           "-I" + CSRC, "-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "bc6h_modes_kernels.hip")],
                          stderr=subprocess.DEVNULL)
    metas = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", open(out).read(), re.S):
        blk = m.group(0)
        metas[re.search(r"\.name:\s+(\S+)", blk).group(1)] = (int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)),
                                                              int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)))
    names = [_name(c, n, 1) for c in CODECS for n in (3, 4)]
    names += [n.replace("_kernel", "_narrow_kernel") for n in names]
    assert len(names) == 8
    for n in names:
        assert n in metas, n
        assert metas[n] == (SCRATCH_BYTES, 0), "%s uses %d bytes of scratch, %d spilled VGPRs" % ((n,) + metas[n])
    design = open(os.path.join(T.ROOT, "DESIGN.md")).read()
    assert "scratch: %d bytes" % SCRATCH_BYTES in design[design.index("### 3.24"):]
