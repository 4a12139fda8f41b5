"""The host half of the JPEG decoder, without a GPU: yxh_jpeg_probe / yxh_jpeg_decode and the scalar
render yxh_jpeg_render_host against PIL byte for byte, the refused kinds, damaged input against guard
bytes, JpegDecoder's routing, and the stand-alone sanitizer build of tools/jpeg_check.cpp."""
import ctypes as C
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_cases as J
from conftest import PKG_ROOT, REPO

EVERY = {**J.SUPPORTED, **J.GOLDEN_IMAGES}


@pytest.fixture(scope="module")
def N():
    from yolox_amd import _native
    _native.lib()
    return _native


@pytest.fixture(scope="module")
def rendered(N):
    """name -> the host render of every supported fixture, decoded once and rendered as ONE ragged batch."""
    images, coefs = [], []
    for name in EVERY:
        rc, _, image, coef, intact = J.host_decode(J.fixture_bytes(name))
        assert rc == N.OK and intact, (name, rc, N.lib().yxh_last_error())
        images.append(image)
        coefs.append(coef)
    return dict(zip(EVERY, J.host_render(images, coefs)))


def test_abi_entries_and_layouts(N):
    lib = N.lib()
    assert lib.yxh_sizeof_jpeg_info() == C.sizeof(N.JpegInfo) == 24
    assert lib.yxh_sizeof_jpeg_image() == C.sizeof(N.JpegImage) == 464
    assert {"yxh_jpeg_probe", "yxh_jpeg_decode", "yxh_jpeg_render_host", "yxh_jpeg_render_batch",
            "yxh_jpeg_workspace_bytes"} <= set(N.EXPORTED)
    assert lib.yxh_abi_version() == 21  # additive: no new ABI version
    info = N.JpegInfo()
    assert lib.yxh_jpeg_probe(None, 0, C.byref(info)) == N.EINVAL
    assert lib.yxh_jpeg_render_batch(None, None, 1, None, None, None) == N.EINVAL  # before any launch
    assert lib.yxh_jpeg_workspace_bytes(0, 5, J.S420) == 0 and lib.yxh_jpeg_workspace_bytes(5, 5, 9) == 0
    # planes padded to whole MCUs: 17 x 17 at 4:2:0 is 2 x 2 MCUs of 16 x 16 luma + 2 of 8 x 8 chroma
    assert lib.yxh_jpeg_workspace_bytes(17, 17, J.S420) == 32 * 32 + 2 * 16 * 16


@pytest.mark.parametrize("name", list(EVERY))
def test_probe_reports_the_file(N, name):
    h, w, comps, sampling = EVERY[name]
    info = N.JpegInfo()
    data = J.fixture_bytes(name)
    assert N.lib().yxh_jpeg_probe(data, len(data), C.byref(info)) == N.OK
    assert (info.height, info.width, info.components, info.sampling) == (h, w, comps, sampling)
    assert info.coef_bytes == J.mcu_blocks(h, w, sampling) * 128


@pytest.mark.parametrize("name", list(EVERY))
def test_host_render_equals_pil_byte_for_byte(rendered, name):
    got = rendered[name]
    live = J.pil_rgb(J.fixture_bytes(name))
    assert got.shape == live.shape and got.dtype == np.uint8
    assert np.array_equal(got, live), f"{int((got != live).sum())} bytes differ from the live PIL decode"
    if name in J.SUPPORTED:
        assert np.array_equal(got, J.recorded()[name]), "differs from the recorded decode"


def test_descriptor_holds_the_layout(N):
    rc, info, image, coef, _ = J.host_decode(J.fixture_bytes("420_37x53"))
    assert rc == N.OK
    # 37 x 53 at 4:2:0: 4 x 3 MCUs -> luma 8 x 6 blocks, chroma 4 x 3
    assert list(image.blocks_w) == [8, 4, 4] and list(image.blocks_h) == [6, 3, 3]
    assert list(image.comp_block0) == [0, 48, 60]
    assert (image.coef_offset, image.dst_offset, image.ws_offset) == (0, 0, 0)
    assert coef.size == 72 * 64
    q = np.ctypeslib.as_array(image.quant)
    from PIL import Image
    with Image.open(J.fixture_path("420_37x53")) as im:
        tables = im.quantization
    zigzag = np.argsort(np.array(  # natural index of each zigzag position -> back to natural order
        [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
         21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
         60, 61, 54, 47, 55, 62, 63]))
    for c, t in enumerate((0, 1, 1)):
        want = np.array(tables[t])
        assert sorted(q[c].tolist()) == sorted(want.tolist())
        # PIL hands the tables out in either order depending on its version: one of the two matches
        assert np.array_equal(q[c], want) or np.array_equal(q[c], want[zigzag])


@pytest.mark.parametrize("name", J.UNSUPPORTED)
def test_other_kinds_are_unsupported_with_a_reason(N, name):
    data = J.fixture_bytes(name)
    info = N.JpegInfo()
    assert N.lib().yxh_jpeg_probe(data, len(data), C.byref(info)) == N.EUNSUPPORTED
    reason = N.lib().yxh_last_error().decode()
    assert reason.startswith("jpeg: ") and len(reason) > 10
    buf = np.zeros(1 << 16, np.int16)
    image = N.JpegImage()
    assert N.lib().yxh_jpeg_decode(data, len(data), buf.ctypes.data, buf.nbytes, C.byref(image)) == N.EUNSUPPORTED
    assert not buf.any()


def test_freshly_written_kinds(N):
    """The same kinds written now by the installed PIL (the committed files are one encoder's)."""
    from PIL import Image
    rng = np.random.default_rng(5)
    img = Image.fromarray(rng.integers(0, 256, (24, 40, 3), dtype=np.uint8))

    def probe(**kw):
        buf = io.BytesIO()
        kw.pop("im", img).save(buf, "JPEG", **kw)
        data = buf.getvalue()
        return N.lib().yxh_jpeg_probe(data, len(data), C.byref(N.JpegInfo())), data

    assert probe(progressive=True)[0] == N.EUNSUPPORTED
    assert probe(im=img.convert("CMYK"))[0] == N.EUNSUPPORTED
    rc, data = probe(subsampling="4:2:2", quality=40)
    assert rc == N.OK
    rc, _, image, coef, intact = J.host_decode(data)
    assert rc == N.OK and intact
    assert np.array_equal(J.host_render([image], [coef])[0], J.pil_rgb(data))


def test_buffer_too_small_is_refused_untouched(N):
    data = J.fixture_bytes("420_17x17_q30")
    buf = np.full(3072 + 64, 0xA5, np.uint8)
    image = N.JpegImage()
    assert N.lib().yxh_jpeg_decode(data, len(data), buf.ctypes.data, 3071, C.byref(image)) == N.EINVAL
    assert (buf == 0xA5).all()


def test_png_and_every_truncation_error_or_decode_fully(N):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(buf, "PNG")
    rc, _, _, _, intact = J.host_decode(buf.getvalue())
    assert rc == N.EINVAL and intact
    data = J.fixture_bytes("420_17x17_q30")
    full = J.recorded()["420_17x17_q30"]
    outcomes = {}
    for cut in range(len(data)):
        rc, _, image, coef, intact = J.host_decode(data[:cut])
        assert intact, f"prefix of {cut} bytes: guard bytes around the coefficient buffer were written"
        assert rc in (N.OK, N.EINVAL, N.EUNSUPPORTED), (cut, rc)
        outcomes[rc] = outcomes.get(rc, 0) + 1
        if rc == N.OK:  # only the trailing EOI marker (and its fill) may be missing
            assert cut >= len(data) - 2, cut
            assert np.array_equal(J.host_render([image], [coef])[0], full)
    assert outcomes.get(N.EINVAL, 0) >= len(data) - 2


def test_restart_markers_are_checked(N):
    data = bytearray(J.fixture_bytes("420_50x70_rst3"))
    at = [i for i in range(len(data) - 1) if data[i] == 0xFF and 0xD0 <= data[i + 1] <= 0xD7]
    assert len(at) >= 3  # 5 x 4 MCUs, a marker every 3
    data[at[1] + 1] = 0xD0 + ((data[at[1] + 1] - 0xD0 + 3) & 7)  # the wrong number
    rc, _, _, _, intact = J.host_decode(bytes(data))
    assert rc == N.EINVAL and intact


def test_decode_is_thread_safe(N):
    """Sixteen threads decode different files at once: every result equals the single-threaded one."""
    from concurrent.futures import ThreadPoolExecutor
    names = [n for n in J.SUPPORTED] * 6
    single = {n: J.host_decode(J.fixture_bytes(n))[3].copy() for n in J.SUPPORTED}
    with ThreadPoolExecutor(16) as ex:
        got = list(ex.map(lambda n: J.host_decode(J.fixture_bytes(n))[3], names))
    for n, cf in zip(names, got):
        assert np.array_equal(cf, single[n]), n


def test_exif_orientation_reader():
    from PIL import Image

    from yolox_amd.jpeg import exif_orientation
    assert exif_orientation(J.fixture_bytes("420_37x53")) == 1
    for order in (6, 3, 1):
        buf = io.BytesIO()
        exif = Image.Exif()
        exif[0x0112] = order
        Image.fromarray(np.zeros((8, 12, 3), np.uint8)).save(buf, "JPEG", exif=exif)
        assert exif_orientation(buf.getvalue()) == order


def test_decoder_routes_each_fixture(N, monkeypatch):
    from yolox_amd import jpeg
    from yolox_amd.jpeg import JpegDecoder, device_path_enabled
    monkeypatch.delenv("YOLOX_AMD_JPEG", raising=False)
    assert device_path_enabled() is jpeg.DEFAULT_ON is True  # chosen by measurement
    dec = JpegDecoder(workers=64, enabled=True)
    assert dec.workers == 16
    taken = [dec.accept(J.fixture_bytes(n), gray=True) for n in J.SUPPORTED]
    assert all(e is not None for e in taken)
    assert [(e.height, e.width, e.components, e.sampling) for e in taken] == list(J.SUPPORTED.values())
    total = sum((e.coef_bytes + 15) // 16 * 16 for e in taken)
    staging = J.aligned(total)
    offs = np.cumsum([0] + [(e.coef_bytes + 15) // 16 * 16 for e in taken])[:-1]
    res = dec.decode(taken, staging.ctypes.data, offs)
    assert all(err is None for _, err in res)
    # the condition that keeps a fallback from hiding a failure: nothing of the supported list went to PIL
    assert dec.stats == {"device": len(J.SUPPORTED), "pil": 0, "reasons": {}}
    coefs = [staging[o:o + e.coef_bytes].view(np.int16) for o, e in zip(offs, taken)]
    for name, out in zip(J.SUPPORTED, J.host_render([im for im, _ in res], coefs)):
        assert np.array_equal(out, J.recorded()[name]), name
    # the other side
    for n in J.UNSUPPORTED:
        assert dec.accept(J.fixture_bytes(n)) is None
    assert dec.accept(J.fixture_bytes("gray_19x45")) is None  # serving keeps PIL's 2-D array
    assert dec.accept(b"\x89PNG\r\n\x1a\n" + bytes(32)) is None
    s = dec.stats
    assert s["device"] == len(J.SUPPORTED) and s["pil"] == len(J.UNSUPPORTED) + 2 == sum(s["reasons"].values())
    assert s["reasons"]["jpeg: progressive"] == 1 and s["reasons"]["grayscale"] == 1 and s["reasons"]["not a JPEG"] == 1
    # a file the probe takes and the entropy decoder refuses is handed on with its reason
    data = J.fixture_bytes("420_17x17_q30")
    before = dec.stats["pil"]
    e = dec.accept(data[:-6])
    assert e is not None
    (image, err), = dec.decode([e], staging.ctypes.data, [0])
    assert image is None and err.startswith("jpeg: ") and dec.stats["pil"] == before + 1
    assert dec.stats["device"] == len(J.SUPPORTED)
    # the switch
    off = JpegDecoder(enabled=None)
    monkeypatch.setenv("YOLOX_AMD_JPEG", "0")
    assert not device_path_enabled() and off.accept(data) is None and off.stats["reasons"] == {"device path off": 1}
    monkeypatch.setenv("YOLOX_AMD_JPEG", "1")
    assert device_path_enabled() and off.accept(data) is not None
    monkeypatch.setenv("YOLOX_AMD_JPEG", "yes")
    with pytest.raises(ValueError, match="YOLOX_AMD_JPEG"):
        device_path_enabled()
    dec.close()


def test_as_array_takes_encoded_bytes():
    from yolox_amd.serve import as_array
    data = J.fixture_bytes("444_40x56_bw_q20")
    want = J.recorded()["444_40x56_bw_q20"]
    for kind in (bytes, bytearray, memoryview):
        assert np.array_equal(as_array(kind(data)), want)


def test_standalone_checker_under_sanitizers(tmp_path):
    """tools/jpeg_check.cpp + csrc/jpeg_host.cpp alone, built with the host compiler and ASan + UBSan:
    the fixtures decode, and seeded truncations and byte flips of them only ever return."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "jpeg_check")
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "-DYXH_JPEG_STANDALONE", "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(PKG_ROOT, "csrc"),
         os.path.join(REPO, "tools", "jpeg_check.cpp"), os.path.join(PKG_ROOT, "csrc", "jpeg_host.cpp"), "-o", exe],
        capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr and ("cannot find" in build.stderr or "unsupported" in build.stderr):
        pytest.skip("the host compiler has no sanitizer runtimes")
    assert build.returncode == 0, build.stderr[-2000:]
    small = [n for n in list(J.SUPPORTED) + J.UNSUPPORTED if n != "420_239x317"]
    run = subprocess.run([exe] + [J.fixture_path(n) for n in small], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-3000:])
    lines = run.stdout.splitlines()
    for n in small:
        line = next(ln for ln in lines if J.fixture_path(n) in ln)
        assert line.startswith("ok " if n in J.SUPPORTED else "rc -3 "), line
    assert lines[-1].endswith(" 0 guard failures")
