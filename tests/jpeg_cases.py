"""Shared by the JPEG tests: the fixture lists of tests/golden/jpeg (written by
tests/golden/make_golden_jpeg.py) and the host decode + render through the C ABI."""
import ctypes as C
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
JPEG_DIR = os.path.join(GOLDEN, "jpeg")

GRAY, S444, S422, S420 = 0, 1, 2, 3

# name -> (height, width, components, sampling): what the probe must report
SUPPORTED = {
    "420_1x1": (1, 1, 3, S420),
    "420_17x17_q30": (17, 17, 3, S420),
    "420_37x53": (37, 53, 3, S420),
    "420_64x96_q95": (64, 96, 3, S420),
    "420_31x33_q100": (31, 33, 3, S420),
    "420_239x317": (239, 317, 3, S420),
    "420_50x70_rst3": (50, 70, 3, S420),
    "420_40x56_noise_q100": (40, 56, 3, S420),
    "422_41x23_q60": (41, 23, 3, S422),
    "422_33x64_rstrow_opt": (33, 64, 3, S422),
    "444_1x1": (1, 1, 3, S444),
    "444_40x56_bw_q20": (40, 56, 3, S444),
    "gray_19x45": (19, 45, 1, GRAY),
}
UNSUPPORTED = ["progressive_24x40", "cmyk_24x40", "411_24x40", "440_24x40"]
GOLDEN_IMAGES = {  # the project's three golden photographs, 4:4:4
    "000000000001": (480, 640, 3, S444),
    "000000000009": (480, 640, 3, S444),
    "000000000016": (640, 480, 3, S444),
}


def fixture_path(name: str) -> str:
    if name in GOLDEN_IMAGES:
        return os.path.join(GOLDEN, "images", name + ".jpg")
    return os.path.join(JPEG_DIR, name + ".jpg")


def fixture_bytes(name: str) -> bytes:
    with open(fixture_path(name), "rb") as f:
        return f.read()


def recorded() -> dict:
    with np.load(os.path.join(JPEG_DIR, "decoded.npz")) as z:
        return {k: z[k] for k in z.files}


def pil_rgb(data: bytes) -> np.ndarray:
    import io

    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"))


def mcu_blocks(h: int, w: int, sampling: int) -> int:
    """Blocks of an image with block rows padded to whole MCUs (the coefficient layout)."""
    hm, vm = {GRAY: (1, 1), S444: (1, 1), S422: (2, 1), S420: (2, 2)}[sampling]
    mx, my = -(-w // (8 * hm)), -(-h // (8 * vm))
    return mx * my * (hm * vm + (0 if sampling == GRAY else 2))


GUARD = 64


def host_decode(data: bytes, guard: int = GUARD):
    """probe + decode into a guarded buffer -> (rc, info, image, coef int16 array or None, guards intact)."""
    from yolox_amd import _native as N
    lib = N.lib()
    info = N.JpegInfo()
    rc = lib.yxh_jpeg_probe(data, len(data), C.byref(info))
    if rc != N.OK:
        return rc, info, None, None, True
    n = int(info.coef_bytes)
    buf = np.full(n + 2 * guard, 0xA5, np.uint8)
    image = N.JpegImage()
    rc = lib.yxh_jpeg_decode(data, len(data), buf.ctypes.data + guard, n, C.byref(image))
    intact = bool((buf[:guard] == 0xA5).all() and (buf[guard + n:] == 0xA5).all())
    coef = buf[guard:guard + n].view(np.int16) if rc == N.OK else None
    return rc, info, image, coef, intact


def aligned(nbytes: int) -> np.ndarray:
    """A zeroed uint8 array of ``nbytes`` (a multiple of 16) whose data is 16-byte aligned."""
    raw = np.zeros(nbytes + 16, np.uint8)
    lo = -raw.ctypes.data % 16
    return raw[lo:lo + nbytes]


def host_render(images, coefs) -> list:
    """yxh_jpeg_render_host over a batch in one call -> the H x W x 3 arrays.  Destinations are laid
    out with odd gaps and 0xA5 guards, which are checked."""
    from yolox_amd import _native as N
    lib = N.lib()
    descs = (N.JpegImage * len(images))()
    coef_off = ws_off = 0
    dst_off = 5
    for k, (im, cf) in enumerate(zip(images, coefs)):
        C.memmove(C.byref(descs[k]), C.byref(im), C.sizeof(N.JpegImage))
        descs[k].coef_offset, descs[k].ws_offset, descs[k].dst_offset = coef_off, ws_off, dst_off
        coef_off += (cf.nbytes + 15) // 16 * 16
        ws_off += int(lib.yxh_jpeg_workspace_bytes(im.height, im.width, im.sampling))
        dst_off += im.height * im.width * 3 + 7
    coef = aligned(coef_off + 16).view(np.int16)
    for d, cf in zip(descs, coefs):
        coef[d.coef_offset // 2:d.coef_offset // 2 + cf.size] = cf
    ws = aligned(ws_off + 16)
    dst = np.full(dst_off, 0xA5, np.uint8)
    rc = lib.yxh_jpeg_render_host(coef.ctypes.data, descs, len(images), ws.ctypes.data, dst.ctypes.data)
    assert rc == N.OK, lib.yxh_last_error()
    out, covered = [], np.zeros(dst_off, bool)
    for d in descs:
        n = d.height * d.width * 3
        out.append(dst[d.dst_offset:d.dst_offset + n].reshape(d.height, d.width, 3).copy())
        covered[d.dst_offset:d.dst_offset + n] = True
    assert (dst[~covered] == 0xA5).all(), "the host render wrote outside a destination"
    return out
