"""Writes tests/golden/jpeg/: small JPEG fixtures for the baseline decoder and PIL's decoded arrays.

Every file is a PIL re-encoding of a crop of tests/golden/images/000000000009.jpg with seeded
noise added (or of pure noise), at the smallest sizes at which each edge rule of the decoder can
go wrong: a 1-pixel image, odd sizes under 4:2:0 and 4:2:2, a width below one MCU, restart
intervals, content that saturates.  ``decoded.npz`` holds ``np.asarray(Image.open(f).convert("RGB"))``
of every supported file, as the PIL / libjpeg-turbo that ran this script decoded it.

PIL has no switch for 4:1:1 or 4:4:0 sampling, so those two files are a 4:2:0 file whose luma
sampling byte in the frame header is rewritten (0x22 -> 0x41 / 0x12): their scan no longer
matches the header, which is all a probe needs to refuse them.

    python tests/golden/make_golden_jpeg.py
"""
import io
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "jpeg")

# (name, subsampling or "gray", H, W, content, save options)
SUPPORTED = [
    ("420_1x1", "4:2:0", 1, 1, "crop", {}),
    ("420_17x17_q30", "4:2:0", 17, 17, "crop", dict(quality=30)),
    ("420_37x53", "4:2:0", 37, 53, "crop", {}),
    ("420_64x96_q95", "4:2:0", 64, 96, "crop", dict(quality=95)),
    ("420_31x33_q100", "4:2:0", 31, 33, "crop", dict(quality=100)),
    ("420_239x317", "4:2:0", 239, 317, "crop", {}),
    ("420_50x70_rst3", "4:2:0", 50, 70, "crop", dict(restart_marker_blocks=3)),
    ("420_40x56_noise_q100", "4:2:0", 40, 56, "uniform", dict(quality=100)),
    ("422_41x23_q60", "4:2:2", 41, 23, "crop", dict(quality=60)),
    ("422_33x64_rstrow_opt", "4:2:2", 33, 64, "crop", dict(restart_marker_rows=1, optimize=True)),
    ("444_1x1", "4:4:4", 1, 1, "crop", {}),
    ("444_40x56_bw_q20", "4:4:4", 40, 56, "bw", dict(quality=20)),
    ("gray_19x45", "gray", 19, 45, "crop", {}),
]


def content(kind: str, h: int, w: int, rng) -> np.ndarray:
    if kind == "uniform":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "bw":
        return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    with Image.open(os.path.join(HERE, "images", "000000000009.jpg")) as im:
        base = np.asarray(im.convert("RGB"))[100:100 + h, 200:200 + w].astype(np.int32)
    return np.clip(base + rng.integers(-12, 13, base.shape), 0, 255).astype(np.uint8)


def encode(img: np.ndarray, sub: str, **opts) -> bytes:
    buf = io.BytesIO()
    if sub == "gray":
        Image.fromarray(img[:, :, 1]).save(buf, "JPEG", **opts)
    else:
        Image.fromarray(img).save(buf, "JPEG", subsampling=sub, **opts)
    return buf.getvalue()


def patch_luma_sampling(data: bytes, factor: int) -> bytes:
    i = data.index(b"\xff\xc0")
    assert data[i + 9] == 3 and data[i + 11] == 0x22, "expected a 3-component 4:2:0 frame header"
    return data[:i + 11] + bytes([factor]) + data[i + 12:]


def main() -> None:
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20251021)
    decoded = {}
    for name, sub, h, w, kind, opts in SUPPORTED:
        data = encode(content(kind, h, w, rng), sub, **opts)
        with open(os.path.join(OUT, name + ".jpg"), "wb") as f:
            f.write(data)
        with Image.open(io.BytesIO(data)) as im:
            decoded[name] = np.asarray(im.convert("RGB"))
        assert decoded[name].shape == (h, w, 3)
    img = content("crop", 24, 40, rng)
    base = encode(img, "4:2:0")
    unsupported = {
        "progressive_24x40": encode(img, "4:2:0", progressive=True),
        "411_24x40": patch_luma_sampling(base, 0x41),
        "440_24x40": patch_luma_sampling(base, 0x12),
    }
    buf = io.BytesIO()
    Image.fromarray(img).convert("CMYK").save(buf, "JPEG")
    unsupported["cmyk_24x40"] = buf.getvalue()
    for name, data in unsupported.items():
        with open(os.path.join(OUT, name + ".jpg"), "wb") as f:
            f.write(data)
    np.savez_compressed(os.path.join(OUT, "decoded.npz"), **decoded)
    for f in sorted(os.listdir(OUT)):
        print(f"{os.path.getsize(os.path.join(OUT, f)):7d}  {f}")


if __name__ == "__main__":
    main()
