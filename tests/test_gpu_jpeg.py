"""JPEG decoding with the render on the GPU: yxh_jpeg_render_batch against PIL and against the host
restatement byte for byte (one ragged launch, guard bytes, odd destination offsets, a second launch,
a captured replay), then the two users: Yolox.stream over paths / bytes / arrays, and the
StreamedImages pool with the device path on and off."""
import ctypes as C
import io
import json
import os
import shutil

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_cases as J

pytestmark = pytest.mark.gpu

EVERY = {**J.SUPPORTED, **J.GOLDEN_IMAGES}
SIZE = (128, 128)
GUARD = 0xA5


# ------------------------------------------------------------------ the kernels alone
class Batch:
    """Every supported fixture, entropy-decoded once, laid out for one yxh_jpeg_render_batch call:
    destinations start at byte 5 and are 7 bytes apart, so most offsets are no multiple of 4, and
    everything between and around them is 0xA5."""

    def __init__(self):
        from yolox_amd import _native as N
        lib = N.lib()
        self.names = list(EVERY)
        images, coefs = [], []
        for name in self.names:
            rc, _, image, coef, intact = J.host_decode(J.fixture_bytes(name))
            assert rc == N.OK and intact, name
            images.append(image)
            coefs.append(coef)
        self.host = J.host_render(images, coefs)
        self.descs = (N.JpegImage * len(images))()
        coef_off = ws_off = 0
        dst_off = 5
        for k, (im, cf) in enumerate(zip(images, coefs)):
            C.memmove(C.byref(self.descs[k]), C.byref(im), C.sizeof(N.JpegImage))
            d = self.descs[k]
            d.coef_offset, d.ws_offset, d.dst_offset = coef_off, ws_off, dst_off
            coef_off += (cf.nbytes + 15) // 16 * 16
            ws_off += int(lib.yxh_jpeg_workspace_bytes(im.height, im.width, im.sampling))
            dst_off += im.height * im.width * 3 + 7
        assert sum(d.dst_offset % 4 != 0 for d in self.descs) >= len(images) // 2
        coef = np.zeros(coef_off // 2, np.int16)
        for d, cf in zip(self.descs, coefs):
            coef[d.coef_offset // 2:d.coef_offset // 2 + cf.size] = cf
        dev = torch.device("cuda")
        self.coef = torch.from_numpy(coef).to(dev)
        self.desc = torch.from_numpy(np.frombuffer(self.descs, np.uint8).copy()).to(dev)
        self.ws = torch.zeros(ws_off, dtype=torch.uint8, device=dev)
        self.dst_bytes = dst_off + 64
        self.covered = np.zeros(self.dst_bytes, bool)
        for d in self.descs:
            self.covered[d.dst_offset:d.dst_offset + d.height * d.width * 3] = True

    def fresh_dst(self):
        return torch.full((self.dst_bytes,), GUARD, dtype=torch.uint8, device="cuda")

    def launch(self, dst, stream=None):
        from yolox_amd import _native as N
        N.check(N.lib().yxh_jpeg_render_batch(self.coef.data_ptr(), self.desc.data_ptr(), len(self.names),
                                              self.ws.data_ptr(), dst.data_ptr(),
                                              N.stream_ptr(dst.device) if stream is None else stream), "render")

    def split(self, dst):
        flat = dst.cpu().numpy()
        assert (flat[~self.covered] == GUARD).all(), "a byte outside every destination was written"
        return [flat[d.dst_offset:d.dst_offset + d.height * d.width * 3].reshape(d.height, d.width, 3)
                for d in self.descs]


@pytest.fixture(scope="module")
def batch():
    return Batch()


@pytest.fixture(scope="module")
def first_launch(batch):
    dst = batch.fresh_dst()
    batch.launch(dst)
    torch.cuda.synchronize()
    return dst


def test_ragged_batch_equals_pil_and_host_render(batch, first_launch):
    got = batch.split(first_launch)
    recorded = J.recorded()
    for name, g, h in zip(batch.names, got, batch.host):
        live = J.pil_rgb(J.fixture_bytes(name))
        assert g.shape == live.shape
        assert np.array_equal(g, live), f"{name}: {int((g != live).sum())} bytes differ from PIL"
        assert np.array_equal(g, h), f"{name}: differs from yxh_jpeg_render_host"
        if name in recorded:
            assert np.array_equal(g, recorded[name]), f"{name}: differs from the recorded decode"


def test_second_launch_into_the_same_buffers(batch, first_launch):
    before = first_launch.clone()
    batch.launch(first_launch)
    torch.cuda.synchronize()
    assert torch.equal(first_launch, before)


def test_captured_replay_equals_the_eager_call(batch, first_launch):
    dst = batch.fresh_dst()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        batch.launch(dst)
    dst.fill_(GUARD)
    batch.ws.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(dst, first_launch)


def test_a_bad_descriptor_is_skipped_whole(batch):
    """Impossible sizes or a misaligned coefficient offset: that image writes nothing, the others do."""
    from yolox_amd import _native as N
    descs = (N.JpegImage * 3)()
    for k in range(3):
        C.memmove(C.byref(descs[k]), C.byref(batch.descs[1]), C.sizeof(N.JpegImage))  # 420_17x17_q30
    descs[0].coef_offset += 2
    descs[1].sampling = J.GRAY  # three components cannot be grayscale
    n = 17 * 17 * 3
    for k in range(3):
        descs[k].dst_offset = 3 + k * (n + 9)
    desc = torch.from_numpy(np.frombuffer(descs, np.uint8).copy()).to("cuda")
    dst = torch.full((3 * (n + 9) + 16,), GUARD, dtype=torch.uint8, device="cuda")
    N.check(N.lib().yxh_jpeg_render_batch(batch.coef.data_ptr(), desc.data_ptr(), 3, batch.ws.data_ptr(),
                                          dst.data_ptr(), N.stream_ptr(dst.device)), "render")
    flat = dst.cpu().numpy()
    lo = descs[2].dst_offset
    assert np.array_equal(flat[lo:lo + n].reshape(17, 17, 3), J.recorded()["420_17x17_q30"])
    flat[lo:lo + n] = GUARD
    assert (flat == GUARD).all()


# ------------------------------------------------------------------ Yolox.stream
@pytest.fixture(scope="module")
def yolox():
    from yolox_amd.config import named_config
    from yolox_amd.models import Yolox, YoloxModule, YoloxProcessor
    cfg = named_config("yolox_s")
    cfg.test_size = SIZE
    return Yolox(YoloxModule.synthetic("yolox_s", seed=0, device="cuda", dtype=torch.bfloat16), YoloxProcessor(cfg))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The three golden JPEGs (4:4:4), a 4:2:0 re-encoding of each, a PNG and a progressive JPEG."""
    root = tmp_path_factory.mktemp("jpeg_stream")
    paths = [J.fixture_path(n) for n in J.GOLDEN_IMAGES]
    for n in J.GOLDEN_IMAGES:
        with Image.open(J.fixture_path(n)) as im:
            p = str(root / f"{n}_420.jpg")
            im.save(p, "JPEG", subsampling="4:2:0", quality=85)
            paths.append(p)
    with Image.open(paths[0]) as im:
        small = im.resize((160, 120))
        small.save(str(root / "a.png"))
        small.save(str(root / "prog.jpg"), "JPEG", progressive=True)
    for p in paths[3:]:
        with open(p, "rb") as f:
            info = J.host_decode(f.read())[1]
        assert info.sampling == J.S420
    return dict(jpeg=paths, png=str(root / "a.png"), progressive=str(root / "prog.jpg"))


def read(path):
    with open(path, "rb") as f:
        return f.read()


def pil_array(path):
    with Image.open(path) as im:
        return np.asarray(im)


@pytest.mark.parametrize("batch_size", [1, 4])
def test_stream_paths_bytes_and_arrays_agree(yolox, files, monkeypatch, batch_size):
    monkeypatch.setenv("YOLOX_AMD_JPEG", "1")
    paths = files["jpeg"]
    yolox.jpeg.reset_stats()
    from_arrays = list(yolox.stream([pil_array(p) for p in paths], threshold=0.01, batch_size=batch_size))
    assert yolox.jpeg.stats == {"device": 0, "pil": 0, "reasons": {}}  # arrays are no files
    from_paths = list(yolox.stream(paths, threshold=0.01, batch_size=batch_size))
    assert yolox.jpeg.stats == {"device": 6, "pil": 0, "reasons": {}}
    kinds = (bytes, bytearray, memoryview, bytes, bytearray, memoryview)
    from_bytes = list(yolox.stream([k(read(p)) for k, p in zip(kinds, paths)], threshold=0.01, batch_size=batch_size))
    assert yolox.jpeg.stats == {"device": 12, "pil": 0, "reasons": {}}
    assert sum(len(d["scores"]) for d in from_arrays) > 0
    for a, p, b in zip(from_arrays, from_paths, from_bytes):
        for key in ("bboxes", "scores", "labels"):
            assert a[key] == p[key] == b[key], key
    # and the switch: the same call through PIL
    monkeypatch.setenv("YOLOX_AMD_JPEG", "0")
    yolox.jpeg.reset_stats()
    assert list(yolox.stream(paths, threshold=0.01, batch_size=batch_size)) == from_arrays
    assert yolox.jpeg.stats == {"device": 0, "pil": 6, "reasons": {"device path off": 6}}


def test_stream_mixes_kinds_inside_a_batch(yolox, files, monkeypatch):
    monkeypatch.setenv("YOLOX_AMD_JPEG", "1")
    j = files["jpeg"]
    rng = np.random.default_rng(3)
    noise = rng.integers(0, 256, (97, 131, 3), dtype=np.uint8)
    inputs = [j[0], read(files["png"]), read(j[4]), files["progressive"], noise, j[5], Image.open(j[1]), j[2]]
    plain = [pil_array(j[0]), pil_array(files["png"]), pil_array(j[4]), pil_array(files["progressive"]), noise,
             pil_array(j[5]), pil_array(j[1]), pil_array(j[2])]
    want = list(yolox.stream(plain, threshold=0.01, batch_size=4))
    yolox.jpeg.reset_stats()
    got = list(yolox.stream(inputs, threshold=0.01, batch_size=4))
    assert got == want
    s = yolox.jpeg.stats
    assert s["device"] == 4 and s["pil"] == 2, s
    assert s["reasons"] == {"not a JPEG": 1, "jpeg: progressive": 1}


def test_stream_keeps_its_errors(yolox, monkeypatch, tmp_path):
    monkeypatch.setenv("YOLOX_AMD_JPEG", "1")
    with pytest.raises(FileNotFoundError):
        list(yolox.stream([str(tmp_path / "missing.jpg")], batch_size=4))
    with pytest.raises(ValueError, match="H x W x 3"):  # grayscale stays PIL's 2-D array, refused as before
        list(yolox.stream([J.fixture_path("gray_19x45")], batch_size=4))
    # a scan cut short: the probe takes it, the entropy decoder refuses it, PIL decides as it always did
    data = read(J.fixture_path("420_64x96_q95"))[:-300]
    try:
        want = list(yolox.stream([np.asarray(Image.open(io.BytesIO(data)))], threshold=0.01, batch_size=4))
    except OSError as e:
        with pytest.raises(OSError, match=str(e)[:20]):
            list(yolox.stream([data], threshold=0.01, batch_size=4))
    else:
        assert list(yolox.stream([data], threshold=0.01, batch_size=4)) == want
    assert list(yolox.stream([J.fixture_path("420_64x96_q95")], threshold=0.01, batch_size=4))  # still serving


# ------------------------------------------------------------------ the streamed COCO pool
def make_dataset(root, wrong_size=None):
    """A COCO-layout directory: golden JPEGs, small fixtures of every sampling (grayscale too), a
    PNG and a JPEG with EXIF orientation 6, which decodes transposed."""
    split = os.path.join(root, "train2017")
    os.makedirs(split, exist_ok=True)
    os.makedirs(os.path.join(root, "annotations"), exist_ok=True)
    files = []
    for n in ["000000000001", "000000000016", "420_239x317", "422_41x23_q60", "444_40x56_bw_q20", "gray_19x45",
              "420_50x70_rst3"]:
        shutil.copy(J.fixture_path(n), os.path.join(split, n + ".jpg"))
        h, w = EVERY[n][:2]
        files.append((n + ".jpg", h, w))
    rng = np.random.default_rng(1)
    Image.fromarray(rng.integers(0, 256, (50, 30, 3), dtype=np.uint8)).save(os.path.join(split, "p.png"))
    files.append(("p.png", 50, 30))
    exif = Image.Exif()
    exif[0x0112] = 6
    with Image.open(J.fixture_path("420_64x96_q95")) as im:
        im.save(os.path.join(split, "turned.jpg"), "JPEG", exif=exif, subsampling="4:2:0")
    files.append(("turned.jpg", 96, 64))  # 64 x 96 stored, 96 x 64 once the orientation is applied
    images, anns = [], []
    for k, (name, h, w) in enumerate(files):
        if wrong_size == name:
            h += 1
        images.append(dict(id=10 + k, file_name=name, height=h, width=w))
        anns.append(dict(id=k + 1, image_id=10 + k, bbox=[1.0, 1.0, w / 2, h / 2], area=w * h / 4.0, iscrowd=0,
                         category_id=1 + k))
    with open(os.path.join(root, "annotations", "instances_train2017.json"), "w") as f:
        json.dump(dict(images=images, annotations=anns, categories=[dict(id=i, name=f"c{i}") for i in range(1, 81)]), f)
    return root


def filled_pool(root, setting, monkeypatch):
    from yolox_amd.data import CocoDataset, StreamedImages
    monkeypatch.setenv("YOLOX_AMD_JPEG", setting)
    ds = CocoDataset(root, img_size=(64, 64))
    pool = StreamedImages(ds, capacity_slots=len(ds), workers=4)
    pool.ensure(range(len(ds)))
    torch.cuda.synchronize()
    data = pool.pool.cpu().numpy()
    out = []
    for i in range(len(ds)):
        rh, rw = (int(v) for v in pool.shapes[i])
        out.append(data[pool.offsets[i]:pool.offsets[i] + rh * rw * 3].copy())
    return pool, out


def test_streamed_pool_holds_the_same_bytes_either_way(tmp_path, monkeypatch):
    root = make_dataset(str(tmp_path))
    off, want = filled_pool(root, "0", monkeypatch)
    on, got = filled_pool(root, "1", monkeypatch)
    assert len(want) == 9
    for k, (a, b) in enumerate(zip(want, got)):
        assert a.size > 0 and np.array_equal(a, b), f"image {k}"
    assert on.stats["decodes"] == off.stats["decodes"] == 9
    s = on.jpeg.stats
    assert s["device"] == 7 and s["pil"] == 2, s  # grayscale on the device; the PNG and the turned file to PIL
    assert s["reasons"] == {"not a JPEG": 1, "EXIF orientation": 1}
    assert off.jpeg.stats["device"] == 0


@pytest.mark.parametrize("setting", ["0", "1"])
def test_size_mismatch_against_the_json_raises_as_before(tmp_path, monkeypatch, setting):
    from yolox_amd.data import CocoDataset, StreamedImages
    root = make_dataset(str(tmp_path), wrong_size="422_41x23_q60.jpg")
    monkeypatch.setenv("YOLOX_AMD_JPEG", setting)
    ds = CocoDataset(root, img_size=(64, 64))
    pool = StreamedImages(ds, capacity_slots=len(ds), workers=4)
    with pytest.raises(ValueError, match=r"422_41x23_q60\.jpg decodes to 41x23, the annotation file says 42x23"):
        pool.ensure(range(len(ds)))
    assert 3 not in pool.table  # the failed round's images are dropped, as before
    pool.ensure([0, 1])  # and the pool still serves
    torch.cuda.synchronize()
    assert (pool.offsets[[0, 1]] >= 0).all()
