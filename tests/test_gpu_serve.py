"""The serving pipeline on the GPU: yxh_detections_pack alone against numpy, and Yolox.stream /
yolox_amd.serve.Pipeline end to end against the CPU oracle (not against the code under test) and
against Yolox.__call__.  yolox_s synthetic weights at test_size 128 x 128 (A = 336), batches of 2."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FILES = [os.path.join(GOLDEN, "images", f"{n}.jpg") for n in ("000000000001", "000000000009", "000000000016")]
SIZE = (128, 128)
EMPTY = {"bboxes": [], "scores": [], "labels": []}
CANARY = 0x5AC3A55A


# ------------------------------------------------------------------ the kernel alone
def pack(det, counts, ratios, n_valid, capacity, slack=16):
    """Run yxh_detections_pack; returns (offsets [B+1], the whole output buffer as uint32 [capacity + slack, 8])."""
    from yolox_amd import _native as N
    B, A, _ = det.shape
    dev = torch.device("cuda")
    d = torch.from_numpy(det).to(dev)
    c = torch.from_numpy(np.asarray(counts, np.int32)).to(dev)
    r = torch.from_numpy(np.asarray(ratios, np.float32)).to(dev)
    rows = torch.from_numpy(np.full((capacity + slack, 8), CANARY, np.uint32).view(np.int32)).to(dev)
    offs = torch.full((B + 1,), -7, dtype=torch.int32, device=dev)
    N.check(N.lib().yxh_detections_pack(d.data_ptr(), c.data_ptr(), B, A, n_valid, r.data_ptr(), rows.data_ptr(),
                                        capacity, offs.data_ptr(), N.stream_ptr(dev)), "detections_pack")
    torch.cuda.synchronize()
    return offs.cpu().numpy(), rows.cpu().numpy().view(np.uint32)


def expected_rows(det, counts, ratios, n_valid):
    out = []
    for b in range(n_valid):
        n = counts[b]
        rec = np.zeros((n, 8), np.float32)
        rec[:, :4] = det[b, :n, :4] / np.float32(ratios[b])
        rec[:, 4:6] = det[b, :n, 4:6]
        rec.view(np.int32)[:, 6] = det[b, :n, 6].astype(np.int32)
        rec.view(np.int32)[:, 7] = b
        out.append(rec)
    return np.concatenate(out) if out else np.zeros((0, 8), np.float32)


@pytest.fixture(scope="module")
def kernel_case():
    rng = np.random.default_rng(11)
    B, A = 3, 70
    counts = [0, 70, 5]
    ratios = np.array([1.0, 0.832, 1 / 3], np.float32)
    det = np.full((B, A, 7), np.nan, np.float32)
    for b, n in enumerate(counts):
        det[b, :n, :4] = rng.uniform(-30, 700, (n, 4))
        det[b, :n, 4:6] = rng.uniform(0, 1, (n, 2))
        det[b, :n, 6] = rng.integers(0, 80, n)
    # signed zero, denormals and values whose quotient is denormal: the divide keeps them
    det[1, 0, :4] = [-0.0, 1e-45, -3e-39, 1.1754944e-38]
    det[2, 4, :4] = [1e-38, -1e-40, 5e-39, 1e38]
    return det, counts, ratios


@pytest.mark.parametrize("n_valid,capacity", [(3, 100), (2, 100), (3, 8)])
def test_detections_pack_against_numpy(kernel_case, n_valid, capacity):
    det, counts, ratios = kernel_case
    offs, buf = pack(det, counts, ratios, n_valid, capacity)
    eff = [c if b < n_valid else 0 for b, c in enumerate(counts)]
    assert offs.tolist() == np.concatenate([[0], np.cumsum(eff)]).tolist()  # the total too, past the capacity
    want = expected_rows(det, counts, ratios, n_valid)
    total = len(want)
    assert total == (75 if n_valid == 3 else 70)
    written = min(total, capacity)
    assert buf[:written].tobytes() == want[:written].tobytes()
    assert not np.isnan(buf[:written].view(np.float32)[:, :6]).any()
    assert (buf[written:] == CANARY).all()  # nothing at or beyond capacity_rows, nothing beyond the total


def test_detections_pack_single_row():
    det = np.array([[[3.0, 4.5, 100.0, 7.25, 0.5, 0.75, 79.0]]], np.float32)
    offs, buf = pack(det, [1], [0.4], 1, 1)
    assert offs.tolist() == [0, 1]
    assert buf[:1].tobytes() == expected_rows(det, [1], np.array([0.4], np.float32), 1).tobytes()
    assert (buf[1:] == CANARY).all()


# ------------------------------------------------------------------ end to end
def inputs5():
    rng = np.random.default_rng(21)
    return FILES + [rng.integers(0, 256, (97, 131, 3), dtype=np.uint8),
                    rng.integers(0, 256, (201, 77, 3), dtype=np.uint8)]


def arrays5():
    from PIL import Image
    return [np.asarray(Image.open(f)) for f in FILES] + inputs5()[3:]


def make_api(dtype, seed=0):
    from yolox_amd.config import named_config
    from yolox_amd.models import Yolox, YoloxModule, YoloxProcessor
    cfg = named_config("yolox_s")
    cfg.test_size = SIZE
    return Yolox(YoloxModule.synthetic("yolox_s", seed=seed, device="cuda", dtype=dtype), YoloxProcessor(cfg))


@pytest.fixture(scope="module")
def apis():
    return {"bf16": make_api(torch.bfloat16), "fp32": make_api(torch.float32)}


@pytest.fixture(scope="module")
def oracle_results(apis, oracle):
    """(dtype, threshold) -> the five Detections the oracle computes from the eager forward of each
    letterboxed pair; the short last batch is [img4, img3]: slot 1 still holds batch 1's image."""
    cache = {}

    def get(dtype, thr):
        if (dtype, thr) not in cache:
            yolox = apis[dtype]
            arrs = arrays5()
            res = []
            for pair, keep in (((0, 1), 2), ((2, 3), 2), ((4, 3), 1)):
                batch = yolox.processor.images_to_device([arrs[i] for i in pair], "u8_nhwc")
                host = yolox.module.forward_nhwc(batch).cpu().numpy().copy()
                rows = oracle.postprocess(host, 80, thr, 0.65)
                res += [oracle.detections(rows[j], arrs[i].shape[:2], SIZE) for j, i in enumerate(pair)][:keep]
            cache[(dtype, thr)] = res
        return cache[(dtype, thr)]

    return get


def call_chunks(yolox, thr):
    """The parent's public path: Yolox.__call__ per chunk of 2 (PIL images for the arrays)."""
    from PIL import Image
    ins = FILES + [Image.fromarray(a) for a in inputs5()[3:]]
    return [d for i in range(0, 5, 2) for d in yolox(ins[i:i + 2], threshold=thr)]


@pytest.mark.parametrize("thr", [0.3, 0.01])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_stream_equals_oracle_and_call(apis, oracle_results, dtype, thr):
    yolox = apis[dtype]
    got = list(yolox.stream(inputs5(), threshold=thr, batch_size=2))
    want = oracle_results(dtype, thr)
    print(f"{dtype} thr {thr}: detections per image {[len(d['labels']) for d in want]}")
    assert len(got) == 5
    assert got == want
    assert yolox.detect(inputs5(), threshold=thr, batch_size=2) == want
    assert got == call_chunks(yolox, thr)
    pipe = yolox.pipeline(2)
    assert (pipe.scores is not None) == (dtype == "bf16")  # records on / the row-filter fallback


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_overflow_path_fetches_the_remainder(apis, oracle_results, dtype):
    from yolox_amd.serve import Pipeline
    yolox = apis[dtype]
    want = oracle_results(dtype, 0.01)
    per_batch = [sum(len(d["labels"]) for d in want[i:i + 2]) for i in range(0, 5, 2)]
    print(f"{dtype}: detections per batch {per_batch}")
    assert max(per_batch) > 4  # the second copy is taken
    pipe = Pipeline(yolox.module, yolox.processor, 2, capacity_rows=4)
    assert pipe.capacity == 4
    assert list(pipe.run(inputs5(), 0.01)) == want
    assert list(yolox.stream(inputs5(), threshold=0.01, batch_size=2)) == want  # ample capacity


def test_zero_detections_and_empty_input(apis):
    yolox = apis["bf16"]
    got = list(yolox.stream(inputs5(), threshold=0.999, batch_size=2))
    assert got == call_chunks(yolox, 0.999)
    empties = [g for g in got if not g["labels"]]
    assert empties and all(g == EMPTY for g in empties)
    assert list(yolox.stream([], threshold=0.3, batch_size=2)) == []
    assert list(yolox.stream(iter(()), threshold=0.3, batch_size=2)) == []


def test_stream_is_lazy(apis, oracle_results):
    yolox = apis["bf16"]
    ins = inputs5() + inputs5()[:2]
    pulled = []

    def counting():
        for i, im in enumerate(ins):
            pulled.append(i)
            yield im

    g = yolox.stream(counting(), threshold=0.3, batch_size=2)
    first = next(g)
    assert len(pulled) <= 4
    assert first == oracle_results("bf16", 0.3)[0]
    rest = list(g)
    assert len(rest) == 6 and len(pulled) == 7


def test_error_recovery_and_one_stream_at_a_time(apis, oracle_results):
    from PIL import Image
    yolox = apis["bf16"]
    want = oracle_results("bf16", 0.3)
    gray = Image.fromarray(np.zeros((64, 64), np.uint8), mode="L")
    rgba = np.zeros((64, 64, 4), np.uint8)
    for bad in (gray, rgba, np.zeros((0, 5, 3), np.uint8)):
        with pytest.raises(ValueError):
            list(yolox.stream(inputs5()[:3] + [bad], threshold=0.3, batch_size=2))
        assert list(yolox.stream(inputs5(), threshold=0.3, batch_size=2)) == want
    g = yolox.stream(inputs5(), threshold=0.3, batch_size=2)
    assert next(g) == want[0]
    with pytest.raises(RuntimeError):
        next(yolox.stream(inputs5(), threshold=0.3, batch_size=2))
    assert next(g) == want[1]  # the first stream is unharmed
    g.close()  # abandoned with a batch in flight: released
    assert list(yolox.stream(inputs5(), threshold=0.3, batch_size=2)) == want


def test_stream_sees_new_weights_after_load_state_dict():
    yolox, other = make_api(torch.float32, seed=0), make_api(torch.float32, seed=1)
    before = list(yolox.stream(inputs5(), threshold=0.01, batch_size=2))
    yolox.module.load_state_dict(other.module.state_dict())
    after = list(yolox.stream(inputs5(), threshold=0.01, batch_size=2))
    assert after == call_chunks(other, 0.01)
    assert after != before


def test_pipeline_is_rebuilt_when_the_module_changes_dtype():
    yolox = make_api(torch.float32)
    a = yolox.pipeline(2)
    assert yolox.pipeline(2) is a and a.scores is None
    yolox.module.to(torch.bfloat16)
    b = yolox.pipeline(2)
    assert b is not a and b.scores is not None and b.dtype == torch.bfloat16
    assert list(yolox.stream(inputs5(), threshold=0.3, batch_size=2)) == call_chunks(yolox, 0.3)
