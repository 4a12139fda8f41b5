"""The id space of yxh_wgrad_desc.tile (csrc/wgrad.hip kWgradFamilies): every id from -1 to 33 on three
tiny convs and three operand types returns what it returned before the family table existed, and
every launch that runs computes the weight gradient."""
import pytest

TILE_IDS = range(-1, 34)
# 32 -> 32 channels over one plain source, batch 1, H = W = 16: (k, stride, pad)
SWEEP_CONVS = {"3x3s1": (3, 1, 1), "3x3s2": (3, 2, 1), "1x1": (1, 1, 0)}
CH, HW = 32, 16


def spans(*ranges):
    return [i for lo, hi in ranges for i in range(lo, hi + 1)]


# Recorded by running sweep() on the commit before the table (the nested switch of train.hip's
# wgrad_tile), not derived from the table: {dtype: {conv: (ids that ran, ids refused as unsupported)}};
# every other id is YXH_EINVAL.  bf16 and f16 behave alike.
_F32 = {"3x3s1": (spans((0, 4), (11, 24)), spans((5, 10), (25, 30))),
        "3x3s2": (spans((0, 4), (11, 24)), spans((5, 10), (25, 30))),
        "1x1": (spans((0, 4), (17, 20)), spans((5, 16), (21, 30)))}
_16BIT = {"3x3s1": (spans((0, 10), (25, 30)), spans((11, 24))),
          "3x3s2": (spans((0, 10), (25, 26), (28, 30)), spans((11, 24), (27, 27))),
          "1x1": (spans((0, 10)), spans((11, 30)))}
SWEEP_EXPECTED = {"float32": _F32, "bfloat16": _16BIT, "float16": _16BIT}


def tolerance(dtype_name, tile):
    """test_gpu_train.py's bounds: fp32 1e-4 on tiles 0-16 and 1e-5 on the k-major 17-24; 16-bit 1e-4
    (fp32 accumulation of exact products of the rounded operands: order-only differences)."""
    return 1e-5 if dtype_name == "float32" and 17 <= tile <= 24 else 1e-4


def sweep(dtype_name, conv):
    """{tile: status} of every id on one conv and operand type; every OK result is compared with torch
    fp32 autograd on the way."""
    import torch
    import torch.nn.functional as F
    from test_gpu_train import rel, src, wgrad
    dtype = getattr(torch, dtype_name)
    k, s, p = SWEEP_CONVS[conv]
    oh = (HW + 2 * p - k) // s + 1
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, HW, HW, CH, generator=g).to(dtype)
    dy = torch.randn(1, oh, oh, CH, generator=g).to(dtype)
    wr = torch.zeros(CH, CH, k, k, requires_grad=True)
    F.conv2d(x.float().permute(0, 3, 1, 2), wr, stride=s, padding=p).backward(dy.float().permute(0, 3, 1, 2))
    xd, dyd = x.cuda(), dy.cuda()
    status = {}
    for tile in TILE_IDS:
        try:
            dw = wgrad(dtype, [src(xd)], src(dyd), CH, CH, k, s, p, (HW, HW), (oh, oh), 1, tile=tile)
        except ValueError as e:
            status[tile] = "EINVAL"
            assert "tile" in str(e), (tile, str(e))
            continue
        except NotImplementedError:
            status[tile] = "EUNSUPPORTED"
            continue
        status[tile] = "OK"
        assert rel(dw, wr.grad) < tolerance(dtype_name, tile), (dtype_name, conv, tile)
    return status


@pytest.mark.gpu
def test_every_wgrad_tile_is_routed_as_before():
    for dtype_name, convs in SWEEP_EXPECTED.items():
        for conv, (ok, unsupported) in convs.items():
            status = sweep(dtype_name, conv)
            assert [t for t, s in status.items() if s == "OK"] == ok, (dtype_name, conv)
            assert [t for t, s in status.items() if s == "EUNSUPPORTED"] == unsupported, (dtype_name, conv)
