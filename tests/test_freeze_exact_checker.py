"""tests/freeze_exact.py on the CPU: every case meets the conditions it is judged under, and the judge tells a
right result from the faults a frozen-BatchNorm backward could have."""
import pytest
import torch

import freeze_exact as fe
import train_exact as te


def test_cases_cover_the_issue_grid():
    for dt in te.ALL:
        cs = fe.cases(dt)
        assert {c.C for c in cs} == {1, 8, 20, 24, 80, 256}
        assert {c.M for c in cs} == {1, 35, 400}
        assert {c.act for c in cs} == {te.ACT_SILU, te.ACT_LRELU, te.ACT_NONE}
        assert {c.view for c in cs} == {"dense", "slice", "padded"}
        assert all(c.B > 1 for c in cs if c.M > 1)  # padding rows between images mean something
    # a partial last chunk and rows off the 16-byte grid, in every dtype
    assert any(C % te.EPC[torch.float32] for C in fe.CHANNELS) and any(C % te.EPC[torch.bfloat16] for C in fe.CHANNELS)
    off, idle, _ = te.VIEWS["slice"]
    assert any(((C + idle) * 2) % 16 for C in fe.CHANNELS) and any(((C + idle) * 4) % 16 for C in fe.CHANNELS)


@pytest.mark.parametrize("dt", te.ALL)
def test_references_stay_inside_their_regime(dt):
    """the float64 reference alone: the undefined-side share under AMBIGUOUS_CAP, 16-bit SiLU inside the measured
    range, every bound positive and small against the values"""
    dtype = te.DTYPES[dt]
    for case in fe.cases(dt):
        ops = fe.operands(case, dt)
        ref = fe.act_bwd_reference(ops["y"], ops["dout"], ops["stats"], case.act, dtype)
        assert ref["ambiguous"] <= te.AMBIGUOUS_CAP, (case.id, ref["ambiguous"])
        z = te._z(ops["y"], ops["stats"])[2]
        assert float(z.abs().max()) <= te.FAST_SILU_RANGE, case.id
        assert bool((ref["tol"] > 0).all())
        # not vacuous: against |dout scale| (|act'| <= 1.1) the bound is the store's rounding plus at most
        # G (1 + |z|) <= 32 * 21 fp32 half-ulps
        full = (ops["dout"].to(te.F64) * ops["stats"][2].to(te.F64)).abs() * 1.1 + 1e-30
        rel = (ref["tol"] - te.HALF_SUBNORMAL[dtype]) / full
        assert float(rel.max()) < float(te.U_OUT[dtype] + 1024 * te.U32), (case.id, float(rel.max()))


@pytest.mark.parametrize("dt", te.ALL)
def test_judge_accepts_the_rounded_reference_and_names_faults(dt):
    dtype = te.DTYPES[dt]
    case = next(c for c in fe.cases(dt) if c.C == 20 and c.M == 35 and c.act == te.ACT_SILU and c.view == "slice")
    ops = fe.operands(case, dt)
    ref = fe.act_bwd_reference(ops["y"], ops["dout"], ops["stats"], case.act, dtype)
    good = ref["dx"].to(dtype)
    assert te.judge(good, ref["dx"], ref["tol"]) <= 1.0
    scale = ops["stats"][2].to(te.F64)
    faults = {
        "scale left out": (ref["dx"] / scale).to(dtype),
        "act' left out": (ops["dout"].to(te.F64) * scale).to(dtype),
        "batch-statistics term kept": (ref["dx"] - ref["dx"].mean((0, 1, 2))).to(dtype),
        "last channel unwritten": torch.cat([good[..., :-1], torch.zeros_like(good[..., -1:])], -1),
    }
    for name, got in faults.items():
        with pytest.raises(te.PerElementError):
            te.judge(got, ref["dx"], ref["tol"], label=name)


@pytest.mark.parametrize("C,has_gamma,has_beta", fe.STATS_CASES)
def test_stats_reference(C, has_gamma, has_beta):
    o = fe.stats_operands(C, has_gamma, has_beta)
    assert float(o["rvar"][0]) == 0.0 and (C == 1 or 0.9e-12 < float(o["rvar"][1]) < 1.1e-12)
    want, tol = fe.stats_reference(o)
    # torch's own eval-mode BatchNorm agrees with the table: y = x * scale + shift
    x = torch.randn(3, C, 2, 2, dtype=te.F64)
    ref = torch.nn.functional.batch_norm(
        x, o["rmean"].to(te.F64), o["rvar"].to(te.F64), None if o["gamma"] is None else o["gamma"].to(te.F64),
        None if o["beta"] is None else o["beta"].to(te.F64), False, 0.0, te.f32_value(te.EPS))
    got = x * want[2].view(1, C, 1, 1) + want[3].view(1, C, 1, 1)
    assert float((got - ref).abs().max()) < 1e-9
    assert abs(float(want[1][0]) - te.f32_value(te.EPS) ** -0.5) < 1e-9
    # the fp32 evaluation in the kernel's operation order sits inside the bars; a float sqrt of a float sum need not
    f32 = torch.float32
    invstd = (1 / torch.sqrt(o["rvar"].to(te.F64) + te.f32_value(te.EPS))).to(f32)
    scale = (o["gamma"] if has_gamma else torch.ones(C)) * invstd
    shift = (o["beta"] if has_beta else torch.zeros(C)) - o["rmean"] * scale
    got = torch.stack([o["rmean"], invstd, scale, shift])
    assert te.judge(got[1:], want[1:], tol[1:]) <= 1.0
    with pytest.raises(te.PerElementError):
        te.judge(got[1:] * (1 + 2.0 ** -20), want[1:], tol[1:])
