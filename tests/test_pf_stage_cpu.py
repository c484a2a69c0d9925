"""CPU: the case table, inputs, references and checker of the prefill stage tests (pf_stage_cases.py,
pf_stage_ref.py) hold together without a GPU.

* every case names a path that prefill.hip's own choices, restated in pf_stage_cases.expect, give it,
  and the table reaches every edge the stages have;
* every case's inputs have the properties the case is there for (a clip that bites on both signs, a lo
  half that is not zero, GELU arguments past the exp2 overflow in both signs, a vocab tile whose whole
  contribution underflows, the row maximum outside the target's tile and twice in the row ...);
* an honest f32 evaluation in the kernels' own order (pf_stage_ref.emulate) passes check at every case:
  exact cases bit for bit, float cases five times under each bar; the bars that are measured here
  (LP_ATOL, PSUM_REL, RECON_REL) are 5 x the worst error of that evaluation, and LP_ATOL <= 1e-4 nats;
* act_fast's own formulas in f32 meet the f16 bar five times over;
* every deliberately wrong kernel of pf_stage_ref.WRONG is rejected by check at the cases meant for
  it: the standing evidence that the GPU test fails on a subtly wrong kernel."""
import numpy as np
import pytest

import pf_stage_cases as C
import pf_stage_ref as R

MARGIN = 5.0


def test_every_case_names_the_path_the_launcher_gives_it():
    for c in C.CASES:
        assert c.want, c
        assert not C.reaches(c, C.expect(c)), f"{c}: {C.reaches(c, C.expect(c))}"


def test_table_reaches_every_edge():
    ex = {c.name: C.expect(c) for c in C.CASES}
    by = lambda st: [c for c in C.CASES if c.stage == st]
    assert {ex[c.name]["norm_nv"] for c in by(C.NORM)} == {0, 4, 8, 12, 16, 24, 32}
    assert any(c.dim > 32 * 256 for c in by(C.NORM)) and any("wnorm:0" in c.forms for c in by(C.NORM))
    assert {c.split for c in by(C.NORM)} == {0, 1} and all(c.T == 5 for c in by(C.NORM))
    q = by(C.QKV)
    assert {c.head_dim for c in q} == {64, 128} and {c.T for c in q} >= {1, 17, 64, 65, 256, 257}
    assert all(c.pos0 > 0 for c in q) and {c.bias for c in q} == {False, True}
    for fam in ("exact", "float"):
        qf = [c for c in q if c.family == fam]
        assert any(ex[c.name]["skinny"] for c in qf) and any(ex[c.name]["two_depth"] for c in qf)
        assert any(c.split and ex[c.name]["n_gemm"] == 1 for c in qf)
        for p8 in (0, 3):
            assert {ex[c.name]["bn"] for c in qf if ex[c.name]["n_gemm"] == 2 and (
                ex[c.name]["eight_phase"] == p8 or ex[c.name]["bn"][0] == 320)} >= {(b, b) for b in (128, 192, 256, 320)}
        assert {ex[c.name]["bn"][0] for c in qf if c.split} == {128, 192, 256, 320}
        assert any(c.split and c.q_dim == 384 and c.kv_dim == 128 for c in qf)
        assert any(c.kv_dim == 128 and ex[c.name]["bn"] == (256, 256) for c in qf)
        # the skinny reduce's partial counts: 1, 2 or 3, exactly 4, above 4 and no multiple of 4, 8
        counts = {ex[c.name]["ks"] for c in C.CASES if c.family == fam and ex[c.name]["skinny"]} | {
            ex[c.name]["ks2"] for c in qf if ex[c.name]["skinny"]}
        assert counts >= {1, 2, 3, 4, 5, 6, 8}
        assert {c.T for c in C.CASES if c.family == fam and ex[c.name]["skinny"]} >= {1, 16, 17, 33, 64}
        r = [c for c in by(C.RESIDUAL) if c.family == fam]
        assert {c.scale for c in r} == {1.0, 8.0} and {c.kind for c in r} == {C.PF_WO, C.PF_W2}
        assert any(ex[c.name]["persistent"] for c in r) and {(c.k // 64) % 2 for c in r if not ex[c.name]["skinny"]} == {0, 1}
        lp = [c for c in by(C.LOGPROB) if c.family == fam]
        assert {c.T for c in lp} >= {1, 17, 256, 257, 513}
        assert {(ex[c.name]["bn"][0], ex[c.name]["eight_phase"]) for c in lp} >= {
            (128, 0), (128, 1), (192, 0), (192, 1), (256, 0), (256, 1), (320, 0)}
        assert any(ex[c.name]["persistent"] and c.T > 256 for c in lp) and any(c.vocab // ex[c.name]["bn"][0] > 256 for c in lp)
    for c in C.CASES:  # skl:1 and skl:0 twins must give the same bits: they share the reference
        if "skl:0" in c.forms:
            assert ex[c.name]["skinny"], c
    g = by(C.GLU)
    assert {c.act for c in g} == {C.GELU, C.SILU} and {c.hscale for c in g} == {1.0, 0.0625}
    assert {ex[c.name]["bn"][0] for c in g if not ex[c.name]["skinny"]} == {128, 256} and {c.split for c in g} == {0, 1}
    assert any(ex[c.name]["skinny"] for c in g)


def test_inputs_have_the_properties_the_cases_are_there_for():
    for c in C.CASES:
        i, r = R.inputs(c), R.reference(c)
        if c.stage == C.QKV:
            raw = np.concatenate([(i.a_hi + i.a_lo if c.split else i.a_hi) @ i.w[:c.q_dim].T,
                                  (i.a_hi + i.a_lo) @ i.w[c.q_dim:].T], axis=1) + i.bias
            assert (raw > i.clip).any() and (raw < -i.clip).any(), f"{c}: the clip must bite on both signs"
            assert np.count_nonzero(i.a_lo) > i.a_lo.size // 2 and np.abs(r["q"]).max() < 65504
            if c.exact:  # the reference is exactly representable: any f32 order gives it
                for k in ("q", "k", "v"):
                    if not (c.split and k == "q"):
                        assert np.array_equal(R.h16(r[k]).astype(np.float64), r[k]), (c, k)
            if getattr(c, "wide", False):
                assert (np.abs(r["q"]) > 2048).any()
        if c.stage == C.GLU:
            if c.act == C.GELU:
                y = 0.797885 * (r["x1"] + 0.044715 * r["x1"] ** 3)
                assert (2.8853900817779268 * y > 130).any() and (2.8853900817779268 * y < -160).any(), c
            assert r["over"] == bool(getattr(c, "over", False)), (c, r["vmax"])
            assert abs(r["vmax"] * c.hscale / 65504.0 - 1.0) > 0.01
        if c.stage == C.LOGPROB:
            bn, tn = R.lp_wave_cols(c)
            lg, tg = r["logits"], i.targets
            assert np.abs(lg).max() < 120, c
            if c.T > 1:
                assert tg[-1] == -1
            if c.exact:
                assert np.array_equal(lg, np.round(lg)) and (lg.max(axis=1) == R.LP_MAX).all()
                assert ((lg == R.LP_MAX).sum(axis=1) >= 2).all()  # the maximum twice, in two tiles
                under = lg[:, i.under * bn:(i.under + 1) * bn]
                assert (np.exp2((under.max(axis=1) - R.LP_MAX) * 1.4426950408889634) == 0).all() or \
                    (under.max(axis=1) - R.LP_MAX < -103.3).all()
                assert (np.abs(np.diff(r["pmax"], axis=1)) > 8).mean() > 0.5  # neighbours differ widely in maximum
            assert {int(t) for t in tg[:min(c.T, 10)]} <= {bn - 1, 0, bn % c.vocab, tn - 1, tn, c.vocab - 1, -1,
                                                           i.under * bn + 7, i.maxcols[0], 2 * bn - 1, bn - 2}
            assert tg[0] == bn - 1 and ((tg >= 0) & (tg // bn != np.argmax(r["pmax"], axis=1))).any() or c.T == 1


def test_f32_evaluation_meets_every_bar_with_margin():
    """emulate(): exact cases give the reference's bits; float cases stay MARGIN times under each bar. The
    measured bars are MARGIN x this evaluation's worst error (rounded up), LP_ATOL at or under 1e-4."""
    worst = {}
    lp_err = ps_err = rec_err = 0.0
    for c in C.CASES:
        got = R.emulate(c)
        ok, val = R.check(c, got)
        assert ok, c
        if c.exact:
            assert val is True, c
        else:
            assert val * MARGIN <= 1.0, f"{c}: {val:.3f} bars"
            worst[c.stage] = max(worst.get(c.stage, 0.0), val)
        i, r, T = R.inputs(c), R.reference(c), c.T
        if c.stage == C.LOGPROB:
            nt = c.vocab // R.lp_wave_cols(c)[0]
            has = r["has"]
            lp_err = max(lp_err, float(np.abs(got["lp"][has] - r["lp"][has]).max()) if has.any() else 0.0)
            ps = got["psum"][:T * nt].reshape(T, nt).astype(np.float64)
            ps_err = max(ps_err, float((np.abs(ps - r["psum"]) / r["psum"]).max()))
        if c.stage == C.NORM and c.split and not c.exact:
            xn = got["xn"][:T].view(np.float16).astype(np.float64)
            rec = xn[:, :c.dim] + xn[:, c.dim:]
            rec_err = max(rec_err, float((np.abs(rec - r["y"]) / np.abs(r["y"]).max(axis=1, keepdims=True)).max()))
    print(f"measured: lp {lp_err:.3g} nats, psum {ps_err:.3g} rel, norm hi + lo {rec_err:.3g} of the row max; "
          f"worst float case per stage, bars: { {C.STAGE_NAMES[k]: round(v, 4) for k, v in worst.items()} }")
    assert R.LP_ATOL <= 1e-4
    for bar, err in ((R.LP_ATOL, lp_err), (R.PSUM_REL, ps_err), (R.RECON_REL, rec_err)):
        assert MARGIN * err <= bar <= 1.2 * MARGIN * err, (bar, err)  # 5 x the measured error, rounded up


def test_act_fast_formulas_meet_the_f16_bar_five_times_over():
    """act_fast (prefill_gemm.h): SiLU as x * rcp(1 + exp2(-log2(e) x)), GELU-tanh through exp2 and rcp,
    evaluated in f32 over integer arguments (what the GLU cases feed it) against float64; a row is 64
    consecutive arguments (the bar's REL_TOL term is of the row's largest |reference|)."""
    x = np.arange(-4096, 4096, dtype=np.float64)
    x32 = x.astype(np.float32)
    f32 = np.float32
    with np.errstate(over="ignore"):
        silu = x32 * (f32(1) / (f32(1) + np.exp2(f32(-1.4426950408889634) * x32, dtype=f32)))
        y = f32(0.797885) * (x32 + f32(0.044715) * x32 * x32 * x32)
        gelu = f32(0.5) * x32 * (f32(1) + (f32(1) - f32(2) * (f32(1) / (np.exp2(f32(2.8853900817779268) * y, dtype=f32) + f32(1)))))
    for act, got in ((C.SILU, silu), (C.GELU, gelu)):
        ref = R.act64(act, x)
        bar = 0.5 * R.ulp16(ref) + R.REL_TOL * np.repeat(np.abs(ref).reshape(-1, 64).max(axis=1), 64)
        assert (MARGIN * np.abs(got.astype(np.float64) - ref) <= bar).all(), act
    assert gelu[0] == 0 and gelu[-1] == 4095  # t = -1 and t = 1 past the exp2 range


def _applies(c, wrong):
    e = C.expect(c)
    return {
        "rope_sign": lambda: True, "rope_row": lambda: c.T > 1, "bias_kv": lambda: c.bias, "clip_after": lambda: True,
        "cache_row": lambda: True, "q_hilo": lambda: not c.split, "kv_hi": lambda: True, "ks2": lambda: bool(e["skinny"]),
        "glu_swap": lambda: True, "hscale_lo": lambda: bool(c.split) and c.hscale != 1.0,
        "scale_x": lambda: c.scale != 1.0, "rows_T": lambda: True,
        "tgt_last_col": lambda: True, "stale_tile": lambda: True,
        "stop256": lambda: c.vocab // max(1, e["bn"][0]) > 256,
        "lo_dropped": lambda: bool(c.split) and c.mode != "nan",
    }[wrong]()


@pytest.mark.parametrize("wrong", sorted(R.WRONG))
def test_wrong_kernels_are_rejected(wrong):
    stage, what = R.WRONG[wrong]
    meant = [c for c in C.CASES if c.stage == stage and _applies(c, wrong)]
    assert len(meant) >= 2, what
    for c in meant:
        ok, val = R.check(c, R.emulate(c, wrong))
        rejected = not ok or (val is not True if c.exact else val > 1.0)
        assert rejected, f"{what}: not rejected at {c} ({ok}, {val})"
