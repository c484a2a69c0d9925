"""CPU: what keeps tests/test_gpu_gemv.py honest -- the launch plan of the single-row GEMV
(yalm_gemv_plan, the function launch_gemv itself calls) is the restated plan of gemv_cases.py at every
case and at every GEMV launch of the presets and of Qwen2.5-7B's shapes, it is the geometry the
launcher computed for the Mistral-7B and Llama-3.2-3B launches before the plan became a function of
its own, every case of gemv_cases.py reaches the path it names, every fact the suite is there for
is wanted by a case of every type, an f32 restatement of the kernels' order stays under a fifth of
the GPU test's bar on every float case, and each slip of gemv_ref.DEFECTS is seen.

Measured, the f32 restatement's worst error per output vector against float64, in bars of REL_TOL =
2e-5: store 0.016, residual 0.011, glu 0.047, qkv 0.032 -- all under a fifth, so
every family keeps REL_TOL."""
import numpy as np
import pytest

import gemv_cases as C
import gemv_ref as GR
from yalm_amd import models as M

LDS_PER_CU = 160 * 1024
MUTANT_BARS = 10.0


def rt():
    from yalm_amd import runtime

    return runtime


def lib_plan(c):
    return rt().gemv_plan(c.dtype, c.policy, c.kind, c.n, c.n_groups, c.norm, c.threads, c.unroll, c.wpc, c.cus, c.rows)


def test_constants_match_the_project():
    assert (C.F32, C.F16, C.F8, C.Q4, C.E4M3) == (M.F32, M.F16, M.F8E5M2, M.Q4, M.E4M3)
    assert (C.GELU, C.SILU) == (M.GELU, M.SILU)
    assert (GR.WEIGHT_SCALE, GR.NORM_SCALE, GR.NORM_OFFSET) == (M.WEIGHT_SCALE, M.NORM_SCALE, M.NORM_OFFSET)
    r = rt()
    assert (C.STORE1, C.STORE2, C.RESIDUAL, C.ADDTO, C.GLU, C.QKV, C.QKVB, C.QKVN) == (
        r.GEMV_STORE1, r.GEMV_STORE2, r.GEMV_RESIDUAL, r.GEMV_ADDTO, r.GEMV_GLU, r.GEMV_QKV, r.GEMV_QKVB, r.GEMV_QKVN)
    assert (C.GK_QKV, C.GK_WO, C.GK_GLU, C.GK_W2, C.GK_CLS) == (r.GK_QKV, r.GK_WO, r.GK_GLU, r.GK_W2, r.GK_CLS)
    # the capacities of the xregs staging, each a whole number of every type's chunks
    assert [C.xcap(True, t) for t in (256, 512, 1024)] == [2048, 4096, 8192]
    assert [C.xcap(False, t) for t in (256, 512, 1024)] == [4096, 14336, 16384]
    assert all(C.xcap(nm, t) % 2048 == 0 for nm in (False, True) for t in (256, 512, 1024))


def _launches():
    """(policy, kind, n, n_groups, norm) of every single-row GEMV launch of a dense model's forward pass."""
    shapes = [(c.dim, c.hidden_dim, c.n_heads * c.head_dim, c.n_kv_heads * c.head_dim, c.vocab_size,
               C.QKVN if c.qk_norm else C.QKV)
              for c in (M.MISTRAL_7B, M.LLAMA_32_3B, M.QWEN3_8B, M.TINY, M.SMALL)]
    shapes.append((3584, 18944, 3584, 512, 152064, C.QKVB))  # Qwen2.5-7B
    out = []
    for dim, hidden, q_dim, kv_dim, vocab, qkv in shapes:
        out += [(qkv, C.GK_QKV, dim, (q_dim + 2 * kv_dim) // 2, True), (C.RESIDUAL, C.GK_WO, q_dim, dim, False),
                (C.GLU, C.GK_GLU, dim, hidden, True), (C.RESIDUAL, C.GK_W2, hidden, dim, False),
                (C.STORE2, C.GK_CLS, dim, vocab // 2, True) if vocab % 2 == 0 else (C.STORE1, C.GK_CLS, dim, vocab, True)]
    return out


def test_plan_is_the_restated_plan_at_every_launch():
    """yalm_gemv_plan at 256 CUs, the kind's default geometry, five types x every launch of the presets
    and of Qwen2.5-7B: the restated plan of gemv_cases.py, and the invariants the kernels rely on."""
    generic = set()
    for dt in C.DTYPES:
        for policy, kind, n, G, norm in _launches():
            if dt == C.Q4 and n % 32:
                continue
            p = rt().gemv_plan(dt, policy, kind, n, G, norm, cus=C.PLAN_CUS)
            assert p == C.plan(dt, policy, kind, n, G, norm), (dt, policy, kind, n, G)
            assert 1 <= p["nb"] <= G and p["lds"] <= LDS_PER_CU
            assert p["ngl_min"] >= 1 and p["ngl_max"] - p["ngl_min"] in (0, 1) or p["generic"]
            W = p["threads"] // 64
            if p["generic"]:
                generic.add((dt, n))
                assert p["nb"] * W >= G > (p["nb"] - 1) * W
            else:
                assert p["nb"] * p["ngl_max"] >= G >= p["nb"] * p["ngl_min"]
                assert p["lds"] == (C.xs_len(dt, n) + 64 + p["ngl_max"] * C.POLICY_R[policy] * W) * 4
                if p["rows"]:
                    assert p["ngl_min"] == p["ngl_max"] and (p["ngl_max"] * C.POLICY_R[policy]) % W == 0
    # dim 3584 is not a test-only path: every dim-length row of an fp8 / q4 / e4m3 Qwen2.5-7B is generic
    assert {(C.F8, 3584), (C.Q4, 3584), (C.E4M3, 3584), (C.F8, 18944), (C.Q4, 18944)} <= generic
    assert (C.F16, 3584) not in generic and (C.F32, 18944) not in generic


# {kind: (threads, U, nb, rows, lds)} by hand from the launcher's arithmetic before yalm_gemv_plan
# existed (launch_rb_t / launch_gemv and default_rb_cfg of that commit), at 256 CUs
MISTRAL_PINS = {
    "wide": {C.GK_QKV: (512, 4, 256, 1, 17408), C.GK_WO: (1024, 2, 512, 0, 17152), C.GK_GLU: (512, 4, 256, 1, 20224),
             C.GK_W2: (1024, 2, 256, 0, 58624), C.GK_CLS: (512, 4, 1024, 0, 17664)},
    "narrow": {C.GK_QKV: (512, 4, 256, 1, 17408), C.GK_WO: (512, 2, 512, 0, 16896), C.GK_GLU: (512, 4, 256, 1, 20224),
               C.GK_W2: (512, 4, 256, 1, 58112), C.GK_CLS: (512, 2, 512, 0, 18688)},
    "q4": {C.GK_QKV: (512, 2, 256, 1, 17408), C.GK_WO: (512, 4, 256, 1, 17152), C.GK_GLU: (512, 2, 512, 1, 18432),
           C.GK_W2: (512, 2, 256, 1, 58112), C.GK_CLS: (512, 4, 768, 0, 17984)},
}
LLAMA_PINS = {
    "wide": {C.GK_QKV: (512, 4, 256, 0, 13184), C.GK_WO: (1024, 2, 512, 0, 12928), C.GK_GLU: (512, 4, 256, 1, 14592),
             C.GK_W2: (1024, 2, 256, 0, 33792), C.GK_CLS: (512, 4, 1024, 0, 16576)},
    "narrow": {C.GK_QKV: (512, 4, 256, 0, 13184), C.GK_WO: (512, 2, 512, 0, 12736), C.GK_GLU: (512, 4, 256, 1, 14592),
               C.GK_W2: (512, 4, 256, 0, 33408), C.GK_CLS: (512, 2, 512, 0, 20608)},
}


def _pinned(cfg, pins, types):
    launches = [l for l in _launches() if l[2:4] in (
        (cfg.dim, (cfg.n_heads + 2 * cfg.n_kv_heads) * cfg.head_dim // 2), (cfg.n_heads * cfg.head_dim, cfg.dim),
        (cfg.dim, cfg.hidden_dim), (cfg.hidden_dim, cfg.dim), (cfg.dim, cfg.vocab_size // 2))]
    seen = 0
    for dt in types:
        cls = "q4" if dt == C.Q4 else "narrow" if dt in (C.F8, C.E4M3) else "wide"
        for policy, kind, n, G, norm in {l[1]: l for l in launches}.values():
            p = rt().gemv_plan(dt, policy, kind, n, G, norm, cus=256)
            assert not p["generic"], (dt, kind)
            assert (p["threads"], p["unroll"], p["nb"], p["rows"], p["lds"]) == pins[cls][kind], (dt, kind, p)
            seen += 1
    assert seen == 5 * len(types)


def test_plan_of_the_mistral_and_llama_launches_is_pinned():
    """No production launch changed its kernel instantiation (threads, U, whole-row mode), grid or LDS
    when the launcher began to take them from yalm_gemv_plan."""
    _pinned(M.MISTRAL_7B, MISTRAL_PINS, C.DTYPES)
    _pinned(M.LLAMA_32_3B, LLAMA_PINS, (C.F32, C.F16, C.F8, C.E4M3))
    # q4 Llama-3.2-3B: 3072 is one chunk and a half, so the dim-length rows take the generic kernel
    p = rt().gemv_plan(C.Q4, C.QKV, C.GK_QKV, 3072, 2560, True, cus=256)
    assert (p["generic"], p["threads"], p["unroll"], p["nb"], p["lds"]) == (1, 256, 4, 640, 4096 * 4 + 256)
    # the logits launch: 16000 pairs over 1024 workgroups, 16 or 15 each
    p = rt().gemv_plan(C.F16, C.STORE2, C.GK_CLS, 4096, 16000, True, cus=256)
    assert (p["ngl_min"], p["ngl_max"], p["xregs"]) == (15, 16, 1)
    # Qwen2.5-7B's W2: x above 64 KiB, past every xregs capacity
    p = rt().gemv_plan(C.F16, C.RESIDUAL, C.GK_W2, 18944, 3584, False, cus=256)
    assert p["lds"] > 65536 and not p["xregs"] and not p["generic"]


def test_plan_refusals():
    ok = (C.F16, C.STORE1, C.GK_CLS, 4096, 100)
    rt().gemv_plan(*ok, cus=256)
    for bad, why in (((M.BF16,) + ok[1:], "bad dtype"), ((C.F16, 8) + ok[2:], "bad policy"),
                     ((C.F16, C.STORE1, 5, 4096, 100), "bad kind"), ((C.F16, C.STORE1, C.GK_CLS, 4104, 100), "multiple of 16"),
                     ((C.Q4, C.STORE1, C.GK_CLS, 4112, 100), "q4: n must be a multiple of 32"),
                     ((C.F16, C.STORE1, C.GK_CLS, 4096, 0), "bad argument")):
        with pytest.raises(rt().YalmError, match=why):
            rt().gemv_plan(*bad, cus=256)
    for kw in (dict(threads=128), dict(unroll=3), dict(wpc=-1), dict(cus=-1), dict(rows=1)):
        with pytest.raises(rt().YalmError):
            rt().gemv_plan(*ok, **dict(dict(cus=256), **kw))


def test_every_case_reaches_its_path():
    """By the library's plan; no case is model-sized; and every fact the suite is there for is wanted
    by at least one case of every type it applies to."""
    for c in C.CASES:
        p = lib_plan(c)
        assert p == c.plan(), c
        assert not C.reaches(c, p), (c, C.reaches(c, p))
        assert p["lds"] <= LDS_PER_CU and c.cus in (1, 2, C.PLAN_CUS)
        assert c.n_vrows * M.row_bytes(c.dtype, c.n) <= 6 << 20, c
    for fact, value, types in C.REQUIRED:
        for dt in types or C.DTYPES:
            assert any(c.dtype == dt and fact in c.want and c.want[fact] == value for c in C.CASES), (
                fact, value, C.DTYPE_NAMES[dt])
    for dt in C.DTYPES:
        cs = [c for c in C.CASES if c.dtype == dt]
        f = [(c, C.facts(c, c.plan())) for c in cs]
        for policy in range(8):  # every policy on both kernels
            assert {k["generic"] for c, k in f if c.policy == policy} == {False, True}, (dt, policy)
        assert {c.act for c in cs if c.policy == C.GLU} == {C.SILU, C.GELU}
        # the norm with glu, store1 / store2 and qkv* as production has it, and with residual
        assert {c.policy for c in cs if c.norm} == set(range(8)) - {C.ADDTO}
        # whole-row mode for glu, residual, qkv, qkvb, qkvn; the epilogue loop for residual (PRE)
        assert {c.policy for c, k in f if k.get("rows")} == set(C.ROWS_POLICIES), dt
        assert any(k.get("epi_loop") and c.policy == C.RESIDUAL for c, k in f)
        if dt == C.E4M3:  # the preloaded row scale's split, every policy family
            assert {c.family for c, k in f if k.get("epi_loop")} == set(C.FAMILIES)
        assert any(k["generic"] and c.policy in C.QKV_POLICIES and c.kv_sink == 2 for c, k in f)  # late(early())
        if dt in C.NARROW:
            assert any(c.n == 3584 and k["generic"] for c, k in f)
        assert any(c.n == 18944 and k["lds_big"] and k["generic"] == (dt in C.NARROW) for c, k in f)


def test_clip_cases_clip_some_values_and_not_others():
    n = 0
    for c in C.CASES:
        if c.policy in C.QKV_POLICIES:
            frac = GR.reference(c.name).clipped
            assert (0.05 <= frac <= 0.5) if c.clip else frac == 0.0, (c, frac)
            n += c.clip
    assert n >= 5 * 10


def _detects(c, got):
    untouched, value = GR.check(c, got)
    if c.exact:
        return not (untouched and value)
    return not untouched or value >= MUTANT_BARS


def test_model_without_a_defect_passes_every_case():
    """The float64 traversal is the reference at every case: the same bits on the exact family, within
    a hundredth of a bar on the float family (the model's buffers are f32, and half an f32 ulp is 0.003
    bars of 2e-5), nothing written that must not be."""
    for c in C.CASES:
        untouched, value = GR.check(c, GR.model(c, c.plan()))
        assert untouched, c
        assert value is True if c.exact else value < 1e-2, (c, value)


@pytest.mark.parametrize("family", list(C.FAMILIES))
def test_f32_restatement_stays_within_a_fifth_of_the_bar(family):
    """An honest f32 evaluation in the kernels' order (lane chains of fused multiply-adds, q4's two
    chains per block, the wave_sum butterfly, partials added in wave order, the norm in stage_x's
    statement order, f32 epilogues) stays under a fifth of REL_TOL per output vector on every float
    case; on the small exact cases it must give the reference's bits."""
    worst, at = 0.0, None
    for c in C.CASES:
        if c.family != family or (c.exact and c.n_vrows * c.n > 1 << 17):
            continue
        untouched, value = GR.check(c, GR.model(c, c.plan(), f32=True), tol=GR.REL_TOL)
        assert untouched, c
        if c.exact:
            assert value is True, c
            continue
        if value > worst:
            worst, at = value, c
        assert value < 0.2, (c, value)
    assert worst <= GR.F32_WORST[family] * 1.01, (family, worst)
    print(f"{family}: the f32 restatement's worst error {worst:.4f} bars at {at}")


def _applies(defect, c, k, p):
    """Cases on which the defect changes what is read or written (the others are not tried)."""
    rb, qkv = not k["generic"], c.policy in C.QKV_POLICIES
    return {
        "ngl without the remainder groups": rb and k.get("uneven"),
        "mine one short": rb,
        "advance's while as an if": rb and k.get("multistep"),
        "the start cursor's wave % nch dropped": rb and k.get("cursor_chunk"),
        "whole-row mine rounded down": rb and k.get("rows"),
        "partial slot without the row": rb and p["ngl_max"] * C.POLICY_R[c.policy] > 1,
        "the row flush skipped": rb and k.get("flush"),
        "xr used for gl >= THREADS": rb and k.get("epi_loop") and c.policy == C.RESIDUAL,
        "rs used for gl >= THREADS": rb and k.get("epi_loop") and c.dtype == C.E4M3,
        # (a capacity taken too small only falls back to stage_x: 1024 threads cannot show this slip)
        "xregs capacity taken for the wrong thread count": rb and k.get("xcap") == "above" and p["threads"] < 1024,
        "the norm's sum over clamped duplicates": rb and c.norm and k.get("xclamp"),
        "generic tail loop skipped": k["generic"] and k.get("tail"),
        "rem lanes off by one": k["generic"],
        "q4 scale one chunk off": c.dtype == C.Q4,
        "xs_at<true> taken as plain for the last partial 2048-block": k["generic"] and k.get("q4_partial"),
        "rope index without % head_dim": c.policy in (C.QKV, C.QKVB) and c.n_heads > 1,
        "K at row pos instead of kv_pos": c.policy in (C.QKV, C.QKVB),
        "V rotated": qkv,
        "bias after the clip": c.policy == C.QKVB and c.clip,
        "sink rotation with rope": qkv and c.kv_sink > 0,
        "sink rotation when kv_sink = 0": qkv and c.kv_sink == 0,
        "late as an if": qkv and k.get("late_loops"),
        "raw indexed per matrix instead of 2g": c.policy == C.QKVN,
    }[defect]


@pytest.mark.parametrize("defect", GR.DEFECTS)
def test_every_defect_is_seen(defect):
    """Each slip, switched into the traversal model, changes a bit of an exact case or makes a float
    case miss by at least 10 bars -- in EVERY case the slip applies to that is tried (the smallest twelve
    and the smallest four of the float family), not just one: a slip that some case lets through
    would be a case that proves less than it seems to."""
    tried, floats = [], 0
    for c in sorted(C.CASES, key=lambda c: c.n_vrows * c.n):
        p = c.plan()
        if not _applies(defect, c, C.facts(c, p), p):
            continue
        if len(tried) >= 12 and (c.exact or floats >= 4):
            continue
        assert _detects(c, GR.model(c, p, defect=defect)), (defect, c)
        tried.append(c)
        floats += not c.exact
    assert tried, f"no case for: {defect}"
    print(f"{defect}: seen by {', '.join(c.name for c in tried)}")
