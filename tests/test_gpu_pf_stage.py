"""GPU: the stages of the batched prefill one launch sequence at a time, through yalm_prefill_stage --
the functions enqueue_prefill itself calls (csrc/prefill.hip), on host arrays -- at every case of
pf_stage_cases.py: the row norm at every NV bracket and the workgroup kernel; the QKV GEMM's epilogue
(bias, clip, RoPE, Q and cache rows) in its four forms (skinny, one GEMM over [hi | lo], one launch
with two depths, q then k | v at a column offset) at every tile width, 8-phase and 2-phase; the
residual epilogue of Wo and W2 with and without the power-of-two scale, in the persistent tile loop
and at odd and even K tile counts; the GLU epilogue with both activations, both widths, the [hi | lo]
store and the range slot; the logits epilogue and logprob_kernel with the target at every edge column,
in the persistent tile loop and past 256 vocab tiles; and the skinny reduce at 1 .. 10 partials.

Each case asserts first that the library took the path the case names (reaches), then check: what the
launch must not write (rows past T, cache rows outside [pos0, pos0 + T), tgt_logit of rows without a
target) kept its 0xA5 bytes; an exact case (integer operands, biases and residuals, rope entries of
(+-1, 0), (0, +-1), (+-1/2, +-1/2), power-of-two scales: any f32 summation order gives the one result)
is the float64 reference's bits; a float case is within its bar: half an f16 ulp of the reference plus
REL_TOL = 2e-5 of the row's largest |reference| for an f16 output (counted in bars of the REL_TOL part
beyond the half ulp), REL_TOL of the row's largest |reference| for an f32 one, and the bars measured
in test_pf_stage_cpu.py as 5 x the worst error of an f32 evaluation in the kernels' order: log p 3.2e-5
nats (measured 6.29e-6), a tile's sum of exp 3.2e-5 relative (6.24e-6), the norm's hi + lo 1.1e-6 of
the row's largest |y| (2.06e-7). Then a second call must return the same bits. test_pf_stage_cpu.py
shows check rejects sixteen deliberately wrong kernels at these cases."""
import numpy as np
import pytest

import pf_stage_cases as C
import pf_stage_ref as R

pytestmark = pytest.mark.gpu


def rt():
    from yalm_amd import runtime

    return runtime


def _run(c):
    rt().set_gemm_forms(c.forms)
    try:
        return rt().prefill_stage(c.stage, **R.inputs(c).kw)
    finally:
        rt().set_gemm_forms("")


def _path(c, p):
    if c.stage == C.NORM:
        return f"wave NV {p['norm_nv']}" if p["norm_nv"] else "workgroup per row"
    if p["skinny"]:
        return f"skinny ks {p['ks']} ks2 {p['ks2']}"
    w = "+".join(f"{p['bn'][j]}{'/8p' if p['eight_phase'] >> j & 1 else '/2p'}" for j in range(p["n_gemm"]))
    return f"tiles {w}{' two-depth' if p['two_depth'] else ''} grid {p['grid']} of {p['tiles']}" + (
        " persistent" if p["persistent"] else "")


@pytest.mark.parametrize("stage,family", list(C.BY_STAGE), ids=[f"{C.STAGE_NAMES[s]}-{f}" for s, f in C.BY_STAGE])
def test_stage_against_reference(stage, family):
    worst, at = 0.0, None
    for c in C.BY_STAGE[(stage, family)]:
        got, p = _run(c)
        assert not C.reaches(c, p), f"{c}: not the path it is there for: {C.reaches(c, p)} ({p})"
        untouched, value = R.check(c, got)
        print(f"{c.name} ({_path(c, p)}): " + (("exact" if value else "NOT EXACT") if c.exact else f"{value:.3f} bars"))
        assert untouched, f"{c}: something the launch must not write was written"
        if c.exact:
            assert value, f"{c}: not the reference's bits"
        else:
            assert value <= 1.0, f"{c}: {value:.3f} bars"
            if value > worst:
                worst, at = value, c
        again, _ = _run(c)  # the summation order is fixed: the same bits
        for nm, a in got.items():
            np.testing.assert_array_equal(again[nm].view(np.uint8), a.view(np.uint8), err_msg=f"{c.name} {nm}")
    if family == "float":
        print(f"{C.STAGE_NAMES[stage]}: worst float case {worst:.3f} bars at {at}")


def test_skl_forms_give_the_same_bits():
    """The skinny GEMMs' two weight paths (skl:1 LDS-DMA stages, skl:0 register loads) leave the same partials."""
    twins = [c for c in C.CASES if "skl:0" in c.forms.split(",") and c.family == "float"]
    assert twins
    for c in twins:
        got0, _ = _run(c)
        rt().set_gemm_forms(",".join(k for k in c.forms.split(",") if k != "skl:0"))
        try:
            got1, p = rt().prefill_stage(c.stage, **R.inputs(c).kw)
        finally:
            rt().set_gemm_forms("")
        assert p["skinny"]
        for nm, a in got0.items():
            np.testing.assert_array_equal(got1[nm].view(np.uint8), a.view(np.uint8), err_msg=f"{c.name} {nm}")


def test_refusals():
    """YALM_ERR_ARG, before anything is uploaded: a dim that is no multiple of 128 (a depth: of 64), a head_dim
    other than 64 or 128, cache_rows < pos0 + T, q_rows / x_rows / h_rows / xn_rows < T, a target >= vocab, a
    scale that is no power of two, an unknown stage."""
    Rt = rt()
    z16 = lambda *s: np.zeros(s, np.uint16)
    z32 = lambda *s: np.zeros(s, np.float32)
    rng = lambda: np.zeros(1, np.uint32)

    def norm(dim=128, T=2, xn_rows=2):
        return Rt.prefill_stage(C.NORM, T=T, dim=dim, x=z32(T, dim), normw=z32(dim), eps=1.0, xn=z16(max(xn_rows, 1), dim),
                                xn_rows=xn_rows, range=rng())

    def qkv(dim=128, nh=1, nkv=1, hd=128, T=2, pos0=1, q_rows=2, cache_rows=3):
        qd, kd = nh * hd, nkv * hd
        return Rt.prefill_stage(C.QKV, T=T, dim=dim, a=z16(T, 2 * dim), n_heads=nh, n_kv_heads=nkv, head_dim=hd, pos0=pos0,
                                q_rows=q_rows, cache_rows=cache_rows, clip=1.0, wq=z16(qd, dim), wk=z16(kd, dim),
                                wv=z16(kd, dim), rope=z32(T, hd), q=z16(max(q_rows, 1), qd),
                                kc=z16(max(cache_rows, 1), kd), vc=z16(max(cache_rows, 1), kd), range=rng())

    def res(n=128, k=64, T=2, x_rows=2, scale=1.0, kind=C.PF_WO):
        return Rt.prefill_stage(C.RESIDUAL, T=T, a=z16(T, k), kind=kind, n=n, k=k, x_rows=x_rows, w=z16(n, k),
                                scale=scale, xres=z32(max(x_rows, 1), n))

    def glu(hidden=128, dim=64, T=2, h_rows=2, hscale=1.0, act=C.SILU):
        return Rt.prefill_stage(C.GLU, T=T, dim=dim, a=z16(T, dim), hidden=hidden, act=act, h_rows=h_rows,
                                w1=z16(hidden, dim), w3=z16(hidden, dim), hscale=hscale, h=z16(max(h_rows, 1), hidden),
                                range=rng())

    def lp(vocab=128, dim=64, T=2, targets=(0, -1)):
        return Rt.prefill_stage(C.LOGPROB, T=T, dim=dim, a=z16(T, dim), vocab=vocab, wcls=z16(vocab, dim),
                                targets=np.array(targets, np.int32), lp=z32(T), pmax=z32(T * (vocab // 128 + 1)),
                                psum=z32(T * (vocab // 128 + 1)), tgt_logit=z32(T))

    assert norm()[0]["xn"].shape == (2, 128) and qkv()[0]["q"].shape == (2, 128) and res()[0]["xres"].shape == (2, 128)
    assert glu()[0]["h"].shape == (2, 128) and lp()[0]["lp"][1] == 0.0
    for fn, kw, why in ((norm, dict(dim=192), "multiple of 128"), (norm, dict(xn_rows=1), "xn_rows >= T"),
                        (qkv, dict(hd=32, nh=4, nkv=4), "head_dim must be 64 or 128"), (qkv, dict(dim=96), "multiple of 64"),
                        (qkv, dict(cache_rows=2), "cache_rows >= pos0 \\+ T"), (qkv, dict(q_rows=1), "q_rows >= T"),
                        (res, dict(n=192), "multiple of 128"), (res, dict(k=96), "k of 64"), (res, dict(x_rows=1), "x_rows >= T"),
                        (res, dict(scale=3.0), "power of two"), (res, dict(kind=2), "kind must be"),
                        (glu, dict(hidden=64), "multiple of 128"), (glu, dict(h_rows=1), "h_rows >= T"),
                        (glu, dict(hscale=0.3), "power of two"), (glu, dict(act=7), "bad activation"),
                        (lp, dict(vocab=192), "multiple of 128"), (lp, dict(targets=(128, -1)), "target out of range"),
                        (lp, dict(targets=(0, -2)), "target out of range")):
        with pytest.raises(Rt.YalmError, match="yalm error 2.*" + why):
            fn(**kw)
    with pytest.raises(Rt.YalmError, match="yalm error 2.*unknown stage"):
        Rt.prefill_stage(9, T=1)
