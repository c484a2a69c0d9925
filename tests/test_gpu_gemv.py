"""GPU: the single-row (decode) GEMV (gemv_rb_kernel and gemv_kernel, csrc/gemv.h) through
yalm_gemv_one -- one launch_gemv call, the decoder's own -- at every policy, geometry and weight
type of gemv_cases.py: chunk order and whole-row mode at 256 / 512 / 1024 threads and 2 / 4 / 8 loads
in flight, uneven and capped grids, idle and short waves, x staged from registers and from global
memory on both sides of each capacity, LDS above 64 KiB, the epilogue loop past the first THREADS
groups, the generic kernel's loops and ragged lanes, and the QKV policies' clip, bias, RoPE, cache
rows, raw rows and sink rotation.

Each case must reach the path it names by the library's own plan (the case pins the CU count the
grid is sized for). The exact family (integer weights, activations, residuals and biases, rope
tables of signed powers of two: any f32 summation order gives the one exact result) is compared bit
for bit; the float family (the norm, glu, true cos / sin tables) against float64 at REL_TOL = 2e-5
per output vector, the bar of test_gpu_kernels.py, with half an f16 ulp of the reference ahead of it
for a cache row; tests/test_gemv_cpu.py shows an honest f32 evaluation in the kernels' order meets
that bar five times over in every family. Everything the launch must not write -- the floats behind
out, q_out and raw, every K and V row but kv_pos and the rotated sinks -- must come back with the
bits it went in with, and a second call must return the same bits."""
import numpy as np
import pytest

import gemv_cases as C
import gemv_ref as GR
from yalm_amd import models as M

pytestmark = pytest.mark.gpu


def rt():
    from yalm_amd import runtime

    return runtime


def _run(c):
    i = GR.inputs(c.name)
    kw = dict(threads=c.threads, unroll=c.unroll, wpc=c.wpc, cus=c.cus, rows=c.rows, normw=i.normw, eps=i.eps, act=c.act)
    if c.policy in C.QKV_POLICIES:
        kw.update(wq=i.mats[0], wk=i.mats[1], wv=i.mats[2], n_heads=c.n_heads, n_kv_heads=c.n_kv_heads,
                  head_dim=c.head_dim, qkv_clip=float(i.clip), kv_sink=c.kv_sink, kv_pos=c.kv_pos, rope=i.rope,
                  rope_sink=i.rope_sink, kcache=i.kc0, vcache=i.vc0, q_out=i.q0)
        if c.policy == C.QKVN:
            kw.update(raw=i.raw0)
        if c.policy == C.QKVB:
            kw.update(bq=i.bias[:c.q_dim], bk=i.bias[c.q_dim:c.q_dim + c.kv_dim], bv=i.bias[c.q_dim + c.kv_dim:])
    else:
        kw.update(d=c.d, w=i.mats[0], w3=i.mats[1] if c.policy == C.GLU else None, out=i.out0, base=i.base)
    return rt().gemv_one(c.dtype, c.policy, c.kind, c.n, i.x, **kw)


@pytest.mark.parametrize("dtype,family", list(C.BY_KIND), ids=[f"{C.DTYPE_NAMES[d]}-{f}" for d, f in C.BY_KIND])
def test_gemv_against_reference(dtype, family):
    worst, at = 0.0, None
    for c in C.BY_KIND[(dtype, family)]:
        p = rt().gemv_plan(c.dtype, c.policy, c.kind, c.n, c.n_groups, c.norm, c.threads, c.unroll, c.wpc, c.cus, c.rows)
        assert not C.reaches(c, p), f"{c}: not the path it is there for: {C.reaches(c, p)} ({p})"
        got = _run(c)
        untouched, value = GR.check(c, got)
        path = ("generic" if p["generic"] else f"{'rows' if p['rows'] else 'chunks'} t{p['threads']} U{p['unroll']}"
                ) + f" nb {p['nb']} ngl {p['ngl_min']}..{p['ngl_max']} xregs {p['xregs']} lds {p['lds']}"
        print(f"{c.name} ({path}): " + ("exact" if c.exact else f"{value:.3f} bars"))
        assert untouched, f"{c}: something the launch must not write was written"
        if c.exact:
            assert value, f"{c}: not the reference's bits"
        else:
            assert value <= 1.0, f"{c}: {value:.3f} bars of {GR.rel_tol(c)} per output vector"
            if value > worst:
                worst, at = value, c
        again = _run(c)  # the summation order is fixed: the same bits
        for nm, a in got.items():
            np.testing.assert_array_equal(again[nm].view(np.uint8), a.view(np.uint8), err_msg=f"{c.name} {nm}")
    print(f"{C.DTYPE_NAMES[dtype]} {family}: worst float case {worst:.3f} bars at {at}")


def test_refusals():
    """YALM_ERR_ARG, before anything is uploaded: n no multiple of 16 (q4: of 32), a head_dim that is odd
    or above 256, odd q or kv dims, cache_rows below 2 or at most kv_pos, kv_sink above kv_pos, a
    normalising PAddTo, a geometry the launcher has no kernel for."""
    R = rt()

    def store(n=32, dtype=M.F16, policy=C.STORE1, d=8, w=None, **kw):
        w = np.zeros((d, n), np.float16) if w is None else w
        return R.gemv_one(dtype, policy, C.GK_CLS, n, np.zeros(n, np.float32), d=d, w=w,
                          out=np.zeros(d, np.float32), **kw)

    def qkv(n=32, head_dim=4, n_heads=2, n_kv_heads=1, cache_rows=3, kv_pos=1, kv_sink=0, policy=C.QKV):
        q_dim, kv_dim = n_heads * head_dim, n_kv_heads * head_dim
        z = lambda rows: np.zeros((rows, n), np.float16)
        return R.gemv_one(M.F16, policy, C.GK_QKV, n, np.zeros(n, np.float32), wq=z(q_dim), wk=z(kv_dim), wv=z(kv_dim),
                          n_heads=n_heads, n_kv_heads=n_kv_heads, head_dim=head_dim, qkv_clip=1.0, kv_sink=kv_sink,
                          kv_pos=kv_pos, rope=np.zeros(head_dim, np.float32), rope_sink=np.zeros(head_dim, np.float32),
                          kcache=np.zeros((cache_rows, kv_dim), np.uint16), vcache=np.zeros((cache_rows, kv_dim), np.uint16),
                          q_out=np.zeros(q_dim, np.float32))

    assert store()["out"].shape == (8,) and qkv()["q_out"].shape == (8,)
    for kw, why in ((dict(n=24), "n must be a multiple of 16"),
                    (dict(n=48, dtype=M.Q4, w=np.zeros((8, 32), np.uint8)), "q4: n must be a multiple of 32"),
                    (dict(policy=C.STORE2, d=7), "even row count"), (dict(policy=C.ADDTO, normw=np.ones(32), base=np.zeros(8)),
                                                                     "no normalising form"),
                    (dict(threads=128), "threads"), (dict(unroll=3), "unroll"), (dict(dtype=M.BF16), "bad dtype")):
        with pytest.raises(R.YalmError, match="yalm error 2.*" + why):
            store(**kw)
    for kw, why in ((dict(head_dim=3), "head_dim must be even"), (dict(head_dim=258), "at most 256"),
                    (dict(cache_rows=1, kv_pos=0), "cache_rows must be at least 2"),
                    (dict(cache_rows=3, kv_pos=3), "above kv_pos"), (dict(kv_sink=2, kv_pos=1), "kv_sink <= kv_pos"),
                    (dict(policy=C.QKVB), "needs bq"), (dict(policy=C.QKVN), "needs raw")):
        with pytest.raises(R.YalmError, match="yalm error 2.*" + why):
            qkv(**kw)
