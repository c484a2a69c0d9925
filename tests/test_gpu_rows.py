"""GPU: the multi-row GEMV (gemv_rows_kernel, csrc/gemv_rows.h) through yalm_matmul_rows -- one
launch_rows call, the decoder's own -- at every T, weight type and path of rows_cases.py: x staged
whole and in 2 or 3 K segments, the U loop, the chunk tail and the ragged end, gpw 1..3 with idle
and partly idle waves, odd row counts, strides, with and without the norm, RStore / RResidual /
RGlu.

Each case must reach the path it names on THIS device (the plan is re-read with its CU count).
The exact family (integer weights and activations: any f32 summation order gives the one exact
result) is compared bit for bit; the float family (the norm, RGlu) against float64 at REL_TOL =
2e-5 per activation row, the bar of test_gpu_kernels.py, which tests/test_rows_cpu.py shows an
honest f32 evaluation in the kernel's order meets five times over -- but for RGlu with GELU, whose
bar is 2.51e-5, five times that evaluation's measured worst (rows_ref.GELU_GLU_REL_TOL). Every
float of out behind the d outputs must come back as it went in, and a second call must return the
same bits."""
import numpy as np
import pytest

import rows_cases as C
import rows_ref as RR
from yalm_amd import models as M

pytestmark = pytest.mark.gpu


def rt():
    from yalm_amd import runtime

    return runtime


def _run(c):
    i = RR.inputs(c.name)
    return rt().matmul_rows(i.out0, i.x, i.w, c.dtype, c.epilogue, w3=i.w3, normw=i.normw, eps=i.eps, act=c.act)


@pytest.mark.parametrize("dtype,epilogue", sorted(C.BY_KIND),
                         ids=[f"{C.DTYPE_NAMES[d]}-{C.EPILOGUE_NAMES[e]}" for d, e in sorted(C.BY_KIND)])
def test_rows_against_reference(dtype, epilogue):
    worst = 0.0
    for c in C.BY_KIND[(dtype, epilogue)]:
        p = rt().rows_plan(c.dtype, c.n, c.n_groups, c.T, 0)
        assert not C.reaches(c, p), f"{c}: not the path it is there for on this device: {C.reaches(c, p)} ({p})"
        want = RR.reference(c.name)
        got = _run(c)
        assert got.shape == (c.T, c.ostride) and got.dtype == np.float32
        assert RR.pads_intact(c, got), f"{c}: a float behind the outputs was written"
        path = f"nseg {p['nseg']} gpw {p['gpw']} blocks {p['blocks']}"
        if c.exact:
            print(f"{c.name} ({path}): exact")
            np.testing.assert_array_equal(got, want, err_msg=c.name)
        else:
            b = RR.bars(c, got, want)
            print(f"{c.name} ({path}): {b:.3f} bars")
            worst = max(worst, b)
            assert b <= 1.0, f"{c}: {b:.3f} bars of {RR.rel_tol(c)} per activation row"
        again = _run(c)  # the summation order is fixed: the same bits
        np.testing.assert_array_equal(again.view(np.uint32), got.view(np.uint32), err_msg=c.name)
    print(f"{C.DTYPE_NAMES[dtype]} {C.EPILOGUE_NAMES[epilogue]}: worst float case {worst:.3f} bars")


def test_refusals():
    """YALM_ERR_ARG: T outside 1..4, n no multiple of 16, a stride below its row or no multiple of
    4, a bad epilogue, RGlu without w3; YALM_ERR_UNSUPPORTED for q4, in the decoder's words."""
    R = rt()
    w = np.zeros((8, 32), np.float16)

    def call(T=2, n=32, xstride=None, ostride=8, dtype=M.F16, epilogue=C.STORE, w=w, w3=None):
        x = np.zeros((T, n if xstride is None else xstride), np.float32)
        return R.matmul_rows(np.zeros((T, ostride), np.float32), x, w, dtype, epilogue, w3=w3, n=n)

    assert call().shape == (2, 8)
    for kw in (dict(T=5), dict(T=0), dict(n=24, w=np.zeros((8, 24), np.float16)), dict(xstride=28), dict(xstride=34),
               dict(ostride=4), dict(ostride=10), dict(epilogue=3), dict(epilogue=C.GLU), dict(dtype=M.BF16)):
        with pytest.raises(R.YalmError, match="yalm error 2"):
            call(**kw)
    with pytest.raises(R.YalmError, match="yalm error 3.*q4 weights have no multi-row form"):
        call(dtype=M.Q4, w=np.zeros((8, M.row_bytes(M.Q4, 32)), np.uint8))
