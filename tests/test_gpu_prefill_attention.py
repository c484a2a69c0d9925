"""GPU: the batched prefill's causal attention (csrc/prefill.h attn_prefill_kernel, through
yalm_attn_prefill_rows: the decoder's own launch) against the float64 reference of pf_attn_ref.py,
in the fast and the split-operand form, at head_dim 64 and 128, on the (T, pos0) pairs that sit
on either side of every integer decision of the tile loop and with score structures that drive
the deferred online-softmax rescale (pf_attn_ref.py lists both). The cache carries 70 rows of
NaN / +inf past pos0 + T and o two guard rows past row T.

Bars (pf_attn_ref.py): fast 2^-10 A + 2^-11 |o| + 1e-7 per element with A = p @ |V|; split
280.8 / 1024 of that, four times what the numpy model of the kernel reaches when the MFMA keeps
f16 subnormal inputs. tests/test_pf_attn_cpu.py shows the model under 0.6 fast bars, a model
that flushes the subnormals outside the split bar, and twelve kernel bugs at least 10 bars away.

Measured on an MI355X: fast worst 0.558 bars (head_dim 64, ramp), split worst 0.389 bars (head_dim
128, ramp at pos0 1100), split on flat data 0.007 bars where the flushing model is at 0.13 to 1.0:
the f16 MFMA keeps subnormal inputs. Before the split epilogue took hi and lo from one f32 value
(prefill.h), nine of the ten split tests failed at 1.0 to 2.0 bars on single elements near an f16
tie, d64-split-flat-T64-p0-g3x2 first."""
import numpy as np
import pytest

import pf_attn_ref as P

pytestmark = pytest.mark.gpu


def rt():
    from yalm_amd import runtime

    return runtime


def _run(c):
    q, kc, vc, o_init = P.inputs(c.name)
    return rt().attn_prefill_rows(o_init, q, kc, vc, c.T, c.pos0, c.n_heads, c.n_kv, c.head_dim, split=c.split)


@pytest.mark.parametrize("head_dim,form,flavour", sorted(P.GROUPS))
def test_attn_prefill_against_float64(head_dim, form, flavour):
    worst = 0.0
    for c in P.GROUPS[(head_dim, form, flavour)]:
        o64, A = P.reference(c.name)
        _, _, _, o_init = P.inputs(c.name)
        og = _run(c)
        assert og.shape == o_init.shape
        # nothing written past row T
        np.testing.assert_array_equal(og.view(np.uint16)[c.T:], o_init.view(np.uint16)[c.T:], err_msg=c.name)
        assert np.all(np.isfinite(og[:c.T].astype(np.float32))), c
        b = P.in_bars(P.out_value(c, og), o64, P.bar_of(c, o64, A))
        print(f"{c.name}: {b:.3f} bars")
        worst = max(worst, b)
        assert b <= 1.0, (c.name, b)
        # no atomics, a fixed order: a second call returns the same bits
        np.testing.assert_array_equal(_run(c).view(np.uint16), og.view(np.uint16), err_msg=c.name)
    print(f"head_dim {head_dim} {form} {flavour}: worst {worst:.3f} bars")

