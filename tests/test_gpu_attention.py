"""GPU: decode attention (yalm_mha, csrc/attention.h) against the float64 reference of
attn_ref.py at every (head_dim, G) pair the dispatcher accepts -- head_dim 16 .. 256 x G 1 .. 8,
so every attn_decode_kernel<D, GT> with G == GT and with masked heads -- in head mode and key
mode, with planted dominant keys and a poisoned tail (NaN / +inf in every K and V row past
kv_len).

Bars: the project's own of test_gpu_kernels.py::test_mha_shapes, against float64 here (xout
2e-5 + 1e-4 |x|, att 2e-6 + 1e-4 |p|). tests/test_attn_cpu.py shows that the f32 oracle stays
under a sixth of them on these cases at every window, 4224 keys included, and that an attention
that mixes up the heads' q or loses key 0 or key kv_len - 1 is at least 10 bars away."""
import numpy as np
import pytest

import attn_ref as A

pytestmark = pytest.mark.gpu


def rt():
    from yalm_amd import runtime

    return runtime


def _run(c):
    """One yalm_mha call over a sentinel-filled att; runtime.mha raises unless the call returned
    YALM_OK (an error code of the launch, or the merger's bounded wait giving up)."""
    kb, vb, q = A.inputs(c.name)
    return rt().mha(kb, vb, q, c.head_dim, c.kv_len, c.max_seq_len, c.n_heads, c.n_kv, att_init=A.att_init(c))


# (head_dim 256 first: its widest instantiations are the ones at the register and LDS limits)
@pytest.mark.parametrize("head_dim,G", sorted(A.PAIRS, key=lambda p: (-p[0], p[1])))
def test_mha_against_float64(head_dim, G):
    worst = [0.0, 0.0]
    for c in A.BY_PAIR[(head_dim, G)]:
        xr, ar = A.reference(c)
        xg, ag = _run(c)
        assert np.all(np.isfinite(xg)), c
        live_g, tail_g = A.live(c, ag)
        live_r, _ = A.live(c, ar)
        assert np.all(tail_g == np.float32(A.SENTINEL)), c  # nothing written past kv_len
        bx = A.bars(xg, xr, A.X_ATOL, A.X_RTOL)
        ba = A.bars(live_g, live_r, A.A_ATOL, A.A_RTOL)
        print(f"{c.name} ({c.mode} mode): xout {bx:.3f} bars, att {ba:.3f} bars")
        worst = [max(worst[0], bx), max(worst[1], ba)]
        np.testing.assert_allclose(xg, xr, atol=A.X_ATOL, rtol=A.X_RTOL, err_msg=c.name)
        np.testing.assert_allclose(live_g, live_r, atol=A.A_ATOL, rtol=A.A_RTOL, err_msg=c.name)
        # the merge order is fixed: a second call returns the same bits
        x2, a2 = _run(c)
        np.testing.assert_array_equal(x2.view(np.uint32), xg.view(np.uint32), err_msg=c.name)
        np.testing.assert_array_equal(a2.view(np.uint32), ag.view(np.uint32), err_msg=c.name)
    print(f"head_dim {head_dim} G {G}: worst xout {worst[0]:.3f} bars, att {worst[1]:.3f} bars")
