"""GPU: the fused attention + Wo launch (csrc/attn_wo.h), one launch at a time through
yalm_attn_wo_one -- the launcher the forward itself calls -- against the float64 reference of
awo_ref.py: every attn_wo_kernel<WT, GT, KB>, Wo rows of 1 to 8 KiB, forced key-split counts from 1
to 32, sequences over one set of buffers (a shrinking context, epochs from 1 and from 1000) and the
forms of a tensor-parallel rank (out a buffer of its own, with and without the base).

Per launch: the hook returns YALM_OK (no error bit, guard rows intact); the granules carry the
launch's epoch and values within attn_ref's bars of mha_ref, finite despite the poisoned tail, and
-- where the launch has the standalone kernel's split count -- the bits of yalm_mha; `out` is within
the decode GEMV's bar (gemv_ref.REL_TOL) of base + W . g for the granule values g the device itself
produced, and within the propagated bar of awo_ref.py of the float64 reference; x comes back
untouched where out is no alias; a second call gives the same bits. tests/test_attn_wo_cpu.py shows
that the f32 restatement stays under a fifth of the end-to-end bar and that the slips of
awo_ref.MUTANTS are at least 10 bars away."""
import numpy as np
import pytest

import attn_ref as A
import awo_ref as R

pytestmark = pytest.mark.gpu


def rt():
    from yalm_amd import runtime

    return runtime


def _run(c, S=None):
    """One yalm_attn_wo_one call; runtime.attn_wo_one raises unless it returned YALM_OK (an error bit of
    a bounded wait, a written guard row, an error of the launch)."""
    i = R.inputs(c.name)
    return rt().attn_wo_one(c.dtype, c.n_heads, c.n_kv, c.dim, c.msl, c.kv, i.q, i.x, i.kb, i.vb, i.wo, out=i.out0,
                            S=c.S if S is None else S, epoch0=c.epoch0, layer=c.layer, n_layers=c.n_layers,
                            add_base=c.add_base, alias=c.alias)


def _check(c, worst):
    i, r = R.inputs(c.name), R.reference(c.name)
    got = _run(c)
    assert got["err"] == 0, c
    nl = len(c.kv)
    for l in range(nl):
        tag = f"{c.name} launch {l} (kv {c.kv[l]}, S {got['S']}, {R.mode_of(c, c.kv[l], got['S'])} mode)"
        # ---- the granules: this launch's epoch in every tag, the attention output in every value
        assert np.all(got["tags"][l] == c.epoch0 + l), tag
        g = got["values"][l]
        assert np.all(np.isfinite(g)), tag
        bg = A.bars(g, r.a[l], A.X_ATOL, A.X_RTOL)
        np.testing.assert_allclose(g, r.a[l], atol=A.X_ATOL, rtol=A.X_RTOL, err_msg=tag)
        # ---- the bits of the standalone kernel where the split count is its own: the same attn_core /
        # attn_merge_body, only the store differs
        if got["S"] == min(R.nchunks(c.msl), A.SPLITS):
            xs, _ = rt().mha(i.kb, i.vb, i.q[l], R.D, c.kv[l], c.msl, c.n_heads, c.n_kv)
            np.testing.assert_array_equal(g.view(np.uint32), xs.view(np.uint32), err_msg=tag)
        # ---- the Wo half alone: a plain f32 GEMV over the values the device itself produced
        out = got["out"][l]
        bw = R.gemv_bars(out, R.wo_ref(c, l, g.astype(np.float64)))
        # ---- end to end
        be = R.in_bars(out, r.out[l], r.bar[l])
        print(f"{tag}: granules {bg:.3f} bars, Wo half {bw:.3f} bars, out {be:.5f} bars")
        assert bw <= 1.0, (tag, bw)
        assert be <= 1.0, (tag, be)
        for k, b in zip(("gran", "wo", "out"), (bg, bw, be)):
            worst[k] = max(worst[k], b)
    if not c.alias:
        np.testing.assert_array_equal(got["x"].view(np.uint32), i.x.view(np.uint32), err_msg=c.name)
    # ---- the hand-offs are ordered by tags, the sums run in a fixed order: the same bits again
    again = _run(c)
    np.testing.assert_array_equal(again["out"].view(np.uint32), got["out"].view(np.uint32), err_msg=c.name)
    np.testing.assert_array_equal(again["gran"], got["gran"], err_msg=c.name)


@pytest.mark.parametrize("t,kb", R.KERNELS, ids=[f"{t}-{kb}k" for t, kb in R.KERNELS])
def test_attn_wo_one_against_float64(t, kb):
    worst = dict(gran=0.0, wo=0.0, out=0.0)
    for c in R.BY_KERNEL[(t, kb)]:
        if c.msl == 4224 or len(c.kv) > 1:
            continue
        _check(c, worst)
    print(f"{t} {kb} KiB: worst granules {worst['gran']:.3f} bars, Wo half {worst['wo']:.3f} bars, "
          f"out {worst['out']:.5f} bars")


@pytest.mark.parametrize("name", [c.name for c in R.CASES if c.msl == 4224 or len(c.kv) > 1])
def test_attn_wo_one_long_windows_and_sequences(name):
    """32 key splits of 2 or 3 chunks over a window of 4224; and kv_len 330, 257, 100, 321, 64, 330 over
    ONE partial buffer and ONE granule buffer, neither cleared between the launches: each launch's out
    and granules against the reference OF THAT LAUNCH, so a partial or a granule that matched on an
    earlier launch's tag shows."""
    worst = dict(gran=0.0, wo=0.0, out=0.0)
    _check(R.BY_NAME[name], worst)
    print(f"{name}: worst granules {worst['gran']:.3f} bars, Wo half {worst['wo']:.3f} bars, out {worst['out']:.5f} bars")


@pytest.mark.parametrize("t,kb", [("f16", 4), ("fp8", 8)])
def test_fused_launch_against_the_separate_launches(t, kb):
    """What the suite already trusts: yalm_mha, then the decode GEMV with the residual epilogue on the same
    Wo, against the hook at the plan's own split count -- within the fused-vs-separate bar of
    test_gpu_attn_wo.py (1e-4 relative: only the f32 summation order of Wo differs)."""
    runtime = rt()
    cases = [c for c in R.BY_KERNEL[(t, kb)] if (c.S, c.msl, c.alias) == (0, 330, 1)]
    assert len(cases) == len(R.KV_330)
    for c in cases:
        i = R.inputs(c.name)
        got = _run(c)
        xs, _ = runtime.mha(i.kb, i.vb, i.q[0], R.D, c.kv[0], c.msl, c.n_heads, c.n_kv)
        sep = runtime.gemv_one(c.dtype, runtime.GEMV_RESIDUAL, runtime.GK_WO, c.q_dim, xs, d=c.dim, w=i.wo,
                               out=i.x[0])["out"]
        e = float(np.max(np.abs(got["out"][0] - sep)) / np.max(np.abs(sep)))
        print(f"{c.name}: fused vs separate {e:.2e}")
        assert e < 1e-4, (c, e)
