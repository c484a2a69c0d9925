"""CPU: the case table, the bar and the mutants of the fused attention + Wo tests (awo_ref.py), and the
argument errors of the one-launch hook yalm_attn_wo_one, which come back before any device is touched.
The same table runs on the device in test_gpu_attn_wo_one.py."""
import ctypes
import os

import numpy as np
import pytest

import attn_ref as A
import awo_ref as R
from yalm_amd import models as M

MUTANT_BARS = 10.0
ERR_ARG, ERR_UNSUPPORTED = 2, 3


def rt():
    """The library is loaded when a test first needs it, never while the suite is collected (as in every
    other test module: a module collected later imports torch, which brings a HIP runtime of its own, and
    a decoder created after both were loaded in that order gets a wrong occupancy answer)."""
    from yalm_amd import runtime

    return runtime


def _cfg(c, **kw):
    return M.MISTRAL_7B.with_(dim=c.dim, n_heads=c.n_heads, n_kv_heads=c.n_kv, head_dim=128, max_seq_len=c.msl,
                              weight_dtype=c.dtype, **kw)


def test_constants_match_the_project():
    src = open(os.path.join(os.path.dirname(rt().__file__), "csrc", "attn_wo.h")).read()
    assert f"#define AWO_RPW {R.RPW} " in src
    assert R.REL_TOL == 2e-5 and (R.X_ATOL, R.X_RTOL) == (2e-5, 1e-4)
    assert R.D == 128 and A.CHUNK == 64 and A.HEAD_MAX == 4 and A.SPLITS == 32


def test_every_kernel_is_covered():
    """Every attn_wo_kernel<WT, GT, KB> the launcher instantiates: (type, Wo row) x GT in 1, 2, 4, 8 (a G
    above n_heads does not exist); every dim of the table, dim == q_dim, both forms besides the alias."""
    have = {(c.t, c.kb, c.G) for c in R.CASES}
    for t, kb in R.KERNELS:
        for g in R.GTS:
            if g <= R.n_heads_of(t, kb):
                assert (t, kb, g) in have, (t, kb, g)
        cs = R.BY_KERNEL[(t, kb)]
        assert {c.dim for c in cs} >= set(R.DIMS)
        assert {(c.add_base, c.alias) for c in cs} == {(1, 1), (1, 0), (0, 0)}
        assert {kv for c in cs if c.msl == 330 for kv in c.kv} >= set(R.KV_330)
        assert {c.S for c in cs if c.msl == 330} == set(R.S_330)
        assert any(c.msl == 64 and c.S == 1 for c in cs)
    assert any(c.dim == c.q_dim for c in R.CASES)
    big = [c for c in R.CASES if c.msl == 4224]
    assert sorted((c.t, c.kb, c.G, c.kv[0]) for c in big) == [("f16", 4, 4, 2049), ("f16", 4, 4, 4224),
                                                              ("fp8", 8, 2, 2049), ("fp8", 8, 2, 4224)]
    assert all(c.S == 32 for c in big)
    for t in R.TYPES:
        seqs = {(c.S, c.epoch0) for c in R.CASES if c.t == t and len(c.kv) > 1}
        assert seqs == {(6, 1), (6, 1000), (2, 1), (2, 1000)}
        assert all(c.kv == R.SEQ and (c.layer, c.n_layers) == (1, 3) for c in R.CASES if c.t == t and len(c.kv) > 1)


def test_every_type_has_both_modes_poisons_and_flavours():
    for t in R.TYPES:
        cs = [c for c in R.CASES if c.t == t]
        assert {R.mode_of(c, kv) for c in cs for kv in c.kv} == {"head", "key"}
        for mode in ("head", "key"):
            sub = [c for c in cs if len(c.kv) == 1 and R.mode_of(c, c.kv[0]) == mode]
            assert {c.poison for c in sub} == {"nan", "inf"}, (t, mode)
            assert {c.flavour for c in sub} == {"ends", "last"}, (t, mode)
        # fewer live splits than S, the prefetch loop (3 chunks of one split), one chunk per split
        assert any(c.S == 6 and 257 in c.kv for c in cs)
        assert any(c.S == 2 and 330 in c.kv for c in cs)


def test_every_shape_is_one_the_plan_fuses_and_every_split_count_one_it_gives():
    for c in R.CASES:
        ok, S, grid = rt().attn_wo_plan(_cfg(c), 1 << 20)
        assert ok, c
        n_wo = -(-c.dim // R.RPW)
        if c.S == 0:
            assert S == min(R.nchunks(c.msl), A.SPLITS) == R.splits(c)
            continue
        # the slot count at which exactly c.S splits fit beside the mergers and the Wo workgroups
        slots = c.n_kv * (c.S + c.G - 1) + c.n_heads + n_wo
        ok, S, grid = rt().attn_wo_plan(_cfg(c), slots)
        if c.forced:
            assert not ok and c.S == 1 and R.nchunks(c.msl) > A.HEAD_MAX, c
        else:
            assert ok and S == c.S and grid == slots, (c, S, grid)


# ---------------------------------------------------------------- the hook's argument errors
def _args(**kw):
    """A well-formed yalm_attn_wo_args over tiny host arrays (f16, 1-KiB Wo rows), with overrides."""
    n_heads, n_kv, dim, msl, n = 4, 2, 16, 64, kw.pop("n_launch", 1)
    keep = dict(kv_len=np.full(8, 3, np.int32), q=np.zeros((8, n_heads * 128), np.float32),
                x=np.zeros((8, dim), np.float32), kcache=np.zeros(msl * n_kv * 128, np.uint16),
                vcache=np.zeros(msl * n_kv * 128, np.uint16), wo=np.zeros((dim, n_heads * 128), np.float16),
                out=np.zeros((8, dim), np.float32))
    a = rt().AttnWoArgs()
    a.dtype, a.n_heads, a.n_kv_heads, a.dim, a.max_seq_len = M.F16, n_heads, n_kv, dim, msl
    a.S, a.slots, a.delay, a.n_launch, a.epoch0, a.layer, a.n_layers, a.add_base, a.alias = 1, 512, -1, n, 1, 0, 1, 1, 1
    for k, v in keep.items():
        setattr(a, k, v.ctypes.data)
    for k, v in kw.items():
        setattr(a, k, v)
    return a, keep


@pytest.mark.parametrize("kw", [
    dict(kv_len=None), dict(q=None), dict(x=None), dict(kcache=None), dict(vcache=None), dict(wo=None), dict(out=None),
    dict(dim=8), dict(dim=24), dict(dim=0), dict(S=-1), dict(S=33), dict(n_launch=0), dict(n_launch=9),
    dict(epoch0=0), dict(epoch0=-3), dict(layer=-1), dict(layer=1), dict(layer=3, n_layers=3), dict(n_layers=0),
    dict(add_base=0, alias=1), dict(add_base=2), dict(alias=-1), dict(slots=-1), dict(max_seq_len=2),
], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_hook_argument_errors_come_back_without_a_device(kw):
    """YALM_ERR_ARG before anything is uploaded or launched (this machine has no GPU: a hook that
    touched one would return YALM_ERR_HIP)."""
    a, keep = _args(**kw)
    assert rt().lib.yalm_attn_wo_one(ctypes.byref(a)) == ERR_ARG, rt().lib.yalm_last_error()
    assert b"yalm_attn_wo_one" in rt().lib.yalm_last_error()


def test_hook_argument_errors_null_and_kv_len_of_a_later_launch():
    assert rt().lib.yalm_attn_wo_one(None) == ERR_ARG
    for bad in (0, 65, -1):
        a, keep = _args(n_launch=3)
        keep["kv_len"][2] = bad
        assert rt().lib.yalm_attn_wo_one(ctypes.byref(a)) == ERR_ARG


@pytest.mark.parametrize("kw", [
    dict(n_heads=2, n_kv_heads=2),            # f16 Wo rows of 512 B
    dict(n_heads=6, n_kv_heads=2),            # 1.5 KiB
    dict(n_heads=64, n_kv_heads=8),           # f16 rows of 16 KiB
    dict(dtype=M.E4M3, n_heads=16, n_kv_heads=2),  # e4m3 below 4 KiB of codes
    dict(dtype=M.E4M3, n_heads=8, n_kv_heads=8),
    dict(dtype=M.F8E5M2, n_heads=4, n_kv_heads=2),  # fp8 rows of 512 B
    dict(dtype=M.F8E5M2, n_heads=16, n_kv_heads=1),  # G 16
    dict(n_heads=4, n_kv_heads=3), dict(n_heads=4, n_kv_heads=0), dict(n_heads=0),
    dict(dtype=M.F32), dict(dtype=M.Q4),
], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_hook_refuses_what_the_plan_does_not_fuse_without_a_device(kw):
    a, keep = _args(**kw)
    assert rt().lib.yalm_attn_wo_one(ctypes.byref(a)) == ERR_UNSUPPORTED, rt().lib.yalm_last_error()
    assert b"yalm_attn_wo_plan" in rt().lib.yalm_last_error()


# ---------------------------------------------------------------- the bar
@pytest.mark.parametrize("t", list(R.TYPES))
def test_f32_restatement_stays_within_a_fifth_of_the_bar(t):
    """f32 attention, then the Wo half in f32 in the kernel's order of pieces, against float64 at the bar
    of `out` (awo_ref's docstring): under a fifth of it on every launch of every case; the worst per type
    is what awo_ref.F32_WORST records."""
    worst, at = 0.0, None
    for c in R.CASES:
        if c.t != t:
            continue
        r = R.reference(c.name)
        for l in range(len(c.kv)):
            b = R.in_bars(R.restatement32(c, l), r.out[l], r.bar[l])
            assert b < 0.2, (c, l, b)
            if b > worst:
                worst, at = b, (c.name, l)
    print(f"f32 restatement {t}: worst {worst:.4f} bars at {at}")
    assert worst <= R.F32_WORST[t] * 1.01, (t, worst, at)


def test_reference_is_finite_and_the_bar_is_small_beside_the_values():
    for c in R.CASES[::7]:
        r = R.reference(c.name)
        assert np.isfinite(r.out).all() and np.isfinite(r.a).all() and (r.bar > 0).all()
        assert r.bar.max() < 0.02 * np.abs(r.out).max(), (c, r.bar.max(), np.abs(r.out).max())


# ---------------------------------------------------------------- mutants
def test_every_mutant_is_far_outside_the_bar():
    """Each slip moves `out` by at least MUTANT_BARS bars on every launch it applies to (one walk over
    the table: a case's inputs are drawn once for all eight)."""
    n = dict.fromkeys(R.MUTANTS, 0)
    least = dict.fromkeys(R.MUTANTS, (float("inf"), None))
    for c in R.CASES:
        r = R.reference(c.name)
        for l in range(len(c.kv)):
            for m in R.MUTANTS:
                if not R.applies(m, c, l):
                    continue
                b = R.in_bars(R.mutant(m, c, l), r.out[l], r.bar[l])
                n[m] += 1
                least[m] = min(least[m], (b, (c.name, l)))
    for m in R.MUTANTS:
        print(f"{m}: {n[m]} launches, least {least[m][0]:.1f} bars at {least[m][1]}")
    for m in R.MUTANTS:
        assert n[m] > 0 and least[m][0] >= MUTANT_BARS, (m, n[m], least[m])
