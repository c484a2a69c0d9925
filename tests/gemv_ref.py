"""Inputs, plain references and a numpy model of both kernels' traversal for the single-row GEMV
tests (gemv_cases.py has the cases). TEST INFRASTRUCTURE ONLY; needs no library.

Two input families, every case seeded by its name:
  exact (store1 / store2 / residual / addto / qkv* without the norm): weights are integers in
    -3 .. 3 (exact in f16, E5M2 and E4M3; q4: nibbles 5 .. 11 under scale 1), e4m3 row scales are
    2^-1 .. 2^2, x is integers in -4 .. 4 (qkv*: -2 .. 2), the residual / base / bias are integers.
    Every partial sum of every order is then an integer below 2^24 (reference() asserts it), so any
    f32 summation is exact. The qkv* rope tables hold (+-2^a, 0) or (0, +-2^b) per pair, distinct per
    j; (1, 0) past rotary_dim; the clip level is an integer. Bias, clip and rotation are then exact
    in f32 and the f16 cache store rounds an exact value: the result has one bit pattern.
  float (the norm, glu; qkv* with true cos / sin tables): weights uniform at WEIGHT_SCALE rounded to
    the stored type (e4m3: rows at 1, 2, 4 x WEIGHT_SCALE in turn, so that neighbouring row scales
    differ), normw at NORM_OFFSET +- NORM_SCALE, x standard normal. The reference is float64
    over the stored weights' exact values with the oracle's formulas (its f32 constants).
Both: every buffer the launch may write (out, q_out, raw, the K and V caches) is longer than what it
writes and starts as a NaN pattern (NAN32 / NAN16) but for the residual's rows and the cache's sink
rows; check() wants every bit the launch must not write back as it went in.

model() walks the launch as the kernels do: groups to workgroups, items dealt to waves, the issue
cursor and advance, `mine`, per-(row, wave) partials parked in LDS and summed in wave order, the
xregs staging with its clamped loads, the epilogue loop with its gl == tid split, early / late --
in float64 (exact family; defects) or as an f32 restatement of the kernel's order (lane chains of
fused multiply-adds, q4's two chains per block, the wave_sum butterfly, stage_x's statement order).
DEFECTS are the slips test_gemv_cpu.py switches in one at a time. LDS and memory the kernel never
wrote read as 0 here, the value that hides the most."""
import functools
import zlib

import numpy as np

import gemv_cases as C
from yalm_amd import models as M

WEIGHT_SCALE = 0.035               # yalm_amd.models WEIGHT_SCALE
NORM_SCALE, NORM_OFFSET = 0.2, 1.0  # yalm_amd.models NORM_SCALE, NORM_OFFSET
EPS = 1e-5
REL_TOL = 2e-5  # tests/test_gpu_kernels.py REL_TOL, here per output vector against float64
# The f32 restatement of the kernels' order (test_gemv_cpu.py test_f32_restatement_stays_within_a_fifth_of_the_bar)
# against float64, the worst case per family in units of REL_TOL, as measured: glu at
# e4m3-glu-n4112-d5-t512u4w1c256-gelu, qkv at fp8-qkvn-n5168-h3x1x6-s0p2r4-clip-t512u4w1c256-norm, store at
# fp8-store1-n3584-d5-t512u4w1c256-norm, residual at q4-residual-n4096-d5-t512u4w1c256-norm. All are below a
# fifth of the bar, so every family keeps REL_TOL (a family above 0.2 would get 5 x its worst as its bar).
F32_WORST = {"store": 0.016, "residual": 0.011, "glu": 0.047, "qkv": 0.032}
FLT_MAX = float(np.finfo(np.float32).max)
NAN32 = np.uint32(0x7FC0BEEF)
NAN16 = np.uint16(0x7E5A)
ROPE_THETA = 10000.0
GELU_C0, GELU_C1 = float(np.float32(0.797885)), float(np.float32(0.044715))

DEFECTS = (
    "ngl without the remainder groups",
    "mine one short",
    "advance's while as an if",
    "the start cursor's wave % nch dropped",
    "whole-row mine rounded down",
    "partial slot without the row",
    "the row flush skipped",
    "xr used for gl >= THREADS",
    "rs used for gl >= THREADS",
    "xregs capacity taken for the wrong thread count",
    "the norm's sum over clamped duplicates",
    "generic tail loop skipped",
    "rem lanes off by one",
    "q4 scale one chunk off",
    "xs_at<true> taken as plain for the last partial 2048-block",
    "rope index without % head_dim",
    "K at row pos instead of kv_pos",
    "V rotated",
    "bias after the clip",
    "sink rotation with rope",
    "sink rotation when kv_sink = 0",
    "late as an if",
    "raw indexed per matrix instead of 2g",
)


def rel_tol(c):
    return max(REL_TOL, 5 * F32_WORST[c.family] * REL_TOL) if F32_WORST[c.family] > 0.2 else REL_TOL


def step_pos(c):
    """StepState::pos of the hook's launch: a cache row other than kv_pos ((kv_pos + 1) % cache_rows),
    so that a K or V row stored at pos lands where check() sees it."""
    return (c.kv_pos + 1) % c.cache_rows


# ---------------------------------------------------------------- inputs
class Inputs:
    __slots__ = ("x", "normw", "eps", "mats", "vals", "rscale", "q4u", "q4s", "out0", "base", "bias", "rope",
                 "rope_sink", "kc0", "vc0", "q0", "raw0", "clip")


def _nan32(n):
    return np.full(n, NAN32, np.uint32).view(np.float32)


def _store_matrix(v, dtype, rng, exact):
    """float matrix (rows, n) -> (stored rows, element values float64 without e4m3's row scale,
    row scales float64, q4 (u - 8) values, q4 group scales)."""
    rows, n = v.shape
    ones = np.ones(rows)
    if dtype == C.Q4:
        if exact:
            a = M.q4_pack((v + 8).astype(np.uint8), np.full((rows, n // 32), 0x3C00, np.uint16))
        else:
            a = M.q4_quantize(v)
        u, sb = M.q4_unpack(a, n)
        s = sb.view(np.float16).astype(np.float64)
        qu = u.astype(np.float64) - 8.0
        return a, qu * np.repeat(s, 32, axis=1), ones, qu, s
    if dtype == C.E4M3:
        if exact:
            a = M.e4m3_pack(M.e4m3_encode(v), np.ldexp(1.0, rng.integers(-1, 3, rows)).astype(np.float32))
        else:
            a = M.e4m3_quantize(v)
        codes, s = M.e4m3_unpack(a, n)
        return a, M.e4m3_table()[codes].astype(np.float64), s.astype(np.float64), None, None
    a = M.encode_weights(v.astype(np.float32), dtype)
    return a, M.decode_weights(a, dtype).astype(np.float64), ones, None, None


def _rope_table(c, rng, pos, exact):
    """head_dim floats: (cos, sin) of pos * theta^(-2 j / rotary_dim) in f32, or the exact family's
    (+-2^a, 0) / (0, +-2^b); (1, 0) past rotary_dim."""
    half = c.head_dim // 2
    t = np.zeros((half, 2), np.float32)
    t[:, 0] = 1.0
    live = c.rotary // 2
    if exact:
        mag = np.ldexp(1.0, rng.integers(-1, 2, live)) * rng.choice((-1.0, 1.0), live)
        side = (np.arange(live) + rng.integers(0, 2)) % 2  # neighbours differ: a slip by one pair shows
        t[:live] = 0.0
        t[np.arange(live), side] = mag
    else:
        ang = (np.float32(pos) * (ROPE_THETA ** (-2.0 * np.arange(live) / c.rotary)).astype(np.float32))
        t[:live, 0], t[:live, 1] = np.cos(ang), np.sin(ang)
    return t.reshape(-1)


@functools.lru_cache(maxsize=4)
def inputs(name):
    """The case's arrays, read-only: x (n), normw, mats (the stored weight matrices: [w], [w, w3] or
    [wq, wk, wv]), vals / rscale (their exact element values and row scales, stacked over the launch's
    virtual rows), and every buffer the launch may write as the launch finds it."""
    c = C.BY_NAME[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    i = Inputs()
    qkv = c.policy in C.QKV_POLICIES
    shapes = [c.q_dim, c.kv_dim, c.kv_dim] if qkv else [c.d] * (2 if c.policy == C.GLU else 1)
    i.eps = EPS if c.norm else 0.0
    i.normw = (NORM_OFFSET + (rng.random(c.n) * 2 - 1) * NORM_SCALE).astype(np.float32) if c.norm else None
    parts = []
    for rows in shapes:
        v = (rng.integers(-3, 4, (rows, c.n)).astype(np.float64) if c.exact
             else (rng.random((rows, c.n)) * 2 - 1) * WEIGHT_SCALE)
        if c.dtype == C.E4M3 and not c.exact:  # rows of 1, 2, 4 x WEIGHT_SCALE in turn over the launch's virtual
            # rows: the row scales of rows 256 groups apart differ (a scale taken from the wrong group shows)
            row0 = sum(p[1].shape[0] for p in parts)
            v *= np.array([1.0, 2.0, 4.0])[(row0 + np.arange(rows)) % 3][:, None]
        parts.append(_store_matrix(v, c.dtype, rng, c.exact))
    i.mats = [p[0] for p in parts]
    i.vals = np.concatenate([p[1] for p in parts])
    i.rscale = np.concatenate([p[2] for p in parts])
    i.q4u = np.concatenate([p[3] for p in parts]) if c.dtype == C.Q4 else None
    i.q4s = np.concatenate([p[4] for p in parts]) if c.dtype == C.Q4 else None
    if c.exact:
        i.x = rng.integers(-2, 3, c.n).astype(np.float32) if qkv else rng.integers(-4, 5, c.n).astype(np.float32)
    else:
        i.x = rng.standard_normal(c.n).astype(np.float32)
    i.out0 = i.base = i.bias = i.rope = i.rope_sink = i.kc0 = i.vc0 = i.q0 = i.raw0 = None
    i.clip = np.float32(FLT_MAX)
    if not qkv:
        i.out0 = _nan32(c.d + 5)
        if c.policy == C.RESIDUAL:
            i.out0[:c.d] = rng.integers(-999, 1000, c.d) if c.exact else rng.standard_normal(c.d)
        if c.policy == C.ADDTO:
            i.base = rng.integers(-999, 1000, c.d).astype(np.float32)
    else:
        nb = c.q_dim + 2 * c.kv_dim
        if c.policy == C.QKVB:
            i.bias = (rng.integers(-20, 21, nb) if c.exact else rng.standard_normal(nb) * 0.5).astype(np.float32)
        i.rope = _rope_table(c, rng, c.kv_pos + 5, c.exact)
        i.rope_sink = _rope_table(c, rng, 1, c.exact)
        i.q0, i.raw0 = _nan32(c.q_dim + 3), _nan32(c.q_dim + c.kv_dim + 3)
        i.kc0 = np.full((c.cache_rows, c.kv_dim), NAN16, np.uint16)
        i.vc0 = np.full((c.cache_rows, c.kv_dim), NAN16, np.uint16)
        sink = (rng.integers(-8, 9, (C.KV_SINKS, c.kv_dim)) if c.exact
                else rng.standard_normal((C.KV_SINKS, c.kv_dim))).astype(np.float16)
        i.kc0[:C.KV_SINKS] = sink.view(np.uint16)  # early() loads both rows whatever kv_sink is
        if c.clip:  # a level that clips about 3 values in 10
            q = np.quantile(np.abs(_pre(c, i)), 0.7)
            i.clip = np.float32(max(1.0, np.rint(q))) if c.exact else np.float32(q)
    for k in Inputs.__slots__:
        a = getattr(i, k)
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    for a in i.mats:
        a.setflags(write=False)
    return i


def _xnorm64(c, i):
    x = i.x.astype(np.float64)
    if c.norm:
        x = x * (1.0 / np.sqrt((x * x).sum() / c.n + float(np.float32(i.eps)))) * i.normw.astype(np.float64)
    return x


def _pre(c, i):
    """float64 row values w . x (+ bias), per virtual row, ahead of every epilogue."""
    a = (i.vals @ _xnorm64(c, i)) * i.rscale
    return a + i.bias.astype(np.float64) if i.bias is not None else a


def act_ref(a, act):
    """The oracle's activations (infer.cpp:187-197) in the precision of a."""
    if act == C.SILU:
        return a / (1.0 + np.exp(-a))
    return 0.5 * a * (1.0 + np.tanh(a.dtype.type(GELU_C0) * (a + a.dtype.type(GELU_C1) * a * a * a)))


def _rot(v0, v1, cr, ci):
    return v0 * cr - v1 * ci, v0 * ci + v1 * cr


def _h16(bits):
    return np.asarray(bits, np.uint16).view(np.float16).astype(np.float64)


class Ref:
    """values[name]: float64 array shaped as the buffer; written[name]: the elements the launch writes."""
    __slots__ = ("values", "written", "clipped")


@functools.lru_cache(maxsize=4)
def reference(name):
    """The plain definition of the launch, no kernel structure."""
    c = C.BY_NAME[name]
    i = inputs(name)
    r = Ref()
    r.values, r.written, r.clipped = {}, {}, None
    a = _pre(c, i)
    if c.exact:  # every partial sum of every order is an exact f32
        bound = (np.abs(i.vals) @ np.abs(i.x.astype(np.float64))) * i.rscale
        assert bound.max() + 1020 < 2 ** 24 / 4
    if c.policy not in C.QKV_POLICIES:
        out = np.zeros(i.out0.size)
        w = np.zeros(i.out0.size, bool)
        w[:c.d] = True
        if c.policy == C.GLU:
            out[:c.d] = act_ref(a[:c.d], c.act) * a[c.d:]
        elif c.policy == C.RESIDUAL:
            out[:c.d] = i.out0[:c.d].astype(np.float64) + a
        elif c.policy == C.ADDTO:
            out[:c.d] = i.base.astype(np.float64) + a
        else:
            out[:c.d] = a
        r.values["out"], r.written["out"] = out, w
        return r
    clip = float(i.clip)
    r.clipped = float(np.mean(np.abs(a) > clip))
    a = np.clip(a, -clip, clip)
    Q, KV, hd = c.q_dim, c.kv_dim, c.head_dim
    rope, sink = i.rope.astype(np.float64).reshape(-1, 2), i.rope_sink.astype(np.float64).reshape(-1, 2)
    j = lambda dim: (np.arange(0, dim, 2) % hd) >> 1
    q0, q1 = _rot(a[0:Q:2], a[1:Q:2], rope[j(Q), 0], rope[j(Q), 1])
    k0, k1 = _rot(a[Q:Q + KV:2], a[Q + 1:Q + KV:2], rope[j(KV), 0], rope[j(KV), 1])
    for nm, buf in (("q_out", i.q0), ("raw", i.raw0), ("kcache", i.kc0), ("vcache", i.vc0)):
        r.values[nm], r.written[nm] = np.zeros(buf.shape), np.zeros(buf.shape, bool)
    if c.policy == C.QKVN:
        r.values["raw"][:Q + KV], r.written["raw"][:Q + KV] = a[:Q + KV], True
    else:
        r.values["q_out"][0:Q:2], r.values["q_out"][1:Q:2], r.written["q_out"][:Q] = q0, q1, True
        r.values["kcache"][c.kv_pos, 0::2], r.values["kcache"][c.kv_pos, 1::2] = k0, k1
        r.written["kcache"][c.kv_pos] = True
    r.values["vcache"][c.kv_pos], r.written["vcache"][c.kv_pos] = a[Q + KV:], True
    for row in range(c.kv_sink):  # the sinks' one-position rotation
        s = _h16(i.kc0[row])
        r.values["kcache"][row, 0::2], r.values["kcache"][row, 1::2] = _rot(s[0::2], s[1::2], sink[j(KV), 0],
                                                                          sink[j(KV), 1])
        r.written["kcache"][row] = True
    if c.policy != C.QKVN:
        del r.values["raw"], r.written["raw"]
    return r


def launch_buffers(c):
    """name -> the buffer as the launch finds it (a fresh copy), for the buffers it may write."""
    i = inputs(c.name)
    if c.policy not in C.QKV_POLICIES:
        return dict(out=i.out0.copy())
    b = dict(q_out=i.q0.copy(), kcache=i.kc0.copy(), vcache=i.vc0.copy())
    if c.policy == C.QKVN:
        b["raw"] = i.raw0.copy()
    return b


def _half_ulp16(v):
    """Half an f16 ulp at |v| (normal range; 2^-25 below it)."""
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -14)))
    return 0.5 * np.ldexp(1.0, (e - 10).astype(np.int64))


def check(c, got, tol=None):
    """(untouched, value): untouched -- every element the launch must not write holds its incoming bits;
    value -- exact family: True when every written element has the reference's bits; float family: the
    worst max |got - ref| / (tol max |ref|) over the output vectors (out; q_out; raw; the written K and V
    rows, each with half an f16 ulp of the reference allowed first); inf for a NaN."""
    ref, start = reference(c.name), launch_buffers(c)
    tol = tol or rel_tol(c)
    untouched, same, worst = True, True, 0.0
    for nm, v in ref.values.items():
        g, w = np.asarray(got[nm]), ref.written[nm]
        assert g.shape == start[nm].shape and g.dtype == start[nm].dtype, nm
        bits = np.uint32 if g.dtype == np.float32 else np.uint16
        untouched &= bool(np.array_equal(g.view(bits)[~w], start[nm].view(bits)[~w]))
        if not w.any():
            continue
        f16 = g.dtype == np.uint16
        if c.exact:
            want = v.astype(np.float32).astype(np.float16).view(np.uint16) if f16 else v.astype(np.float32).view(np.uint32)
            same &= bool(np.array_equal(g.view(bits)[w], want[w]))
            continue
        gv = _h16(g) if f16 else g.astype(np.float64)
        vecs = [(gv[r], v[r]) for r in np.flatnonzero(w.any(axis=1))] if f16 else [(gv[w], v[w])]
        for a, b in vecs:
            err = np.abs(a - b) - (_half_ulp16(b) if f16 else 0.0)
            bar = err.max() / (tol * np.abs(b).max())
            worst = float("inf") if np.isnan(bar) else max(worst, float(bar))
    return untouched, (same if c.exact else worst)


# ---------------------------------------------------------------- the traversal model
_L = np.arange(64)
_WAVE_SUM = (_L ^ 1, _L ^ 2, (_L & ~7) | (7 - (_L & 7)), (_L & ~15) | (15 - (_L & 15)), _L ^ 16, _L ^ 32)


def _fma32(a, b, c):
    """f32 fused multiply-add: the product is exact in float64, one rounding to it, one to f32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _wave_sum32(v):
    """device_common.h wave_sum over the last axis (64 lanes) in f32."""
    for p in _WAVE_SUM:
        v = v + v[..., p]
    return v[..., 0]


def xs_at(i, q4):
    """gemv.h xs_at (the place of the float4 that holds element i) + i % 4: where element i of x lies in LDS."""
    return (i & ~2047) + ((i >> 2) & 7) * 256 + ((i >> 5) & 63) * 4 + (i & 3) if q4 else i


def _scale32(x, n, eps, threads, dup):
    """stage_x / stage_x_regs' norm in f32: threads stride float4s, sumsq4 as its fma chain, wave_sum
    per wave, the wave sums added in order. dup: clamped slots past n counted (a defect)."""
    K = -(-n // (4 * threads))
    v = np.zeros(K * threads * 4, np.float32)
    v[:n] = x
    if dup:
        v[n:] = np.tile(x[n - 4:n], (v.size - n) // 4)
    v = v.reshape(K, threads, 4)
    ss = np.zeros(threads, np.float32)
    for k in range(K):
        t = v[k, :, 0] * v[k, :, 0]
        for e in (1, 2, 3):
            t = _fma32(v[k, :, e], v[k, :, e], t)
        ss = ss + t
    red = _wave_sum32(ss.reshape(threads // 64, 64))
    tot = np.float32(0.0)
    for w in range(threads // 64):
        tot = tot + red[w]
    return np.float32(1.0) / np.sqrt(tot / np.float32(n) + np.float32(eps))


def _stage(c, p, i, f32, defect):
    """x as the multiply-adds read it, element k of a row at [k]: staged (rmsnorm'ed) into LDS by
    stage_x or by prefetch_x / stage_x_regs, read back through the type's LDS layout."""
    fl = np.float32 if f32 else np.float64
    n, threads, q4 = c.n, p["threads"], c.dtype == C.Q4
    slots = n  # elements that reach LDS
    xregs = False
    if not p["generic"]:
        t = threads
        if defect == "xregs capacity taken for the wrong thread count":
            t = 256 if threads == 512 else 512
        xregs = n <= C.xcap(c.norm, t)
        if xregs:  # the registers a thread really has: what lies past them is never staged
            slots = min(n, C.xcap(c.norm, threads))
    x = i.x.astype(fl)
    if c.norm:
        dup = xregs and defect == "the norm's sum over clamped duplicates"
        if f32:
            scale = _scale32(i.x, n, i.eps, threads, dup)
            x = x * scale * i.normw
        else:
            ss = (x * x).sum()
            if dup:
                ss += (C.xcap(c.norm, threads) - n) // 4 * (x[n - 4:] ** 2).sum()
            x = x * (1.0 / np.sqrt(ss / n + float(np.float32(i.eps)))) * i.normw.astype(fl)
    lds = np.zeros(C.xs_len(c.dtype, n) + 4096, fl)
    k = np.arange(slots)
    pos = xs_at(k, q4)
    if defect == "xs_at<true> taken as plain for the last partial 2048-block" and q4 and n % 2048:
        pos = np.where(k >= (n & ~2047), k, pos)
    lds[pos] = x[:slots]
    return lds[xs_at(np.arange(n), q4)]


def _weights(c, i, defect):
    """Element values (rows, n) float64 as the kernel pairs them with x (q4: times the group scale it reads)."""
    if c.dtype != C.Q4:
        return i.vals
    s = i.q4s
    if defect == "q4 scale one chunk off":  # chunk c's scales read at chunk c + 1; the row's zero padding past the end
        s = np.concatenate([s[:, 64:], np.zeros((s.shape[0], 64))], axis=1)[:, :s.shape[1]]
    return i.q4u * np.repeat(s, 32, axis=1)


def _chain32(c, i, xe, rows, chunks, lane_ok=None):
    """f32: per segment s the lanes' accumulators over the chunks[s] (-1: none) of weight row rows[s], in
    order -- fma_chunk's single chain per lane, or q4's two chains per block and one scaled add -- then
    wave_sum. lane_ok[s, chunk slot, lane]: lanes that take the chunk (the ragged end)."""
    S, Lc = chunks.shape
    epl, ch = C.EPL[c.dtype], C.CH[c.dtype]
    acc = np.zeros((S, 64), np.float32)
    for ci in range(Lc):
        cidx = chunks[:, ci]
        ok = (cidx >= 0)[:, None] & (lane_ok[:, ci] if lane_ok is not None else True)
        base = np.maximum(cidx, 0)[:, None] * ch + _L[None, :] * epl  # [S, 64]
        if c.dtype == C.Q4:
            a = [np.zeros((S, 64), np.float32), np.zeros((S, 64), np.float32)]
            for e in range(32):
                k = np.minimum(base + e, c.n - 1)
                a[e & 1] = _fma32(i.q4u[rows[:, None], k].astype(np.float32), xe[k], a[e & 1])
            s = i.q4s[rows[:, None], np.minimum(base, c.n - 1) >> 5].astype(np.float32)
            new = _fma32(s, a[0] + a[1], acc)
        else:
            new = acc
            for e in range(epl):
                k = np.minimum(base + e, c.n - 1)
                new = _fma32(i.vals[rows[:, None], k].astype(np.float32), xe[k], new)
        acc = np.where(ok, new, acc)
    return _wave_sum32(acc)


def _vrow(c, g, r):
    """The weight row (in the stacked vals) of row r of group g: P::row."""
    return g + r * c.d if c.policy == C.GLU else g * C.POLICY_R[c.policy] + r


def _generic(c, p, i, xe, f32, defect):
    """gemv_kernel: one group per wave; the U = 4 loop, the chunk-at-a-time tail, the ragged lanes."""
    ch, epl, R, G, n = C.CH[c.dtype], C.EPL[c.dtype], C.POLICY_R[c.policy], c.n_groups, c.n
    nfull, rem = n // ch, n % ch
    chunks = list(range(nfull // 4 * 4 if defect == "generic tail loop skipped" else nfull))
    lanes = _L[(_L + 1) * epl < rem] if defect == "rem lanes off by one" else _L[_L * epl < rem]
    rows = _vrow(c, np.repeat(np.arange(G), R), np.tile(np.arange(R), G))
    if f32:
        ck = np.tile(np.array(chunks + [nfull], np.int64), (rows.size, 1))
        ok = np.ones((rows.size, ck.shape[1], 64), bool)
        ok[:, -1] = np.isin(_L, lanes)[None]
        acc = _chain32(c, i, xe, rows, ck, ok)
    else:
        P = _weights(c, i, defect)[rows] * xe[None, :]
        end = nfull * ch + (lanes.size * epl if lanes.size else 0)
        acc = P[:, :len(chunks) * ch].sum(axis=1) + P[:, nfull * ch:end].sum(axis=1)
    return acc.reshape(G, R), np.ones(G, bool)


def _traverse(rows, ngl, R, nch, W, defect):
    """One workgroup of ngl groups: per wave the items it consumes, as (wave, LDS slot the partial is
    parked in, [(virtual row, chunk), ...]) in the order the partials are stored."""
    segs = []
    for wave in range(W):
        mine = C.wave_mine(rows, ngl, R, nch, W, wave)
        if defect == "whole-row mine rounded down" and rows:
            mine = max((ngl * R - wave) // W, 0) * nch
        if defect == "mine one short":
            mine = max(mine - 1, 0)
        slot = (lambda vr: wave) if defect == "partial slot without the row" else (lambda vr: vr * W + wave)
        if rows:
            vr, ck = wave, 0
        else:
            vr, ck = wave // nch, 0 if defect == "the start cursor's wave % nch dropped" else wave % nch
        cur, items = vr, []
        for _ in range(mine):
            if vr != cur and defect != "the row flush skipped":
                segs.append((wave, slot(cur), items))
                cur, items = vr, []
            items.append((vr, ck))
            if rows:
                ck += 1
                if ck == nch:
                    ck, vr = 0, vr + W
            else:
                ck += W
                if defect == "advance's while as an if":
                    if ck >= nch:
                        ck, vr = ck - nch, vr + 1
                else:
                    vr, ck = vr + ck // nch, ck % nch
        if mine > 0:
            segs.append((wave, slot(cur), items))
    return segs


def _rowblock(c, p, i, xe, f32, defect):
    """gemv_rb_kernel: group g belongs to workgroup g % nb; returns the row sums [n_groups, R] as the
    epilogue's thread adds the parked partials up in wave order, and the groups some workgroup finishes."""
    ch, R, G, n = C.CH[c.dtype], C.POLICY_R[c.policy], c.n_groups, c.n
    nb, W, nch = p["nb"], p["threads"] // 64, n // ch
    acc = np.zeros((G, R), np.float32 if f32 else np.float64)
    done = np.zeros(G, bool)
    if not f32:
        D = (_weights(c, i, defect) * xe[None, :]).reshape(-1, nch, ch).sum(axis=2)  # [rows, nch] chunk dots
    bs = np.arange(nb)
    ngl_b = G // nb + np.zeros(nb, np.int64) if defect == "ngl without the remainder groups" else (G - 1 - bs) // nb + 1
    for ngl in np.unique(ngl_b):
        b = bs[ngl_b == ngl]
        vr = np.arange(ngl * R)
        VR = _vrow(c, b[:, None] + (vr // R)[None, :] * nb, (vr % R)[None, :])  # [B, ngl R] weight rows
        segs = _traverse(bool(p["rows"]), int(ngl), R, nch, W, defect)
        last = {}
        for s, (wave, slot, items) in enumerate(segs):  # a slot keeps what was stored into it last
            last[slot] = s
        keep = [segs[s] for s in sorted(last.values()) if segs[s][1] < ngl * R * W]
        a = np.zeros((b.size, ngl * R), acc.dtype)
        if f32:
            assert defect is None
            part = np.zeros((b.size, ngl * R, W), np.float32)
            Lc = max(len(it) for _, _, it in keep)
            rows_s = np.concatenate([VR[:, it[0][0]] for _, _, it in keep])
            ck = np.concatenate([np.tile(np.array([k for _, k in it] + [-1] * (Lc - len(it))), (b.size, 1))
                                 for _, _, it in keep])
            sums = _chain32(c, i, xe, rows_s, ck).reshape(len(keep), b.size)
            for s, (wave, slot, it) in enumerate(keep):
                part[:, slot // W, slot % W] = sums[s]
            for w in range(W):
                a = a + part[:, :, w]
        else:
            tgt = np.array([slot // W for _, slot, it in keep for vr_, k in it if k < nch], np.int64)
            src = np.array([vr_ for _, slot, it in keep for vr_, k in it if k < nch], np.int64)
            cks = np.array([k for _, slot, it in keep for vr_, k in it if k < nch], np.int64)
            if tgt.size:
                np.add.at(a, (np.arange(b.size)[:, None], tgt[None, :]), D[VR[:, src], cks[None, :]])
        g = b[:, None] + np.arange(ngl)[None, :] * nb
        acc[g] = a.reshape(b.size, ngl, R)
        done[g] = True
    return acc, done


def model(c, p, f32=False, defect=None):
    """The buffers after the launch (as launch_buffers: f32 / uint16 arrays) as the kernel's traversal
    under plan p computes them: float64 arithmetic, or the f32 restatement. defect: one of DEFECTS."""
    assert defect is None or defect in DEFECTS
    i = inputs(c.name)
    fl = np.float32 if f32 else np.float64
    xe = _stage(c, p, i, f32, defect)
    acc, done = (_generic if p["generic"] else _rowblock)(c, p, i, xe, f32, defect)
    R, G, nb, T = C.POLICY_R[c.policy], c.n_groups, p["nb"], p["threads"]
    g = np.arange(G)
    # the epilogue's thread: group gl of workgroup b is finished by thread gl % THREADS, which holds the
    # preloaded residual rows (xr) and row scales (rs) of group gl % THREADS
    first = np.ones(G, bool) if p["generic"] else (g // nb) < T
    gpre = g if p["generic"] else g % nb + ((g // nb) % T) * nb
    rows = _vrow(c, g[:, None], np.arange(R)[None, :])
    rs_g = np.where(first | (defect == "rs used for gl >= THREADS"), gpre, g)
    acc = (acc * i.rscale[_vrow(c, rs_g[:, None], np.arange(R)[None, :])].astype(fl)).astype(fl)
    out = launch_buffers(c)
    gd = g[done]
    if c.policy not in C.QKV_POLICIES:
        o = out["out"]
        if c.policy == C.GLU:
            o[gd] = (act_ref(acc[gd, 0], c.act) * acc[gd, 1]).astype(np.float32)
        elif c.policy == C.RESIDUAL:
            xr_g = np.where(first | (defect == "xr used for gl >= THREADS"), gpre, g)
            o[gd] = (i.out0[xr_g[gd]].astype(fl) + acc[gd, 0]).astype(np.float32)
        elif c.policy == C.ADDTO:
            o[gd] = (i.base[gd].astype(fl) + acc[gd, 0]).astype(np.float32)
        else:
            o[rows[gd].reshape(-1)] = acc[gd].reshape(-1).astype(np.float32)
        return out
    # ---- PQKV / PQKVB / PQKVN::finish
    Q, KV, hd = c.q_dim, c.kv_dim, c.head_dim
    clip = fl(i.clip)
    a = acc
    if c.policy == C.QKVB and defect != "bias after the clip":
        a = a + i.bias.reshape(G, 2).astype(fl)
    a = np.clip(a, -clip, clip)
    if c.policy == C.QKVB and defect == "bias after the clip":
        a = a + i.bias.reshape(G, 2).astype(fl)
    tab = np.zeros((2, 2 * max(hd, Q) + 512), fl)  # StepState: rope[256], rope_sink[256], then what follows as 0
    tab[0, :hd], tab[0, 256:256 + hd] = i.rope, i.rope_sink
    tab[1, :hd] = i.rope_sink
    krow = step_pos(c) if defect == "K at row pos instead of kv_pos" else c.kv_pos
    f16 = lambda v: np.asarray(v, fl).astype(np.float32).astype(np.float16).view(np.uint16)
    for gg in gd:
        vr = 2 * gg
        v0, v1 = a[gg]
        isv = vr >= Q + KV
        if isv and defect != "V rotated":
            out["vcache"][c.kv_pos, vr - Q - KV:vr - Q - KV + 2] = f16([v0, v1])
            continue
        ii = vr if vr < Q else (vr - Q if vr < Q + KV else vr - Q - KV)
        if c.policy == C.QKVN and not isv:
            at = ii if defect == "raw indexed per matrix instead of 2g" else vr
            out["raw"][at:at + 2] = np.asarray([v0, v1], np.float32)
            continue
        j = ii >> 1 if defect == "rope index without % head_dim" else (ii % hd) >> 1
        r0, r1 = _rot(v0, v1, tab[0, 2 * j], tab[0, 2 * j + 1])
        if isv:
            out["vcache"][c.kv_pos, ii:ii + 2] = f16([r0, r1])
        elif vr < Q:
            out["q_out"][ii:ii + 2] = np.asarray([r0, r1], np.float32)
        else:
            out["kcache"][krow, ii:ii + 2] = f16([r0, r1])
    # ---- early / late: thread t of workgroup b starts at pair t nb + b and strides by threads nb
    half = KV // 2
    npairs = (C.KV_SINKS if defect == "sink rotation when kv_sink = 0" else c.kv_sink) * half
    pi = np.arange(min(npairs, T * nb) if defect == "late as an if" else npairs)
    if pi.size:
        row, col = pi // half, 2 * (pi % half)
        v0, v1 = _h16(i.kc0[row, col]).astype(fl), _h16(i.kc0[row, col + 1]).astype(fl)
        t = tab[0 if defect == "sink rotation with rope" else 1]
        j = (col % hd) >> 1
        o0, o1 = _rot(v0, v1, t[2 * j], t[2 * j + 1])
        out["kcache"][row, col], out["kcache"][row, col + 1] = f16(o0), f16(o1)
    return out
