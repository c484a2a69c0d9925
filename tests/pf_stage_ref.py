"""Inputs, float64 references and the checker of the prefill stage tests (pf_stage_cases.py), shared by
test_pf_stage_cpu.py and test_gpu_pf_stage.py. TEST INFRASTRUCTURE ONLY; needs no library.

inputs(case)     deterministic per case name: the keyword arguments of runtime.prefill_stage (every
                 buffer the stage may write filled with 0xA5 bytes, or the residual's start) and what
                 the reference needs.
reference(case)  each stage from its definition in float64 (infer.cpp statement order where the
                 kernels' headers cite it): rmsnorm (infer.cpp:134-144), QKV + clip + RoPE + cache rows
                 (infer.cpp:280-301), the residual add, the GLU (infer.cpp:183-189 activations), and
                 log softmax of the target (sampler.cpp:11-25). Not written from the kernels.
check(case, got) (untouched, value): whether everything the launch must not write kept its bytes, and
                 for an exact case whether the outputs are the reference's bits, for a float case the
                 worst error in bars.
emulate(case, wrong=None)  an honest f32 evaluation in the kernels' order (K splits, vocab tiles, wave
                 partials, exp2 on a log2(e)-scaled FMA), in the form of `got`; with wrong=<name> one
                 of the deliberately wrong kernels of WRONG, which check must reject.

Bars. An f16 output: half an f16 ulp of the reference plus REL_TOL = 2e-5 of the row's largest
|reference| (test_gpu_kernels.py, gemv_ref.rel_tol); an f32 output: REL_TOL of the row's largest
|reference|. Measured here (test_pf_stage_cpu.py: the worst error of emulate() against the float64
reference over all cases) and multiplied by 5:
  LP_ATOL     log p of the target, nats         measured 6.29e-6 -> bar 3.2e-5 (<= 1e-4 as required)
  PSUM_REL    a tile's sum of exp, relative     measured 6.24e-6 -> bar 3.2e-5
  RECON_REL   the norm's hi + lo against y, of the row's largest |y|   measured 2.06e-7 -> bar 1.1e-6
"""
import zlib

import numpy as np

import pf_stage_cases as C

REL_TOL = 2e-5
LP_ATOL = 3.2e-5
PSUM_REL = 3.2e-5
RECON_REL = 1.1e-6
L2E32 = np.float32(1.4426950408889634)
ROPE_THETA = 10000.0


def sent(shape, dt):
    a = np.empty(shape, dt)
    a.view(np.uint8)[...] = 0xA5
    return a


def is_sent(a):
    return bool(np.all(np.ascontiguousarray(a).view(np.uint8) == 0xA5))


def ulp16(x):
    """The f16 ulp at |x| (float64 array): 2^-24 in the subnormal range."""
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -14)))
    return 2.0 ** (np.minimum(e, 15) - 10)


def h16(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x).astype(np.float16)


def bits16(x):
    return h16(x).view(np.uint16)


class Inputs:
    pass


_cache = {}


def inputs(c):
    if c.name not in _cache:
        i = Inputs()
        i.rng = np.random.default_rng(zlib.crc32(c.name.encode()))
        (_in_norm, _in_qkv, _in_res, _in_glu, _in_lp)[c.stage](c, i)
        i.ref = (_ref_norm, _ref_qkv, _ref_res, _ref_glu, _ref_lp)[c.stage](c, i)
        del i.rng
        _cache[c.name] = i
    return _cache[c.name]


def reference(c):
    return inputs(c).ref


def _ints(rng, lo, hi, shape, nonzero=False):
    a = rng.integers(lo, hi + 1, shape)
    if nonzero:
        a[a == 0] = hi
    return a.astype(np.float64)


def _a_operand(c, i, T, K, both, amp=3, lo_amp=2):
    """The A operand as f16 values [T][K] (hi) or [T][2 K] ([hi | lo]); i.a_hi / i.a_lo float64."""
    if c.exact or c.stage == C.GLU:
        i.a_hi = _ints(i.rng, -amp, amp, (T, K))
        i.a_lo = _ints(i.rng, -lo_amp, lo_amp, (T, K), nonzero=True)
    else:
        v = i.rng.standard_normal((T, K))
        i.a_hi = h16(v).astype(np.float64)
        i.a_lo = h16(v - i.a_hi).astype(np.float64)
        i.a_lo[i.a_lo == 0] = 2.0 ** -14
    if not both:
        i.a_lo = np.zeros_like(i.a_hi)
        return h16(i.a_hi)
    return h16(np.concatenate([i.a_hi, i.a_lo], axis=1))


# ---------------------------------------------------------------- NORM
def _in_norm(c, i):
    T, dim, sp = c.T, c.dim, 2 if c.split else 1
    rng = i.rng
    if c.mode == "gauss":
        x = (rng.standard_normal((T, dim)) * np.exp2(rng.integers(-4, 5, (T, 1)))).astype(np.float32)
        w = (1.0 + 0.3 * rng.standard_normal(dim)).astype(np.float32)
        i.eps = 1e-5
    else:  # rows of +-2^k, eps 0: the scale is the exact 2^-k, y = +-w
        x = (np.exp2(rng.integers(-3, 4, (T, 1))) * rng.choice([-1.0, 1.0], (T, dim))).astype(np.float32)
        w = (_ints(rng, -2 ** 15, 2 ** 15, dim, nonzero=True) * 2.0 ** -13).astype(np.float32)  # 16 bits: lo != 0
        i.eps = 0.0
        if c.mode == "big":
            w[7] = 196608.0
        if c.mode == "nan":
            x[2, 5] = np.nan
    i.x, i.w = x, w
    i.kw = dict(T=T, cus=c.cus, split=c.split, dim=dim, x=x, normw=w, eps=i.eps, xn=sent((T + 2, sp * dim), np.uint16),
                xn_rows=T + 2, range=np.zeros(1, np.uint32))


def _ref_norm(c, i):
    x = i.x.astype(np.float64)
    with np.errstate(invalid="ignore"):
        y = x * (1.0 / np.sqrt(np.mean(x * x, axis=1, keepdims=True) + i.eps)) * i.w.astype(np.float64)
    slot = 0
    ymax = np.where(np.isnan(y), np.inf, np.abs(y)).max()
    if not ymax < 65504.0:
        slot = int(np.float32(ymax).view(np.uint32))
    return dict(y=y, slot=slot)


# ---------------------------------------------------------------- QKV
ROPE_EXACT = [(1, 0), (-1, 0), (0, 1), (0, -1), (.5, .5), (-.5, .5), (.5, -.5), (-.5, -.5)]


def _in_qkv(c, i):
    T, dim, rng, sp = c.T, c.dim, i.rng, 2 if c.split else 1
    wide = getattr(c, "wide", False)
    a = _a_operand(c, i, T, dim, True, amp=7 if wide else 3)
    n = c.q_dim + 2 * c.kv_dim
    half = c.head_dim // 2
    if c.exact:
        w = _ints(rng, -3, 3, (n, dim))
        bias = _ints(rng, -40, 40, n)
        if wide:
            bias[:c.q_dim] = rng.choice([-1.0, 1.0], c.q_dim) * _ints(rng, 2500, 3400, c.q_dim)
        i.clip = 3300.0 if wide else float(int(2.5 * np.sqrt(dim)))
        rope = np.array(ROPE_EXACT, np.float64)[rng.integers(0, 8, (T, half))]
    else:
        w = h16(rng.standard_normal((n, dim)) / np.sqrt(dim)).astype(np.float64)
        bias = 0.5 * rng.standard_normal(n)
        i.clip = 1.5
        ang = (c.pos0 + np.arange(T))[:, None] * ROPE_THETA ** (-2.0 * np.arange(half) / c.head_dim)[None, :]
        rope = np.stack([np.cos(ang), np.sin(ang)], axis=-1)
    i.w = w
    i.bias = bias.astype(np.float32).astype(np.float64) if c.bias else np.zeros(n)
    i.rope = rope.astype(np.float32)
    i.cache_rows = c.pos0 + T + 2
    w16 = h16(w)
    b32 = i.bias.astype(np.float32)
    i.kw = dict(T=T, cus=c.cus, split=c.split, dim=dim, a=a, n_heads=c.n_heads, n_kv_heads=c.n_kv_heads,
                head_dim=c.head_dim, pos0=c.pos0, q_rows=T + 3, cache_rows=i.cache_rows, clip=i.clip,
                wq=w16[:c.q_dim], wk=w16[c.q_dim:c.q_dim + c.kv_dim], wv=w16[c.q_dim + c.kv_dim:], rope=i.rope,
                q=sent((T + 3, sp * c.q_dim), np.uint16), kc=sent((i.cache_rows, c.kv_dim), np.uint16),
                vc=sent((i.cache_rows, c.kv_dim), np.uint16), range=np.zeros(1, np.uint32))
    if c.bias:
        i.kw.update(bq=b32[:c.q_dim], bk=b32[c.q_dim:c.q_dim + c.kv_dim], bv=b32[c.q_dim + c.kv_dim:])


def _rope(v, rope, head_dim, sign=1.0):
    """infer.cpp:291-301 on (even, odd) column pairs of every head: v [T][n], rope [T][half][2]."""
    T, n = v.shape
    p = v.reshape(T, n // head_dim, head_dim // 2, 2)
    cs, sn = rope[:, None, :, 0], sign * rope[:, None, :, 1]
    out = np.stack([p[..., 0] * cs - p[..., 1] * sn, p[..., 0] * sn + p[..., 1] * cs], axis=-1)
    return out.reshape(T, n)


def _ref_qkv(c, i):
    aq = i.a_hi + i.a_lo if c.split else i.a_hi
    akv = i.a_hi + i.a_lo
    qd, kd = c.q_dim, c.kv_dim
    v = np.concatenate([aq @ i.w[:qd].T, akv @ i.w[qd:].T], axis=1) + i.bias
    v = np.clip(v, -i.clip, i.clip)
    rope = i.rope.astype(np.float64)
    q, k, vv = _rope(v[:, :qd], rope, c.head_dim), _rope(v[:, qd:qd + kd], rope, c.head_dim), v[:, qd + kd:]
    return dict(q=q, k=k, v=vv, slot=0)


# ---------------------------------------------------------------- RESIDUAL
def _in_res(c, i):
    T, rng = c.T, i.rng
    a = _a_operand(c, i, T, c.k, bool(c.split))
    if c.exact:
        w = _ints(rng, -3, 3, (c.n, c.k))
        x0 = _ints(rng, -1000, 1000, (T, c.n))
    else:
        w = h16(rng.standard_normal((c.n, c.k)) / np.sqrt(c.k)).astype(np.float64)
        x0 = rng.standard_normal((T, c.n)).astype(np.float32).astype(np.float64)
    i.w, i.x0 = w, x0
    xres = sent((T + 3, c.n), np.float32)
    xres[:T] = x0
    i.kw = dict(T=T, cus=c.cus, split=c.split, a=a, kind=c.kind, n=c.n, k=c.k, x_rows=T + 3, w=h16(w), scale=c.scale,
                xres=xres)


def _ref_res(c, i):
    return dict(x=i.x0 + c.scale * ((i.a_hi + i.a_lo) @ i.w.T))


# ---------------------------------------------------------------- GLU
def act64(act, x):
    """infer.cpp:183-189."""
    if act == C.SILU:
        with np.errstate(over="ignore"):
            return x / (1.0 + np.exp(-x))
    return 0.5 * x * (1.0 + np.tanh(0.797885 * (x + 0.044715 * x * x * x)))


def _in_glu(c, i):
    T, rng, sp = c.T, i.rng, 2 if c.split else 1
    a = _a_operand(c, i, T, c.dim, bool(c.split), amp=c.amp, lo_amp=1)
    i.w1, i.w3 = _ints(rng, -c.amp, c.amp, (c.hidden, c.dim)), _ints(rng, -c.amp, c.amp, (c.hidden, c.dim))
    i.kw = dict(T=T, cus=c.cus, split=c.split, dim=c.dim, a=a, hidden=c.hidden, act=c.act, h_rows=T + 3, w1=h16(i.w1),
                w3=h16(i.w3), hscale=c.hscale, h=sent((T + 3, sp * c.hidden), np.uint16), range=np.zeros(1, np.uint32))


def _ref_glu(c, i):
    ae = i.a_hi + i.a_lo
    x1, x3 = ae @ i.w1.T, ae @ i.w3.T
    v = act64(c.act, x1) * x3
    vmax = np.abs(v).max()
    over = vmax * c.hscale >= 65504.0
    return dict(x1=x1, x3=x3, v=v, over=bool(over), vmax=vmax)


# ---------------------------------------------------------------- LOGPROB
LP_MAX, LP_UNDER = 70.0, -110.0


def lp_wave_cols(c):
    """Columns of one wave's partial in the logits epilogue (TN) for the case's tile."""
    e = C.expect(c)
    bn = e["bn"][0]
    return bn, bn // (4 if (e["eight_phase"] or bn != 128) else 2)


def _in_lp(c, i):
    T, K, V, rng = c.T, c.dim, c.vocab, i.rng
    bn, tn = lp_wave_cols(c)
    nt = V // bn
    a = _a_operand(c, i, T, K, bool(c.split), amp=1, lo_amp=1)
    if c.exact:
        # logit[m][n] = off[n] + noise: A column 0 is 1 (lo 0), W column 0 the offset; tiles differ widely in
        # maximum (a stale partial shows), one tile is far below everything (its contribution underflows
        # to 0), the row maximum LP_MAX stands noise-free in two tiles, neither the target's
        i.a_hi[:, 0], i.a_lo[:, 0] = 1.0, 0.0
        a = h16(np.concatenate([i.a_hi, i.a_lo], axis=1)) if c.split else h16(i.a_hi)
        w = _ints(rng, -1, 1, (V, K))
        off = np.repeat(np.array([10.0, -30.0, 5.0, -60.0, 0.0, -15.0])[np.arange(nt) % 6], bn)
        i.under = min(3, nt - 1)
        off[i.under * bn:(i.under + 1) * bn] = LP_UNDER
        w[i.under * bn:(i.under + 1) * bn, 1:] = 0
        i.maxcols = [1 * bn + 5 if nt > 1 else 5, (nt - 1) * bn + bn // 2]
        w[i.maxcols, 1:] = 0
        off[i.maxcols] = LP_MAX
        w[:, 0] = off
    else:
        w = h16(rng.standard_normal((V, K)) * (3.0 / np.sqrt(K))).astype(np.float64)
        i.under, i.maxcols = min(3, nt - 1), [bn + 5 if nt > 1 else 5]
    i.w = w
    # targets: a tile's last column first (row 0), column 0, a tile's first column, both sides of a wave-column
    # boundary, V - 1, none, inside the far-below tile, the maximum's column; the last row has none
    pat = [bn - 1, 0, bn % V, tn - 1, tn, V - 1, -1, i.under * bn + 7, i.maxcols[0], 2 * bn - 1 if nt > 1 else bn - 2]
    tg = np.array([pat[m % len(pat)] for m in range(T)], np.int32)
    if T > 1:
        tg[T - 1] = -1
    i.targets = tg
    i.kw = dict(T=T, cus=c.cus, split=c.split, dim=K, a=a, vocab=V, wcls=h16(w), targets=tg, lp=sent(T, np.float32),
                pmax=sent(T * (V // 128), np.float32), psum=sent(T * (V // 128), np.float32),
                tgt_logit=sent(T, np.float32))


def _ref_lp(c, i):
    bn, _ = lp_wave_cols(c)
    lg = (i.a_hi + i.a_lo) @ i.w.T
    T, V = lg.shape
    t3 = lg.reshape(T, V // bn, bn)
    pmax = t3.max(axis=2)
    psum = np.exp(t3 - pmax[:, :, None]).sum(axis=2)
    M = lg.max(axis=1)
    lse = M + np.log(np.exp(lg - M[:, None]).sum(axis=1))
    has = i.targets >= 0
    tl = lg[np.arange(T), np.maximum(i.targets, 0)]
    return dict(logits=lg, pmax=pmax, psum=psum, tgt=tl, lp=np.where(has, tl - lse, 0.0), has=has)


# ---------------------------------------------------------------- check
def _bars16(got_bits, ref, rowmax=None):
    """What |got - ref| has beyond half an f16 ulp of ref, in bars of REL_TOL of the row's largest |ref|, worst
    element: <= 1 exactly when |got - ref| <= half an ulp + REL_TOL rowmax (a correctly rounded output
    uses the half ulp whole, so the margin is counted on the rest). Where the reference rounds to inf
    (|ref| >= 65520) the output must be that inf; inside the bar of that edge either is right."""
    got = np.ascontiguousarray(got_bits).view(np.float16).astype(np.float64)
    rowmax = np.abs(ref).max(axis=1, keepdims=True) if rowmax is None else rowmax
    half, bar = 0.5 * ulp16(ref), REL_TOL * rowmax
    big = np.abs(ref) >= 65520.0 - bar
    with np.errstate(invalid="ignore"):
        err = np.where(big & np.isinf(got) & (np.sign(got) == np.sign(ref)), 0.0,
                       np.maximum(np.abs(got - ref) - half, 0.0) / bar)
    err = np.where(np.isnan(err), np.inf, err)
    return float(err.max())


def check(c, got):
    i = inputs(c)
    r, T = i.ref, c.T
    ok, exact, bars = True, True, 0.0
    eqb = lambda bits, ref: bool(np.array_equal(np.ascontiguousarray(bits).view(np.uint16), bits16(ref)))
    if c.stage == C.NORM:
        xn, dim = got["xn"], c.dim
        ok = is_sent(xn[T:])
        hi = xn[:T, :dim]
        hv = hi.view(np.float16).astype(np.float32)
        if c.exact:
            nanrow = np.isnan(r["y"]).any(axis=1)
            y32 = r["y"].astype(np.float32)  # exact: y has 16 significant bits
            exact = eqb(hi[~nanrow], y32[~nanrow]) and bool(np.isnan(hv[nanrow]).all())
            if c.split:
                lo = xn[:T, dim:]
                with np.errstate(invalid="ignore"):
                    exact = exact and eqb(lo[~nanrow], (y32 - hv)[~nanrow]) and bool(
                        np.isnan(lo.view(np.float16)[nanrow]).all())
        else:
            bars = _bars16(hi, r["y"])
            if c.split:
                rec = hv.astype(np.float64) + xn[:T, dim:].view(np.float16).astype(np.float64)
                bars = max(bars, float((np.abs(rec - r["y"]) / (RECON_REL * np.abs(r["y"]).max(axis=1, keepdims=True))).max()))
        exact = exact and int(got["range"][0]) == r["slot"]
        bars = bars if int(got["range"][0]) == r["slot"] else np.inf
    elif c.stage == C.QKV:
        q, kc, vc, qd, p0 = got["q"], got["kc"], got["vc"], c.q_dim, c.pos0
        rows = np.r_[0:p0, p0 + T:i.cache_rows]
        ok = is_sent(q[T:]) and is_sent(kc[rows]) and is_sent(vc[rows])
        qhi = q[:T, :qd]
        qhv = qhi.view(np.float16).astype(np.float64)
        if c.exact:
            exact = eqb(qhi, r["q"]) and eqb(kc[p0:p0 + T], r["k"]) and eqb(vc[p0:p0 + T], r["v"])
            if c.split:
                exact = exact and eqb(q[:T, qd:], r["q"] - qhv)
                if getattr(c, "wide", False):
                    assert np.any(q[:T, qd:] & 0x7FFF), "the wide case must have lo != 0"
        else:
            bars = max(_bars16(qhi, r["q"]), _bars16(kc[p0:p0 + T], r["k"]), _bars16(vc[p0:p0 + T], r["v"]))
            if c.split:
                rec = qhv + q[:T, qd:].view(np.float16).astype(np.float64)
                bar = REL_TOL * np.abs(r["q"]).max(axis=1, keepdims=True)  # (lo's own half ulp: 2^-24 |q|)
                bars = max(bars, float((np.maximum(np.abs(rec - r["q"]) - 2.0 ** -24 * np.abs(r["q"]), 0) / bar).max()))
        exact = exact and int(got["range"][0]) == 0
        bars = bars if int(got["range"][0]) == 0 else np.inf
    elif c.stage == C.RESIDUAL:
        x = got["xres"]
        ok = is_sent(x[T:])
        if c.exact:
            exact = bool(np.array_equal(x[:T].view(np.uint32), r["x"].astype(np.float32).view(np.uint32)))
        else:
            bars = float((np.abs(x[:T].astype(np.float64) - r["x"]) / (REL_TOL * np.abs(r["x"]).max(axis=1, keepdims=True))).max())
    elif c.stage == C.GLU:
        h, hid = got["h"], c.hidden
        ok = is_sent(h[T:])
        vs = r["v"] * c.hscale
        rowmax = np.minimum(np.abs(vs).max(axis=1, keepdims=True), 65504.0)
        bars = _bars16(h[:T, :hid], vs, rowmax)
        if c.split:
            hv = h[:T, :hid].view(np.float16).astype(np.float64)
            fin = np.isfinite(hv)
            rec = hv + h[:T, hid:].view(np.float16).astype(np.float64)
            half = 2.0 ** -24 * np.maximum(np.abs(vs), 2.0 ** -14)  # lo's own half ulp
            bars = max(bars, float(np.where(fin, np.maximum(np.abs(rec - vs) - half, 0) / (REL_TOL * rowmax), 0.0).max()))
        slot = np.array([got["range"][0]], np.uint32).view(np.float32)[0]
        if r["over"]:
            bars = max(bars, abs(float(slot) - r["vmax"]) / (REL_TOL * r["vmax"]))
        elif got["range"][0] != 0:
            bars = np.inf
    else:
        bn, _ = lp_wave_cols(c)
        nt = c.vocab // bn
        pm, ps = got["pmax"], got["psum"]
        has = r["has"]
        ok = is_sent(pm[T * nt:]) and is_sent(ps[T * nt:]) and is_sent(got["tgt_logit"][~has])
        ok = ok and bool(np.all(got["lp"][~has].view(np.uint32) == 0))
        pm, ps = pm[:T * nt].reshape(T, nt).astype(np.float64), ps[:T * nt].reshape(T, nt).astype(np.float64)
        tl, lp = got["tgt_logit"][has].astype(np.float64), got["lp"][has].astype(np.float64)
        with np.errstate(invalid="ignore"):
            bars = max(float((np.abs(ps - r["psum"]) / (PSUM_REL * r["psum"])).max()),
                       float((np.abs(lp - r["lp"][has]) / LP_ATOL).max()) if has.any() else 0.0)
            if c.exact:
                exact = bool(np.array_equal(pm, r["pmax"]) and np.array_equal(tl, r["tgt"][has])) and bars <= 1.0
            else:
                lmax = np.abs(r["logits"]).max(axis=1)
                bars = max(bars, float((np.abs(pm - r["pmax"]) / (REL_TOL * lmax[:, None])).max()),
                           float((np.abs(tl - r["tgt"][has]) / (REL_TOL * lmax[has])).max()) if has.any() else 0.0)
        bars = np.inf if np.isnan(bars) else bars
    return ok, (bool(exact) if c.exact else float(bars))


# ---------------------------------------------------------------- the f32 evaluation in the kernels' order
WRONG = {
    "rope_sign": (C.QKV, "RoPE partner sign swapped"),
    "rope_row": (C.QKV, "RoPE row m taken as m - 1"),
    "bias_kv": (C.QKV, "bias of the k region applied to v"),
    "clip_after": (C.QKV, "clip applied after RoPE"),
    "cache_row": (C.QKV, "cache rows written at m instead of pos0 + m"),
    "q_hilo": (C.QKV, "q columns summed over [hi | lo]"),
    "kv_hi": (C.QKV, "k | v summed over hi only"),
    "ks2": (C.QKV, "skinny reduce summing KS where KS2 is due"),
    "glu_swap": (C.GLU, "GLU W1 / W3 halves swapped"),
    "hscale_lo": (C.GLU, "hscale ignored in the lo half"),
    "scale_x": (C.RESIDUAL, "residual scale applied to x as well as to C"),
    "rows_T": (C.RESIDUAL, "residual written for rows >= T"),
    "tgt_last_col": (C.LOGPROB, "target logit dropped at a tile's last column"),
    "stale_tile": (C.LOGPROB, "one tile's (max, sum) taken from the previous tile"),
    "stop256": (C.LOGPROB, "logprob_kernel stopping at 256 tiles"),
    "lo_dropped": (C.NORM, "norm lo dropped"),
}

f32 = np.float32


def _mm32(a, w, ks=1):
    """a [T][K] . w [N][K]^T in f32, the K range cut into ks chunks summed in order (the skinny reduce)."""
    K = a.shape[1]
    out = np.zeros((a.shape[0], w.shape[0]), f32)
    for s in range(ks):
        sl = slice(s * K // ks, (s + 1) * K // ks)
        out = out + a[:, sl].astype(f32) @ w[:, sl].astype(f32).T
    return out


def _split16(v32):
    with np.errstate(invalid="ignore", over="ignore"):
        hi = v32.astype(np.float16)
        lo = (v32 - hi.astype(f32)).astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16)


def emulate(c, wrong=None):
    assert wrong is None or WRONG[wrong][0] == c.stage
    i = inputs(c)
    kw, T, e = i.kw, c.T, C.expect(c)
    got = {k: np.array(kw[k], copy=True) for k in ("range", "xn", "q", "kc", "vc", "xres", "h", "lp", "pmax", "psum",
                                                   "tgt_logit") if k in kw}
    if c.stage == C.NORM:
        x, dim = i.x, c.dim
        with np.errstate(invalid="ignore", over="ignore"):
            ss = (x * x).sum(axis=1, dtype=f32, keepdims=True)
            scale = f32(1.0) / np.sqrt(ss / f32(dim) + f32(i.eps), dtype=f32)
            y = x * scale * i.w
        hi, lo = _split16(y)
        got["xn"][:T, :dim] = hi
        if c.split:
            got["xn"][:T, dim:] = 0 if wrong == "lo_dropped" else lo
        ymax = np.where(np.isnan(y), np.inf, np.abs(y)).max()
        if not ymax < 65504.0:
            got["range"][0] = f32(ymax).view(np.uint32)
    elif c.stage == C.QKV:
        qd, kd, p0, hd = c.q_dim, c.kv_dim, c.pos0, c.head_dim
        hi, lo, w = i.a_hi.astype(f32), i.a_lo.astype(f32), i.w.astype(f32)
        ks = max(1, e["ks"])
        both = np.concatenate([hi, lo], axis=1)
        w2 = np.concatenate([w, w], axis=1)  # the B wrap
        q_both = bool(c.split) != (wrong == "q_hilo")
        q = _mm32(both, w2[:qd], 2 * ks) if q_both else _mm32(hi, w[:qd], ks)
        if wrong == "kv_hi":
            kv = _mm32(hi, w[qd:], ks)
        elif wrong == "ks2" and e["skinny"]:
            kv = _mm32(both[:, :both.shape[1] // 2], w2[qd:, :both.shape[1] // 2], ks)  # the first KS of 2 KS chunks
        else:
            kv = _mm32(both, w2[qd:], 2 * ks)
        bias = i.bias.astype(f32).copy()
        if wrong == "bias_kv":
            bias[qd + kd:] = bias[qd:qd + kd]
        v = np.concatenate([q, kv], axis=1) + bias
        clip = f32(i.clip)
        rope = i.rope
        if wrong == "rope_row":
            rope = rope[np.maximum(np.arange(T) - 1, 0)]
        sign = f32(-1.0 if wrong == "rope_sign" else 1.0)
        if wrong != "clip_after":
            v = np.clip(v, -clip, clip)
        qo, ko, vo = _rope(v[:, :qd], rope, hd, sign), _rope(v[:, qd:qd + kd], rope, hd, sign), v[:, qd + kd:]
        if wrong == "clip_after":
            qo, ko, vo = (np.clip(t, -clip, clip) for t in (qo, ko, vo))
        qh, ql = _split16(qo.astype(f32))
        got["q"][:T, :qd] = qh
        if c.split:
            got["q"][:T, qd:] = ql
        r0 = 0 if wrong == "cache_row" else p0
        got["kc"][r0:r0 + T] = bits16(ko.astype(f32))
        got["vc"][r0:r0 + T] = bits16(vo.astype(f32))
    elif c.stage == C.RESIDUAL:
        a = np.concatenate([i.a_hi, i.a_lo], axis=1) if c.split else i.a_hi
        w = np.concatenate([i.w, i.w], axis=1) if c.split else i.w
        acc = _mm32(a, w, max(1, e["ks"]))
        x0 = i.x0.astype(f32)
        got["xres"][:T] = (x0 * f32(c.scale) if wrong == "scale_x" else x0) + acc * f32(c.scale)
        if wrong == "rows_T":
            got["xres"][T] = got["xres"][T - 1]
    elif c.stage == C.GLU:
        a = np.concatenate([i.a_hi, i.a_lo], axis=1) if c.split else i.a_hi
        cat = (lambda m: np.concatenate([m, m], axis=1)) if c.split else (lambda m: m)
        w1, w3 = (i.w3, i.w1) if wrong == "glu_swap" else (i.w1, i.w3)
        x1, x3 = _mm32(a, cat(w1), max(1, e["ks"])), _mm32(a, cat(w3), max(1, e["ks"]))
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            if c.act == C.SILU:  # act_fast: hardware exp2 and reciprocal
                g = x1 * (f32(1.0) / (f32(1.0) + np.exp2(f32(-1.4426950408889634) * x1, dtype=f32)))
            else:
                y = f32(0.797885) * (x1 + f32(0.044715) * x1 * x1 * x1)
                t = f32(1.0) - f32(2.0) * (f32(1.0) / (np.exp2(f32(2.8853900817779268) * y, dtype=f32) + f32(1.0)))
                g = f32(0.5) * x1 * (f32(1.0) + t)
            v = (g * x3).astype(f32)
            vs = v * f32(c.hscale)
            hi, lo = _split16(vs)
            if wrong == "hscale_lo":
                lo = (v - hi.view(np.float16).astype(f32)).astype(np.float16).view(np.uint16)
        got["h"][:T, :c.hidden] = hi
        if c.split:
            got["h"][:T, c.hidden:] = lo
        vmax = np.abs(v).max()
        if not vmax * f32(c.hscale) < 65504.0:
            got["range"][0] = f32(vmax).view(np.uint32)
    else:
        bn, tn = lp_wave_cols(c)
        V = c.vocab
        nt = V // bn
        a = np.concatenate([i.a_hi, i.a_lo], axis=1) if c.split else i.a_hi
        w = np.concatenate([i.w, i.w], axis=1) if c.split else i.w
        lg = _mm32(a, w)
        wv = lg.reshape(T, nt, bn // tn, tn)  # [row][tile][wave][col]
        wmx = wv.max(axis=3)
        with np.errstate(under="ignore"):
            arg = (wv.astype(np.float64) * np.float64(L2E32) - (wmx * L2E32).astype(np.float64)[..., None]).astype(f32)
            ws = np.exp2(arg, dtype=f32).sum(axis=3, dtype=f32)
            pmax = wmx.max(axis=2)
            psum = (ws * np.exp(wmx - pmax[:, :, None], dtype=f32)).sum(axis=2, dtype=f32)
            if wrong == "stale_tile":
                pmax[:, 1:], psum[:, 1:] = pmax[:, :-1].copy(), psum[:, :-1].copy()
            n_used = min(nt, 256) if wrong == "stop256" else nt
            M = pmax[:, :n_used].max(axis=1)
            S = (psum[:, :n_used] * np.exp(pmax[:, :n_used] - M[:, None], dtype=f32)).sum(axis=1, dtype=f32)
        tg = i.targets
        has = tg >= 0
        tl = got["tgt_logit"]
        wr = has & ~((tg % bn == bn - 1) if wrong == "tgt_last_col" else np.zeros(T, bool))
        tl[wr] = lg[np.arange(T), np.maximum(tg, 0)][wr]
        with np.errstate(invalid="ignore"):
            got["lp"][:] = np.where(has, tl - M - np.log(S, dtype=f32), f32(0.0))
        got["pmax"][:T * nt], got["psum"][:T * nt] = pmax.ravel(), psum.ravel()
    return got
