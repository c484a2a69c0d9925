"""Inputs, float64 references and a numpy model of the kernel's traversal for the multi-row GEMV
tests (rows_cases.py has the cases). TEST INFRASTRUCTURE ONLY; needs no library.

Two input families, every case seeded by its name:
  exact (RStore / RResidual without the norm): weights are integers in -3 .. 3 (each exact in f16
    and E5M2), x is integers in -4 .. 4 times 1, 2, 4, 8 for row 0 .. 3, the residual starts at
    integers below 1000. Every partial sum of every order is then an integer below 2^24 (reference
    asserts sum |w| |x| + 1000 < 2^24), so any f32 summation is exact and the result has one value.
  float (the norm, RGlu): weights uniform at WEIGHT_SCALE rounded to the stored type, normw at
    NORM_OFFSET +- NORM_SCALE, x rows standard normal times 1, 30, 0.03, 1000 (a row that gets
    another row's scale or data is far off). The reference is float64 over the stored weights'
    exact values: rmsnorm per row, the dot products, act(a) * b for RGlu with the oracle's formulas
    (its f32 constants).
Both: every float of x between n and xstride is NaN; every float of out between d and ostride is
SENTINEL and must come back bit for bit; outputs RStore / RGlu will overwrite start as UNWRITTEN.

model() walks the launch as gemv_rows_kernel does (segments -> chunks -> lanes -> groups, driven
by the plan) with an explicit LDS array, either in float64 (exact family; defects) or as an f32
restatement of the kernel's order (lane chains of fused multiply-adds, the wave_sum butterfly,
stage_x's statement order for the norm). DEFECTS are the index slips test_rows_cpu.py switches
in one at a time. LDS the kernel never wrote reads as 0 here, the value that hides the most."""
import functools
import zlib

import numpy as np

import rows_cases as C

WEIGHT_SCALE = 0.035               # yalm_amd.models WEIGHT_SCALE
NORM_SCALE, NORM_OFFSET = 0.2, 1.0  # yalm_amd.models NORM_SCALE, NORM_OFFSET
EPS = 1e-5
REL_TOL = 2e-5  # tests/test_gpu_kernels.py REL_TOL, here per activation row against float64
# RGlu with GELU: act(a) * b of two f32 dot products, relative to the largest of as few as 5 outputs.
# The f32 restatement of the kernel's order (test_rows_cpu.py) is 5.015e-6 from float64 at its
# worst case (f16-glu-T3-n13360-d5-norm-gelu), above a fifth of REL_TOL = 4e-6, so GELU-GLU's bar
# is 5 x that measured value, 2.51e-5, instead. (SiLU-GLU: 2.87e-6, RStore 8.5e-7, RResidual 6.8e-7:
# these keep REL_TOL.)
GELU_GLU_F32_WORST = 5.02e-6
GELU_GLU_REL_TOL = 5 * GELU_GLU_F32_WORST
SENTINEL = np.float32(-7.25)
UNWRITTEN = np.float32(12345.0)
X_POW2 = (1.0, 2.0, 4.0, 8.0)
X_SCALES = (1.0, 30.0, 0.03, 1000.0)
GELU_C0, GELU_C1 = float(np.float32(0.797885)), float(np.float32(0.044715))

DEFECTS = (
    "segment offset dropped from the weight address",
    "first chunk of the second segment read at the first segment's x",
    "chunk tail skipped",
    "ragged end skipped",
    "ragged end on every lane",
    "normw read without k0",
    "row t's scale taken from row 0",
    "x rows at stride n",
    "out rows at stride d",
    "clamped row stored",
    "last gpw iteration dropped",
)


def encode(v, dtype):
    """float32 -> stored weights (yalm_amd.models.encode_weights: f16 round to nearest even; E5M2
    through f16, round to nearest even on the byte)."""
    v = np.asarray(v, np.float32)
    if dtype == C.F32:
        return v
    h16 = v.astype(np.float16)
    if dtype == C.F16:
        return h16
    hb = h16.view(np.uint16).astype(np.uint32)
    return ((hb + 0x7F + ((hb >> 8) & 1)) >> 8).astype(np.uint8)


def decode(a, dtype):
    """Stored weights -> float32, exactly (E5M2 is the f16 with bits b << 8)."""
    if dtype == C.F8:
        return (a.astype(np.uint16) << 8).view(np.float16).astype(np.float32)
    return a.astype(np.float32)


class Inputs:
    __slots__ = ("x", "w", "w3", "wv", "w3v", "normw", "out0", "eps")


@functools.lru_cache(maxsize=2)
def inputs(name):
    """The case's arrays: x (T, xstride) f32, w / w3 (d, n) stored, wv / w3v their exact f32
    values, normw (n) or None, out0 (T, ostride) f32 as the launch finds it. Read-only."""
    c = C.BY_NAME[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    i = Inputs()
    i.x = np.full((c.T, c.xstride), np.nan, np.float32)
    i.out0 = np.full((c.T, c.ostride), SENTINEL, np.float32)
    i.out0[:, :c.d] = UNWRITTEN
    i.w3 = i.w3v = i.normw = None
    i.eps = EPS if c.norm else 0.0
    if c.exact:
        i.w = encode(rng.integers(-3, 4, (c.d, c.n)), c.dtype)
        i.x[:, :c.n] = rng.integers(-4, 5, (c.T, c.n)) * np.array(X_POW2[:c.T])[:, None]
        if c.epilogue == C.RESIDUAL:
            i.out0[:, :c.d] = rng.integers(-999, 1000, (c.T, c.d))
    else:
        i.w = encode((rng.random((c.d, c.n)) * 2 - 1) * WEIGHT_SCALE, c.dtype)
        if c.epilogue == C.GLU:
            i.w3 = encode((rng.random((c.d, c.n)) * 2 - 1) * WEIGHT_SCALE, c.dtype)
            i.w3v = decode(i.w3, c.dtype)
        if c.norm:
            i.normw = (NORM_OFFSET + (rng.random(c.n) * 2 - 1) * NORM_SCALE).astype(np.float32)
        i.x[:, :c.n] = rng.standard_normal((c.T, c.n)) * np.array(X_SCALES[:c.T])[:, None]
        if c.epilogue == C.RESIDUAL:
            i.out0[:, :c.d] = rng.standard_normal((c.T, c.d))
    i.wv = decode(i.w, c.dtype)
    if c.exact:
        assert np.array_equal(i.wv, np.rint(i.wv)) and np.abs(i.wv).max() <= 3
    for a in (i.x, i.w, i.w3, i.wv, i.w3v, i.normw, i.out0):
        if a is not None:
            a.setflags(write=False)
    return i


def act_ref(a, act):
    """The oracle's activations (infer.cpp:187-197) in the precision of a."""
    if act == C.SILU:
        return a / (1.0 + np.exp(-a))
    return 0.5 * a * (1.0 + np.tanh(a.dtype.type(GELU_C0) * (a + a.dtype.type(GELU_C1) * a * a * a)))


@functools.lru_cache(maxsize=2)
def reference(name):
    """out (T, ostride) float64 after the launch: the plain definition, no kernel structure."""
    c = C.BY_NAME[name]
    i = inputs(name)
    x = i.x[:, :c.n].astype(np.float64)
    if c.norm:
        scale = 1.0 / np.sqrt((x * x).sum(axis=1, keepdims=True) / c.n + float(np.float32(i.eps)))
        x = x * scale * i.normw.astype(np.float64)
    a = x @ i.wv.astype(np.float64).T
    if c.exact:  # every partial sum of every order is an integer below 2^24
        assert (np.abs(x) @ np.abs(i.wv.astype(np.float64)).T).max() + 1000 < 2 ** 24
    out = i.out0.astype(np.float64)
    if c.epilogue == C.STORE:
        out[:, :c.d] = a
    elif c.epilogue == C.RESIDUAL:
        out[:, :c.d] += a
    else:
        out[:, :c.d] = act_ref(a, c.act) * (x @ i.w3v.astype(np.float64).T)
    out.setflags(write=False)
    return out


def rel_tol(c):
    return GELU_GLU_REL_TOL if c.epilogue == C.GLU and c.act == C.GELU else REL_TOL


def bars(c, got, want, tol=None):
    """The worst activation row's max_j |got - want| / (tol max_j |want|) over the d outputs
    (float family), tol = rel_tol(c) unless given; inf for a NaN."""
    g, w = np.asarray(got, np.float64)[:, :c.d], np.asarray(want, np.float64)[:, :c.d]
    b = np.abs(g - w).max(axis=1) / ((tol or rel_tol(c)) * np.abs(w).max(axis=1))
    return float("inf") if np.any(np.isnan(b)) else float(b.max())


def pads_intact(c, got):
    """Every float between d and ostride is SENTINEL, bit for bit."""
    pad = np.ascontiguousarray(np.asarray(got, np.float32)[:, c.d:])
    return bool(np.all(pad.view(np.uint32) == SENTINEL.view(np.uint32)))


# ---------------------------------------------------------------- the traversal model
_L = np.arange(64)
_WAVE_SUM = (_L ^ 1, _L ^ 2, (_L & ~7) | (7 - (_L & 7)), (_L & ~15) | (15 - (_L & 15)), _L ^ 16, _L ^ 32)


def _fma32(a, b, c):
    """f32 fused multiply-add: the product is exact in float64, one rounding to it, one to f32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _wave_sum32(v):
    """device_common.h wave_sum over the last axis (64 lanes) in f32: the DPP row sums (xor 1,
    xor 2, half mirror, mirror), then the lane ^ 16 and lane ^ 32 partners."""
    for p in _WAVE_SUM:
        v = v + v[..., p]
    return v[..., 0]


def _scale32(xrow, n, eps):
    """gemv_rows_kernel's NORM prologue for one row: 512 threads stride float4s, sumsq4 as its
    fma chain, wave_sum per wave, the 8 wave sums added in order."""
    K = -(-n // 2048)
    v = np.zeros(K * 2048, np.float32)
    v[:n] = xrow
    v = v.reshape(K, 512, 4)
    ss = np.zeros(512, np.float32)
    for k in range(K):
        t = v[k, :, 0] * v[k, :, 0]
        for e in (1, 2, 3):
            t = _fma32(v[k, :, e], v[k, :, e], t)
        ss = ss + t
    red = _wave_sum32(ss.reshape(8, 64))
    tot = np.float32(0.0)
    for w in range(8):
        tot = tot + red[w]
    rms = np.sqrt(tot / np.float32(n) + np.float32(eps))
    return np.float32(1.0) / rms


def model(c, p, f32=False, defect=None):
    """out (T, ostride) as the kernel's traversal under plan p computes it: float64, or the f32
    restatement. defect: one of DEFECTS switched in."""
    assert defect is None or defect in DEFECTS
    i = inputs(c.name)
    fl = np.float32 if f32 else np.float64
    ch, epl, T, n, d, G = C.CH[c.dtype], C.EPL[c.dtype], c.T, c.n, c.d, c.n_groups
    kseg, nseg, gpw = p["kseg"], p["nseg"], p["gpw"]
    xflat = i.x.reshape(-1)
    xst = n if defect == "x rows at stride n" else c.xstride
    # the weights as one flat array (zeros behind it: what a read past the last row finds)
    if c.epilogue == C.GLU:
        wflat = np.concatenate([i.wv.reshape(-1), i.w3v.reshape(-1), np.zeros(2 * ch, np.float32)])
        rowoff = np.stack([np.arange(G) * n, (d + np.arange(G)) * n], axis=1)
    else:
        wflat = np.concatenate([i.wv.reshape(-1), np.zeros(2 * ch, np.float32)])
        rowoff = np.minimum(np.arange(G)[:, None] * C.R + np.arange(C.R)[None, :], d - 1) * n
    scale = np.ones(T, fl)
    if c.norm:
        for t in range(T):
            xr = xflat[t * xst:t * xst + n]
            if f32:
                scale[t] = _scale32(xr, n, i.eps)
            else:
                scale[t] = 1.0 / np.sqrt((xr.astype(fl) ** 2).sum() / n + float(np.float32(i.eps)))
        if defect == "row t's scale taken from row 0":
            scale[:] = scale[0]
    xs = np.zeros((T, kseg), fl)  # the LDS
    xs_seg0 = None
    acc = np.zeros((G, C.R, T, 64), fl)

    def step(cidx, lanes, xsrc):
        kk = cidx * ch + lanes[:, None] * epl + np.arange(epl)[None, :]  # [L, epl]
        xv = xsrc[:, kk]                                                # [T, L, epl]
        wv = wflat[rowoff[:, :, None, None] + seg_off + kk[None, None]]  # [G, R, L, epl]
        if f32:
            a = acc[:, :, :, lanes]
            for e in range(epl):
                a = _fma32(wv[:, :, None, :, e], xv[None, None, :, :, e], a)
            acc[:, :, :, lanes] = a
        else:
            acc[:, :, :, lanes] += np.einsum("grle,tle->grtl", wv.astype(fl), xv)

    def steps(chunks, xsrc):
        """Whole chunks, every lane. float64: the order is immaterial, so all of them at once."""
        if f32 or len(chunks) == 0:
            for cidx in chunks:
                step(cidx, _L, xsrc)
            return
        kk = (np.asarray(chunks)[:, None, None] * ch + _L[None, :, None] * epl + np.arange(epl)[None, None, :])
        kk = kk.transpose(1, 0, 2).reshape(64, -1)                       # [64, chunks * epl]
        wv = wflat[rowoff[:, :, None, None] + seg_off + kk[None, None]]  # [G, R, 64, chunks * epl]
        acc[:] += np.einsum("grle,tle->grtl", wv.astype(fl), xsrc[:, kk])

    for s in range(nseg):
        k0 = s * kseg
        kl = min(kseg, n - k0)
        for t in range(T):
            v = xflat[t * xst + k0:t * xst + k0 + kl].astype(fl)
            if c.norm:
                nk = 0 if defect == "normw read without k0" else k0
                v = v * scale[t] * i.normw[nk:nk + kl].astype(fl)
            xs[t, :kl] = v
        if s == 0:
            xs_seg0 = xs.copy()
        nfull, rem = kl // ch, kl % ch
        seg_off = 0 if defect == "segment offset dropped from the weight address" else k0
        chunks = list(range(nfull // C.ROWS_U * C.ROWS_U if defect == "chunk tail skipped" else nfull))
        if defect == "first chunk of the second segment read at the first segment's x" and s == 1 and chunks:
            step(chunks.pop(0), _L, xs_seg0)
        steps(chunks, xs)
        if rem > 0 and defect != "ragged end skipped":
            step(nfull, _L if defect == "ragged end on every lane" else _L[_L * epl < rem], xs)

    tot = _wave_sum32(acc) if f32 else acc.sum(axis=-1)  # [G, R, T]
    ost = d if defect == "out rows at stride d" else c.ostride
    out = i.out0.astype(fl).reshape(-1).copy()
    g = np.arange(G)
    live = (g % gpw != gpw - 1) if defect == "last gpw iteration dropped" else np.ones(G, bool)
    for t in range(T):
        if c.epilogue == C.GLU:
            out[t * ost + g[live]] = (act_ref(tot[:, 0, t], c.act) * tot[:, 1, t])[live]
            continue
        for r in range(C.R):
            j = g * C.R + r
            ok = live & ((j <= d) if defect == "clamped row stored" else (j < d))
            if c.epilogue == C.STORE:
                out[t * ost + j[ok]] = tot[ok, r, t]
            else:
                out[t * ost + j[ok]] += tot[ok, r, t]
    return out.reshape(T, c.ostride)
