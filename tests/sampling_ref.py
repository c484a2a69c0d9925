"""The device sampling rule (include/yalm_hip.h, yalm_generate_sampled) in numpy integers.

The rule takes the fixed-point weights q as input, so a test feeds it the very q the kernel
used (yalm_sample's weights_out) and everything after the weights is exact: the kept set and
the token of every uniform. weights_f32 restates the weights in numpy f32 for the CPU tests
(numpy's expf may differ from the device's by an ulp, which is why the GPU tests do not use it
for exact checks).
"""
import math

import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)


def keys(logits) -> np.ndarray:
    """Order-preserving uint32 keys: larger logit, larger key; -0 as +0; NaN below everything."""
    l = np.asarray(logits, np.float32)
    with np.errstate(invalid="ignore"):
        u = (l + np.float32(0)).view(np.uint32)
    k = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    k[np.isnan(l)] = 0
    return k


def first_max(logits):
    """(m, index) of the strict '>' scan from -FLT_MAX (sampler.cpp:27-38): the first maximum,
    (-FLT_MAX, 0) when nothing exceeds -FLT_MAX."""
    l = np.asarray(logits, np.float32)
    with np.errstate(invalid="ignore"):
        ok = l > -FLT_MAX
    if not ok.any():
        return np.float32(-FLT_MAX), 0
    m = l[ok].max()
    return np.float32(m), int(np.flatnonzero(ok & (l == m))[0])


def weights_f32(logits, temperature) -> np.ndarray:
    """q_i = (uint64) ldexpf(expf((l_i - m) / T), 40) with every step in f32; 0 where the
    weight is not a finite positive number."""
    l = np.asarray(logits, np.float32)
    m, _ = first_max(l)
    with np.errstate(all="ignore"):
        w = np.exp(((l - m) / np.float32(temperature)).astype(np.float32)).astype(np.float32)
        good = (w > 0) & (w <= FLT_MAX)
        q = np.where(good, np.ldexp(np.where(good, w, 0).astype(np.float64), 40), 0.0)
    return np.floor(q).astype(np.uint64)


def frac_target(frac, S: int) -> int:
    """min(S, max(1, ceil((double)frac * (double)S))), frac an f32."""
    c = math.ceil(float(np.float32(frac)) * float(S))
    return min(S, max(1, c))


class Rule:
    """The kept set of (logits, q, top_k, top_p) and the draw for any uniform."""

    def __init__(self, logits, q, top_k: int = 0, top_p: float = 1.0):
        l = np.asarray(logits, np.float32)
        q = np.asarray(q, np.uint64)
        n = l.size
        self.n = n
        self.amax = first_max(l)[1]
        k = keys(l)
        # logit descending, index ascending among equal logits
        order = np.lexsort((np.arange(n), np.uint32(0xFFFFFFFF) - k))
        cand = order[: min(top_k, n)] if top_k > 0 else order
        if np.float32(top_p) < np.float32(1.0):
            cum = np.cumsum(q[cand], dtype=np.uint64)
            S_k = int(cum[-1])
            need = frac_target(top_p, S_k) if S_k > 0 else 0
            cnt = int(np.searchsorted(cum, np.uint64(need), side="left")) + 1 if need > 0 else 0
            cand = cand[:cnt]
        self.mask = np.zeros(n, bool)
        self.mask[cand] = True
        self.kept = int(cand.size)
        self.cum = np.cumsum(np.where(self.mask, q, np.uint64(0)), dtype=np.uint64)
        self.S = int(self.cum[-1])

    def draw(self, u) -> int:
        if self.S == 0:
            return self.amax
        t = frac_target(u, self.S)
        return int(np.searchsorted(self.cum, np.uint64(t), side="left"))

    def draws(self, uniforms) -> np.ndarray:
        return np.array([self.draw(u) for u in np.asarray(uniforms, np.float32).reshape(-1)], np.int32)

    def boundary_uniforms(self, idxs) -> np.ndarray:
        """float32(C_i / S) for the kept indices idxs with its f32 neighbour on each side, clipped
        to [0, 1]: the uniforms at which the draw changes token."""
        out = []
        for i in idxs:
            b = np.float32(int(self.cum[i]) / self.S)
            out += [np.nextafter(b, np.float32(-1)), b, np.nextafter(b, np.float32(2))]
        return np.clip(np.array(out, np.float32), 0, 1)


def inverse_cdf_f64(logits, temperature, uniforms, margin=1e-5):
    """The reference's sampler in f64 (sampler.cpp:43-59): softmax(l / T), first index whose
    cumulative probability reaches u. Returns (tokens, far): far[j] is False where u_j lies
    within margin of a boundary of the cumulative distribution."""
    l = np.asarray(logits, np.float64) / float(temperature)
    p = np.exp(l - l.max())
    cdf = np.cumsum(p / p.sum())
    u = np.asarray(uniforms, np.float64)
    tok = np.minimum(np.searchsorted(cdf, u, side="left"), l.size - 1)
    lo = np.abs(cdf[tok] - u)
    hi = np.abs(np.where(tok > 0, cdf[np.maximum(tok - 1, 0)], -1.0) - u)
    return tok.astype(np.int32), np.minimum(lo, hi) > margin
