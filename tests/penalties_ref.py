"""The penalties and min-p of yalm_generate_sampled_ex (include/yalm_hip.h) in numpy on top of
sampling_ref; like its Rule it takes the weights q as input, so a GPU test feeds it the device's own."""
import math
from collections import Counter

import numpy as np

import sampling_ref as R

NEUTRAL = dict(repetition=1.0, frequency=0.0, presence=0.0, min_p=0.0)


def penalise(logits, history, window, repetition=1.0, frequency=0.0, presence=0.0, **_) -> np.ndarray:
    """l' for every token of the last min(window, len) of history, each operation rounded once to f32."""
    l = np.array(logits, np.float32)
    h = [int(t) for t in history]
    rep, fr, pr = np.float32(repetition), np.float32(frequency), np.float32(presence)
    with np.errstate(all="ignore"):
        for i, c in Counter(h[len(h) - min(window, len(h)):]).items():
            a = l[i] / rep if l[i] > 0 else l[i] * rep
            l[i] = a - (fr * np.float32(c) + pr)
    return l


class Rule(R.Rule):
    """sampling_ref.Rule with the kept set cut to q_i >= qmin = ceil((double)min_p * 2^40)."""

    def __init__(self, logits, q, top_k=0, top_p=1.0, min_p=0.0):
        super().__init__(logits, q, top_k, top_p)
        self.mask &= np.asarray(q, np.uint64) >= np.uint64(math.ceil(float(np.float32(min_p)) * 2.0 ** 40))
        self.cum = np.cumsum(np.where(self.mask, q, np.uint64(0)), dtype=np.uint64)
        self.S = int(self.cum[-1])


def draws(logits, history, window, pen, T, top_k, top_p, uniforms, weights=R.weights_f32) -> np.ndarray:
    """The tokens of yalm_sample_ex; weights(l', T) gives q (the device's own on the GPU)."""
    lp = penalise(logits, history, window, **pen)
    return Rule(lp, weights(lp, T), top_k, top_p, pen.get("min_p", 0.0)).draws(uniforms)


def make_case(n, hist_len, window, seed=0):
    """Logits of both signs and a history: the maximum (n - 1) and token 0 in the window; a token three
    times, whose 2.5 lands on another's 1.0 under 1.25 / 0.25 / 0.25 (a new plateau); past the window
    only a token with a high logit found nowhere else, which must not count."""
    rng = np.random.default_rng(seed + 31 * n + hist_len)
    l = (rng.standard_normal(n) * 2).astype(np.float32)
    old, rep, same = 1, n // 2, n - 2
    l[[n - 1, old, rep, same]] = 9.0, 8.5, 2.5, 1.0
    recent = [n - 1, rep, 0, rep, rep] + [int(t) for t in rng.integers(0, n, max(hist_len, 5))]
    h = [t if t != old else 0 for t in recent[:min(hist_len, window)][::-1]]
    return l, np.array([old] * max(hist_len - window, 0) + h, np.int32)
