"""CPU: the margins that make tests/test_gpu_gqa.py meaningful -- on the float64 reference of
every case of gqa_cases.py the greedy path has no near-tie, and the model without the case's bias
or q / k norm is at least 10 bars from the model with it at every compared position of the walk,
so a decoder that dropped the form at these groups or in key mode cannot pass."""
import numpy as np
import pytest

import attn_ref
import gqa_cases as C
from yalm_amd import models as M

LOGITS_BAR = C.LOGITS_BAR


def test_shapes_are_the_ones_meant():
    """G = 7, 5 and 8 (head_dim 64, 128, 256) over two kv heads; the window is five chunks, so the
    walk passes head mode, the switch to key mode at kv_len 257, the wrap and the sinks, and the
    multi-row steps at 254 and 255 straddle the switch."""
    want = {"g7": (7, 64), "g5": (5, 128), "g8": (8, 256)}
    for name, (cfg, _) in C.CASES.items():
        assert (cfg.n_heads // cfg.n_kv_heads, cfg.head_dim) == want[name[:2]] and cfg.n_kv_heads == 2
        assert (cfg.n_layers, cfg.vocab_size, cfg.max_seq_len) == (2, 1024, 320)
    assert C.G7.qkv_bias and C.G7.tied and C.G5.qk_norm and C.G5.q_dim != C.G5.dim
    assert {C.CASES[n][0].weight_dtype for n in C.CASES if n.startswith("g7")} == {M.F16, M.F8E5M2, M.Q4}
    assert {C.CASES[n][0].weight_dtype for n in C.CASES if n.startswith("g5")} == {M.F16, M.F8E5M2}
    assert attn_ref.mode_of(256, C.MSL) == "head" and attn_ref.mode_of(257, C.MSL) == "key"
    assert C.N_POS == C.MSL + 10 and C.GREEDY_POS < 256 < C.GREEDY_POS + C.GREEDY_N
    for p in C.ROWS_POS:
        assert p + C.SPEC_ROWS <= C.MSL
    assert [[attn_ref.mode_of(p + r + 1, C.MSL) for r in range(4)] for p in C.ROWS_POS] == [
        ["head", "head", "key", "key"], ["head", "key", "key", "key"], ["key"] * 4]
    assert C.GREEDY_POS + C.SPEC_GEN + C.SPEC_ROWS <= C.MSL  # the speculative run stays in the window


@pytest.mark.parametrize("name", list(C.CASES))
def test_greedy_paths_have_no_near_tie(name):
    """The seeds: the reference's greedy path from position 240 keeps a top-2 gap of 10 bars of
    max|logit| over the 24 tokens the device greedy loop is compared on, and of 2 bars over the
    rest of the 70-token speculative path."""
    toks, gaps = C.greedy_run(name)
    assert len(toks) == C.SPEC_GEN
    print(f"{name}: smallest gap {gaps[:C.GREEDY_N].min():.4f} (first {C.GREEDY_N}), {gaps.min():.4f} (all)")
    assert gaps[:C.GREEDY_N].min() > C.GAP, gaps[:C.GREEDY_N].min()
    assert gaps.min() > C.SPEC_GAP, gaps.min()


@pytest.mark.parametrize("name", C.FORM_CASES)
def test_the_form_matters_at_every_compared_position(name):
    """Positions FIRST .. 329 of the walk: the reference without the bias / the norm is at least
    10 x LOGITS_BAR from the reference with it (as test_arch_cpu.py / test_qknorm_cpu.py)."""
    full, plain = C.logits_run(name), C.logits_run(name, "plain")
    d = np.array([C.relerr(plain[pos], full[pos]) for pos in range(C.FIRST[name], C.N_POS)])
    print(f"{name}: the form dropped moves the logits by {d.min():.3f} .. {d.max():.3f}")
    assert d.min() >= 10 * LOGITS_BAR, (int(np.argmin(d)) + C.FIRST[name], d.min())
