"""CPU: every input of the mixture-of-experts prefill tests (tests/moe_prefill_inputs.py) keeps
its routing margin on the reference, so that "experts identical" on the GPU never hangs on
rounding: PREFILL_MARGIN (1e-2) at every (position, layer) of the token sequences, whose router
reads a prefilled state, and moe_ref.MARGIN (1e-3) on the FFN-row inputs, where both sides route
the same x."""
import numpy as np
import pytest

import moe_prefill_inputs as I
import moe_ref as R
import oracle_py as O
from yalm_amd import models as M


@pytest.mark.parametrize("name", list(I.CONFIGS))
def test_sequences_clear_prefill_margin(name):
    cfg, n = I.CONFIGS[name]
    tokens, tries, worst = I.sequence(name)
    print(f"{name}: {n} positions, {tries} tries, min margin {worst:.3e}")
    assert len(tokens) == n and worst >= I.PREFILL_MARGIN
    # an independent pass over the finished sequence (fresh state, no rejected tries in between)
    assert I.margins(cfg, I.tensors(name), tokens) >= I.PREFILL_MARGIN


def test_spike_model_exceeds_f16_range():
    """The range-guard model's GLU product passes 65504 in its spike layer at every position."""
    cfg, _ = I.CONFIGS["spike"]
    t = I.tensors("spike")
    tokens, _, _ = I.sequence("spike")
    ref = R.MoeRef(cfg, t)
    n = M.layer_names(I.SPIKE_LAYER)
    for pos in (0, 1, len(tokens) - 1):
        ref.x[:] = ref.embed(int(tokens[pos]))
        # (position 0's attention sees itself only; enough to reach the spike layer's input)
        for l in range(I.SPIKE_LAYER):
            ref.block(l, 0, 0, 0, 1)
        ref.om.block(I.SPIKE_LAYER, 0, 0, 0, 1)
        xb = R.rmsnorm(ref.x, t[n["rms_ffn"]], cfg.norm_eps)
        r = I.SPIKE_ROWS[0]
        a = float(t[n["w1"]][0, r].astype(np.float32) @ xb)
        b = float(t[n["w3"]][0, r].astype(np.float32) @ xb)
        assert a > 100 and abs(a * b) > 65504 * 2, (pos, a, b)


@pytest.mark.parametrize("case", I.FFN_ROW_CASES, ids=[c[0] for c in I.FFN_ROW_CASES])
def test_ffn_rows_clear_margin(case):
    _, T, _, _, _, K, dtype, _, _ = case
    x, gate = I.ffn_rows_router_inputs(case)
    assert np.array_equal(x, x.astype(np.float16).astype(np.float32))  # f16-exact rows
    worst = min(R.routing_margin(O.matmul(x[t], gate, dtype), K) for t in range(T))
    assert worst >= R.MARGIN, worst


def test_tie_rows_input():
    """The exact-tie input of the GPU test: two identical gate rows, the third pick no near-tie."""
    x, gate = I.tie_inputs()
    lg = O.matmul(x[0], gate, M.F16)
    assert lg[1] == lg[4] and R.moe_gate(lg, 3)[0].tolist()[:2] == [1, 4]
    assert R.routing_margin(np.delete(lg, [1, 4]), 1) >= R.MARGIN


def test_host_model_margins(tmp_path):
    """The CLI test's model (HOST_SEED): the perplexity text clears MARGIN, the hydrated prompt and
    the completion's decode steps clear PREFILL_MARGIN, no greedy step is a near-tie."""
    m_text, m_prompt, gap = I.host_margins(I.host_yalm(tmp_path))
    print(f"text margin {m_text:.3e}, prompt margin {m_prompt:.3e}, min greedy top-2 gap {gap:.3e}")
    assert m_text >= R.MARGIN and m_prompt >= I.PREFILL_MARGIN and gap >= 2 * 5e-3
