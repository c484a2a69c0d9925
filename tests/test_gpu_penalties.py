"""GPU: penalties and min-p in the device sampler (sample_pen_kernel, yalm_generate_sampled_ex).
All exact: tokens against tests/penalties_ref.py fed the device's own fixed-point weights of the
penalised logits (yalm_sample's weights_out), logits bit for bit as uint32."""
import numpy as np
import pytest

import penalties_ref as P
from test_penalties_cpu import KINDS, NS, TRUNC, U, WINDOWS, hist_lens
from yalm_amd import models as M

pytestmark = pytest.mark.gpu

MIN_PS = [0.0, 2.0 ** -20, 0.25, 1.0]
LOOP_PEN = dict(repetition=1.3, frequency=0.2, presence=0.1, min_p=0.05, window=8)
CTX = [3, 1, 4, 1, 5]
OK = dict(P.NEUTRAL, window=8)
BAD = [("repetition", 0.0), ("repetition", -1.0), ("repetition", float("inf")), ("repetition", float("nan")),
       ("frequency", float("inf")), ("frequency", float("nan")), ("presence", float("-inf")),
       ("presence", float("nan")), ("min_p", -0.1), ("min_p", 1.5), ("min_p", float("nan")), ("window", -1),
       ("window", 1025)]


@pytest.fixture
def tiny(request):
    from yalm_amd import runtime

    dm = runtime.DeviceModel.synthetic(M.TINY.with_(weight_dtype=getattr(request, "param", M.F16)), seed=3)
    dec = runtime.Decoder(dm)
    yield runtime, dec
    dec.close()
    dm.close()


def device_rule(runtime, l, h, window, pen, T, k, p):
    lp = P.penalise(l, h, window, **pen)
    return P.Rule(lp, runtime.sample(lp, T, k, p, [0.5])[2], k, p, pen.get("min_p", 0.0))


@pytest.mark.parametrize("trunc", TRUNC, ids=["plain", "k3p0.9"])
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("n", NS)
def test_hook_matches_rule_and_restores_logits(n, window, trunc):
    from yalm_amd import runtime

    (k, p), moved = trunc, 0
    for hl in hist_lens(window):
        l, h = P.make_case(n, hl, window)
        l[0] = np.array([0x7FC12345], np.uint32).view(np.float32)[0]  # a NaN payload, in the window when hl >= 3
        plain = runtime.sample(l, 0.8, k, p, U)[0]
        for kind, base in KINDS.items():
            for min_p in MIN_PS:
                pen = dict(base, min_p=min_p)
                tok, after = runtime.sample_ex(l, 0.8, k, p, dict(pen, window=window), h, U)
                want = device_rule(runtime, l, h, window, pen, 0.8, k, p).draws(U)
                assert np.array_equal(tok, want), (hl, kind, min_p, tok, want)
                assert np.array_equal(after.view(np.uint32), l.view(np.uint32)), (hl, kind, min_p)
                moved += not np.array_equal(tok, plain)
    assert moved > 0


def test_neutral_penalties_are_the_plain_loop(tiny):
    _, dec = tiny
    u = np.random.default_rng(11).random(24, dtype=np.float32)
    plain = dec.generate_sampled(1, 0, 24, 0.8, 40, 0.9, uniforms=u)
    dec.enqueue_greedy(3)
    cont = dec.device_tokens()
    assert cont[:24] == plain and len(cont) == 27
    for pen in (OK, dict(KINDS["all"], min_p=0.0, window=0)):
        assert dec.generate_sampled(1, 0, 24, 0.8, 40, 0.9, uniforms=u, penalties=pen, context=CTX) == plain
        dec.enqueue_greedy(3)
        assert dec.device_step()[1] == 27 and dec.device_tokens() == cont
    assert dec.graph_kernels(4) == dec.graph_kernels(3) == dec.graph_kernels(2)
    assert dec.time_kernel(15, 3) > 0 and dec.kernel_name(15) == "sample_pen_kernel"


@pytest.mark.parametrize("tiny", [M.F16, M.F8E5M2], ids=["fp16", "fp8"], indirect=True)
def test_penalised_loop_matches_host_loop(tiny):
    """24 steps over 5 context tokens with window 8: tokens leave the window. Step by step the
    device's logits, then the numpy rule over the history grown on the host."""
    runtime, dec = tiny
    n, T, k, p = 24, 0.8, 40, 0.9
    u = np.random.default_rng(11).random(n, dtype=np.float32)
    pen = {f: v for f, v in LOOP_PEN.items() if f != "window"}
    seq, hist = [], CTX + [1]
    for i in range(n):
        t = dec.generate_sampled(hist[-1], i, 1, T, k, p, uniforms=u[i:i + 1], penalties=LOOP_PEN, context=hist[:-1])[0]
        want = device_rule(runtime, dec.get_logits(), hist, 8, pen, T, k, p).draw(u[i])
        assert t == want, (i, t, want)
        seq.append(t)
        hist.append(t)
    assert seq != dec.generate_sampled(1, 0, n, T, k, p, uniforms=u)  # the penalties matter here
    assert dec.generate_sampled(1, 0, n, T, k, p, uniforms=u, penalties=LOOP_PEN, context=CTX) == seq
    assert dec.device_step() == (seq[-1], n) and dec.device_tokens() == seq
    after = dec.get_logits().copy()  # of the last fed token, seq[-2] at n - 1: the forward's, not the patched ones
    assert np.array_equal(after.view(np.uint32), dec.forward(seq[-2], n - 1).view(np.uint32))


def test_argument_errors(tiny):
    runtime, dec = tiny
    one = dict(uniforms=[0.5])
    for field, v in BAD:
        pen = dict(OK, **{field: v})
        with pytest.raises(runtime.YalmError, match=f"yalm error 2.*{field}"):
            runtime.sample_ex(np.zeros(16, np.float32), 1.0, penalties=pen, history=[1])
        with pytest.raises(runtime.YalmError, match=f"yalm error 2.*{field}"):
            dec.generate_sampled(1, 0, 1, 1.0, penalties=pen, context=[1], **one)
    for ctx in ([-1], [M.TINY.vocab_size]):
        with pytest.raises(runtime.YalmError, match="yalm error 2.*context token"):
            dec.generate_sampled(1, 0, 1, 1.0, penalties=OK, context=ctx, **one)
    s, pn, u, out = runtime.Sampling(1.0, 0, 1.0), runtime.Penalties(1, 0, 0, 0, 8), np.array([0.5], np.float32), np.zeros(1, np.int32)
    rc = runtime.lib.yalm_generate_sampled_ex(dec.h, 1, 0, 1, s, pn, None, -1, u.ctypes.data, out.ctypes.data)
    assert rc == 2 and b"n_context" in runtime.lib.yalm_last_error()
    with pytest.raises(runtime.YalmError, match="yalm error 2.*top_p"):  # what yalm_generate_sampled rejects
        dec.generate_sampled(1, 0, 1, 1.0, top_p=0.0, penalties=OK, **one)
    assert len(dec.generate_sampled(1, 0, 4, 1.0, seed=1, penalties=OK, context=[1, 2])) == 4
