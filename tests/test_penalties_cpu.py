"""CPU: the numpy statement of the penalties and min-p (tests/penalties_ref.py) on the inputs the
GPU tests use: neutral values are the plain rule, and every penalty kind changes a token."""
import numpy as np
import pytest

import penalties_ref as P
import sampling_ref as R

NS = [5, 4096, 4097, 33000]
WINDOWS = [8, 1024]
U = np.array([0.0, 0.5, 1.0], np.float32)
KINDS = {"repetition": dict(repetition=1.25), "frequency": dict(frequency=0.25), "presence": dict(presence=0.25),
         "min_p": dict(min_p=0.25), "all": dict(repetition=1.25, frequency=0.25, presence=0.25, min_p=0.25)}
TRUNC = [(0, 1.0), (3, 0.9)]


def hist_lens(window):
    return [0, 1, window - 1, window, window + 3]


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("n", NS)
def test_neutral_is_the_plain_rule(n, window):
    for hl in hist_lens(window):
        l, h = P.make_case(n, hl, window)
        for k, p in TRUNC:
            plain = R.Rule(l, R.weights_f32(l, 0.8), k, p).draws(U)
            assert np.array_equal(P.draws(l, h, window, P.NEUTRAL, 0.8, k, p, U), plain)
            assert np.array_equal(P.draws(l, h, 0, dict(KINDS["all"], min_p=0.0), 0.8, k, p, U), plain)


@pytest.mark.parametrize("kind", list(KINDS))
def test_every_kind_moves_a_token(kind):
    moved = 0
    for n in NS:
        for window in WINDOWS:
            for hl in hist_lens(window):
                l, h = P.make_case(n, hl, window)
                plain = R.Rule(l, R.weights_f32(l, 0.8)).draws(U)
                moved += not np.array_equal(P.draws(l, h, window, KINDS[kind], 0.8, 0, 1.0, U), plain)
    assert moved > 0
