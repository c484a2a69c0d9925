"""The q8 kv format's numpy statement (models.kv_q8_quantize / kv_q8_dequantize) on the CPU."""
import numpy as np
import pytest

from yalm_amd import models as M


@pytest.mark.parametrize("D", [64, 128])
def test_format(D):
    rng = np.random.default_rng(D)
    x = (rng.standard_normal((9, 3, D)) * rng.uniform(1e-3, 100, (9, 3, 1))).astype(np.float16)
    x[0, 0] = 0
    x[1, 1, 3] = 65504
    x[2, 2] = np.arange(D) % 11 - 5 + 0.5   # a = 127, inv = 1: every x * inv ends in .5
    x[2, 2, 0] = -127
    c, s = M.kv_q8_quantize(x)
    assert c.dtype == np.uint8 and s.dtype == np.float32 and c.shape == x.shape and s.shape == x.shape[:2]
    assert s[0, 0] == 0 and (c[0, 0] == 128).all()
    assert c.min() >= 1                      # |c| <= 127: the byte 0 never appears
    a = np.abs(x.astype(np.float32)).max(axis=-1)
    np.testing.assert_array_equal(s, a / np.float32(127))
    assert (np.abs(c.astype(int) - 128).max(axis=-1)[a > 0] == 127).all()   # the row's maximum has the largest code
    np.testing.assert_array_equal(c[2, 2, 1:12].astype(int) - 128, [-4, -2, -2, 0, 0, 2, 2, 4, 4, 6, -4])  # -3.5 .. 5.5, -4.5: half to even
    v = M.kv_q8_dequantize(c, s)
    assert np.abs(v - x.astype(np.float32)).max() <= (s.max(axis=None) / 2) * (1 + 1e-6)
    assert (np.abs(v - x.astype(np.float32)) <= s[..., None] * 0.5 * (1 + 1e-6)).all()   # half a step per element
