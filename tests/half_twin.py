"""Host twin of the half-precision distance-transform copy that Params::bounds_fp16 makes (layout 2, dt_to_half_kernel): IEEE binary16,
rounded toward zero -- half subnormals kept, everything above the largest finite half ends AT it (65504, bits 0x7bff), never at infinity.
No device, no engine arithmetic: numpy's round-to-nearest conversion, then one step down the bit pattern wherever that rounded up."""
import numpy as np

HALF_MAX_BITS = 0x7bff          # 65504


def half_rtz(x):
    """float32 array of non-negative values -> float16 array of the same shape, rounded toward zero.  Non-negative halves are ordered as
    their bit patterns, so "the next half below" is the pattern minus one; the nearest half exceeds the input exactly where nearest
    rounded up, and is infinite exactly where the input lies at or above 65520 (infinity itself included)."""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):
        h = x.astype(np.float16)
    bits = h.view(np.uint16).copy()
    up = np.isinf(h) | (h.astype(np.float32) > x)
    bits[up] -= np.uint16(1)
    return bits.view(np.float16)


def half_dt(reg, oracle):
    """the oracle's distance transform over what the half grid of `reg` must hold: reg's fp32 grid through half_rtz, widened back to float32
    (exact), under reg's own geometry.  `reg` needs dt_info() and dt_download() only."""
    V, scale, origin = reg.dt_info()
    grid = half_rtz(reg.dt_download()).astype(np.float32)
    return oracle.DistanceTransform.wrap(V, scale, origin[0], origin[1], origin[2], grid)
