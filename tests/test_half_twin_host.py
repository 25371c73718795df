"""half_twin.half_rtz / half_dt on the CPU: the twin that test_gpu_bounds_fp16 holds the half-precision bound path to is itself held to the
definition of round-toward-zero, exhaustively over the half patterns: every non-negative finite half is a fixed point, the float32 just
above it comes back to it, the float32 just below it goes to the half below; overflow ends at 65504; what lies under the smallest
subnormal ends at 0."""
import numpy as np

from half_twin import HALF_MAX_BITS, half_dt, half_rtz

FINITE = np.arange(0, HALF_MAX_BITS + 1, dtype=np.uint16)          # every non-negative finite half, +0 to 65504
F32_INF = np.float32(np.inf)


def _bits(h):
    assert h.dtype == np.float16
    return h.view(np.uint16)


def test_every_half_is_a_fixed_point():
    x = FINITE.view(np.float16).astype(np.float32)                  # exact
    assert np.array_equal(_bits(half_rtz(x)), FINITE)


def test_next_float_above_comes_back_down():
    x = FINITE.view(np.float16).astype(np.float32)
    above = np.nextafter(x, F32_INF)
    assert np.all(above > x)
    assert np.array_equal(_bits(half_rtz(above)), FINITE)           # 65504's successor included: still 0x7bff


def test_next_float_below_goes_to_the_half_below():
    x = FINITE[1:].view(np.float16).astype(np.float32)
    below = np.nextafter(x, np.float32(0))
    assert np.all(below < x) and np.all(below >= 0)
    assert np.array_equal(_bits(half_rtz(below)), FINITE[1:] - np.uint16(1))


def test_overflow_ends_at_the_largest_finite_half():
    x = np.array([65504.0, 65519.99, 65520.0, 1e6, np.finfo(np.float32).max], np.float32)
    assert x[1] < 65520 and x[1] > 65504
    assert np.array_equal(_bits(half_rtz(x)), np.full(5, HALF_MAX_BITS, np.uint16))
    assert np.array_equal(_bits(half_rtz(np.array([np.inf], np.float32))), [HALF_MAX_BITS])


def test_below_the_smallest_subnormal_is_zero():
    tiny = np.float32(2.0 ** -24)
    n = int(tiny.view(np.uint32))                                   # the float32 patterns 0 .. n - 1 are exactly the values in [0, 2^-24)
    # 864 M patterns: every 4 099th, and both ends in full.  The rest follows from test_never_above_the_input_...: a non-negative half that does
    # not exceed an input below the smallest positive half is 0
    pats = np.unique(np.concatenate([np.arange(0, n, 4099, dtype=np.uint32), np.arange(0, 4096, dtype=np.uint32),
                                     np.arange(n - 4096, n, dtype=np.uint32)]))
    x = pats.view(np.float32)
    assert np.all(x < tiny)
    assert not _bits(half_rtz(x)).any()
    # and every power of two below 2^-24 with all-ones mantissa, subnormal floats included: the largest value of each binade
    edge = (np.arange(1, (n >> 23) + 1, dtype=np.uint32) << np.uint32(23)) - np.uint32(1)
    assert np.all(edge.view(np.float32) < tiny) and not _bits(half_rtz(edge.view(np.float32))).any()
    assert _bits(half_rtz(np.array([tiny], np.float32)))[0] == 1    # 2^-24 itself is the smallest subnormal


def test_never_above_the_input_and_within_one_step():
    rng = np.random.default_rng(20261019)
    pats = rng.integers(0, int(np.float32(np.inf).view(np.uint32)), 2_000_000, dtype=np.uint32)       # every binade of float32, subnormals included
    x = np.concatenate([pats.view(np.float32), rng.uniform(0, 70000, 200_000).astype(np.float32), rng.uniform(0, 2.0 ** -13, 200_000).astype(np.float32)])
    h = half_rtz(x)
    assert np.isfinite(h).all()
    back = h.astype(np.float32)
    assert np.all(back <= x)
    up = np.minimum(_bits(h).astype(np.uint32) + 1, HALF_MAX_BITS + 1).astype(np.uint16).view(np.float16).astype(np.float32)   # 0x7c00 = inf above 65504
    assert np.all(up > x)                                           # the largest half not above the input: the next one is above it
    assert half_rtz(x.reshape(4, -1)).shape == (4, len(x) // 4)


class _Grid:
    """what half_dt reads of a registration: geometry and the fp32 grid"""

    def __init__(self, V, scale, origin, grid):
        self.V, self.scale, self.origin, self.grid = V, scale, origin, grid

    def dt_info(self):
        return self.V, self.scale, self.origin

    def dt_download(self):
        return self.grid


def test_half_dt_returns_the_wrapped_values_at_the_voxel_centres(oracle_mod):
    V, scale, origin = 7, 3.5, (-1.0, 0.25, 2.0)
    rng = np.random.default_rng(3)
    grid = rng.uniform(0, 2, (V, V, V)).astype(np.float32)
    grid[0, 0, 0], grid[1, 2, 3], grid[6, 6, 6], grid[2, 0, 5] = 0.0, 1e-6, 1e5, 70000.0          # zero, a half subnormal, two values above 65504
    dt = half_dt(_Grid(V, scale, origin, grid), oracle_mod)
    assert dt.V == V and dt.scale == scale and tuple(dt.origin) == origin
    z, y, x = np.meshgrid(np.arange(V), np.arange(V), np.arange(V), indexing="ij")
    q = np.stack([origin[0] + x / scale, origin[1] + y / scale, origin[2] + z / scale], -1).reshape(-1, 3)
    want = half_rtz(grid).astype(np.float32)
    got = dt.distance(q).reshape(V, V, V)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got[6, 6, 6] == 65504 and got[2, 0, 5] == 65504 and got[0, 0, 0] == 0 and 0 < got[1, 2, 3] < 1e-6
    assert np.mean(got != grid) > 0.9 and np.all(got <= grid)       # the conversion really changed the grid, downwards only
    assert np.array_equal(dt.grid(), want)
