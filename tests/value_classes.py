"""Value classes for the parity tests: grids of signed, zero, subnormal, huge and non-finite
doubles, each with the diffusion rate it is run at, and the comparisons that go with them.

The oracle's contract (oracle/mm_oracle.h) is bit for bit, so the cells are compared as bits
(assert_same_bits: the sign of a zero and of an infinity count, a NaN's payload does not);
only the step sums, whose summation order differs by design, get the project's 1e-12 bound,
taken relative to the sum of the magnitudes (assert_sum_close).

A plain module, not a conftest: tests/test_oracle.py checks on the CPU that every class keeps
its character under the oracle, tests/test_gpu_values.py runs the kernels on them.
"""
import math

import numpy as np

# class -> the rate it runs with. A positive rate turns every zero into +0 after one step;
# only a negative one keeps both signs of zero alive (about half of each), hence `zeros`.
RATES = {"signed": 0.3, "wide": 1.0, "zeros": -0.25, "subnormal": 0.3, "huge": 1.75,
         "nonfinite": 0.3}
CLASSES = tuple(RATES)
FINITE = tuple(c for c in CLASSES if c != "nonfinite")
NONFINITE_SEEDS = (float("nan"), float("inf"), float("-inf"))


def _rng(H, W, seed):
    return np.random.default_rng(seed + 1000003 * H + W)


def _scaled(rng, H, W, elo, ehi):
    """+-(1 + u) * 2^e, e a uniform integer in [elo, ehi] (one rounding, in ldexp)."""
    m = 1.0 + rng.random((H, W))
    e = rng.integers(elo, ehi + 1, (H, W))
    sign = np.where(rng.random((H, W)) < 0.5, -1.0, 1.0)
    return sign * np.ldexp(m, e)


def signed(H, W, seed=0):
    """Uniform in (-1, 1)."""
    return _rng(H, W, seed).uniform(-1.0, 1.0, (H, W))


def wide(H, W, seed=0):
    """81 binades, both signs."""
    return _scaled(_rng(H, W, seed), H, W, -40, 40)


def zeros(H, W, seed=0):
    """Every cell +0.0 or -0.0, but five cells uniform in (-1, 1): two opposite corners, the
    middle of the first row and of the first column, one interior cell (they coincide on
    degenerate grids)."""
    rng = _rng(H, W, seed)
    v = np.where(rng.random((H, W)) < 0.5, -0.0, 0.0)
    for x, y in ((0, 0), (H - 1, W - 1), (0, W // 2), (H // 2, 0), (H // 2, W // 2)):
        v[x, y] = rng.uniform(-1.0, 1.0)
    return v


def subnormal(H, W, seed=0):
    """Every cell subnormal: magnitudes from the smallest double up to 2^-1040."""
    return _scaled(_rng(H, W, seed), H, W, -1074, -1041)


def huge(H, W, seed=0):
    """Magnitudes 2^900 .. 2^961: products of two cells overflow, the step must not."""
    return _scaled(_rng(H, W, seed), H, W, 900, 960)


def nonfinite(H, W, seed=0, positions=()):
    """`signed`, then nan, +inf, -inf cycled over `positions` ((x, y) cells)."""
    v = signed(H, W, seed)
    for i, (x, y) in enumerate(positions):
        v[x, y] = NONFINITE_SEEDS[i % 3]
    return v


def make(cls, H, W, seed=0, positions=()):
    if cls == "nonfinite":
        return nonfinite(H, W, seed, positions)
    return globals()[cls](H, W, seed)


def ball_mask(shape, positions, radius):
    """Cells within Chebyshev distance `radius` of one of `positions`."""
    H, W = shape
    m = np.zeros((H, W), dtype=bool)
    for x, y in positions:
        m[max(x - radius, 0):x + radius + 1, max(y - radius, 0):y + radius + 1] = True
    return m


def _hex(x):
    return f"{float(x).hex()} (0x{np.float64(x).view(np.uint64):016x})"


def assert_same_bits(got, want, what=""):
    """got and want hold the same doubles bit for bit wherever want is not NaN, and NaN
    exactly where want does (payload and sign of a NaN are not compared: x86 and the GPU
    make different default NaNs)."""
    got = np.ascontiguousarray(got, dtype=np.float64)
    want = np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    bad = (np.isnan(got) != nan) | (~nan & (got.view(np.uint64) != want.view(np.uint64)))
    if bad.any():
        first = tuple(int(i) for i in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(np.count_nonzero(bad))} of {bad.size} cells differ, "
                             f"first at {first}: got {_hex(got[first])}, want {_hex(want[first])}")


def assert_sum_close(got, want_cells, what=""):
    """A kernel's sum of `want_cells` against math.fsum: within 1e-12 of the sum of the
    magnitudes (the summation error of per-lane, butterfly, partials order scales with
    sum |v|, not with |sum v|; for positive data this is the bound the suite always had)."""
    flat = np.asarray(want_cells, dtype=np.float64).ravel()
    want, scale = math.fsum(flat), math.fsum(np.abs(flat))
    assert abs(got - want) <= 1e-12 * scale, (what, float(got).hex(), want.hex(), scale)
