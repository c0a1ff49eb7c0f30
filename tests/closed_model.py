"""The contract of MM_FLOW_DIFFUSE_CLOSED (include/mpimodel.h) as plain numpy: elementwise
IEEE fp64 operations in the stated order, np.where for every select. A plain module, not a
conftest: tests/test_closed_cpu.py checks it against the oracle on the CPU,
tests/test_gpu_closed.py holds mm_closed_kernel to it bit for bit.

A cell is OPEN when it is inside the grid and f != 0.0 (+0 and -0 are both walls); everything
else is a wall. For the in-grid cell c = (x, y):

    cnt(c) = number of OPEN Moore neighbours of c                         (0..8)
    out(c) = f(c) * v(c)              if c is open and cnt(c) > 0, else 0 (by select)
    s(c)   = out(c) * 0.125           if cnt(c) == 8
             out(c) / (double)cnt(c)  if 1 <= cnt(c) <= 7
             0                        otherwise                           (by select)
    q(x,y) = s(x-1,y) + s(x+1,y)
    t(x,y) = q(x,y) + s(x,y)
    nb     = (t(x,y-1) + t(x,y+1)) + q(x,y)
    v'(c)  = (v(c) - out(c)) + nb     if c is open;  v(c), bit for bit, if c is a wall
"""
import numpy as np


def open_cells(f):
    return np.asarray(f, dtype=np.float64) != 0.0


def open_counts(f):
    """cnt: open Moore neighbours of every cell (cells outside the grid are walls)."""
    o = open_cells(f)
    H, W = o.shape
    p = np.zeros((H + 2, W + 2), dtype=np.int64)
    p[1:-1, 1:-1] = o
    box = sum(p[dx:dx + H, dy:dy + W] for dx in range(3) for dy in range(3))
    return box - o


def closed_step(v, f):
    v = np.ascontiguousarray(v, dtype=np.float64)
    f = np.ascontiguousarray(f, dtype=np.float64)
    assert v.shape == f.shape and v.ndim == 2
    H, W = v.shape
    is_open = open_cells(f)
    cnt = open_counts(f)
    emits = is_open & (cnt > 0)
    divides = (cnt >= 1) & (cnt <= 7)
    with np.errstate(all="ignore"):  # walls may hold anything: their products are selected away
        out = np.where(emits, f * v, 0.0)
        quot = out / np.where(divides, cnt, 1).astype(np.float64)
        s = np.where(cnt == 8, out * 0.125, np.where(divides, quot, 0.0))
        sp = np.zeros((H + 2, W + 2), dtype=np.float64)  # +0 outside the grid, by select
        sp[1:-1, 1:-1] = s
        q = sp[0:H, :] + sp[2:H + 2, :]       # rows x, padded columns -1..W
        t = q + sp[1:H + 1, :]
        nb = (t[:, 0:W] + t[:, 2:W + 2]) + q[:, 1:W + 1]
        new = (v - out) + nb
    return np.where(is_open, new, v)


def closed_steps(v, f, steps):
    for _ in range(steps):
        v = closed_step(v, f)
    return v


# ---- domains of the tests (True = open) ----------------------------------------
def domain(kind, H, W, seed=0):
    x, y = np.mgrid[0:H, 0:W]
    if kind == "open":
        return np.ones((H, W), dtype=bool)
    if kind == "checker":  # every open cell has its four diagonal neighbours: cnt = 4 inside
        return (x + y) % 2 == 0
    if kind == "one":
        m = np.zeros((H, W), dtype=bool)
        m[H // 2, W // 2] = True
        return m
    if kind == "random":
        return np.random.default_rng(77 + seed + 1000003 * H + W).random((H, W)) < 0.7
    if kind == "disc":
        r = 0.45 * min(H, W) + 0.5
        return (x - (H - 1) / 2.0) ** 2 + (y - (W - 1) / 2.0) ** 2 <= r * r
    if kind == "seams":
        # one-cell-wide wall lines with one-cell gaps on the strip seams (columns 127 / 128,
        # 255 / 256) and on the row-block seam (rows 7 / 8), wherever the grid has them
        m = np.ones((H, W), dtype=bool)
        for c in (127, 128, 255, 256):
            if c < W:
                m[:, c] = False
                m[(c % 5)::6, c] = True  # gaps
        for r in (7, 8):
            if r < H:
                m[r, :] = False
                m[r, (r % 3)::7] = True
        return m
    raise ValueError(kind)


def rates(mask, seed=0, negative=True):
    """Rates in [0.05, 0.3] on the open cells, one of them negative; 0 on the walls, of either
    sign."""
    H, W = mask.shape
    rng = np.random.default_rng(5 + seed + 1000003 * H + W)
    f = rng.uniform(0.05, 0.3, (H, W))
    idx = np.argwhere(mask)
    if negative and len(idx):
        x, y = idx[len(idx) // 2]
        f[x, y] = -0.125
    wall = np.where(rng.random((H, W)) < 0.5, -0.0, 0.0)
    return np.where(mask, f, wall)
