"""Burgers off the default grid and observation windows: a numpy reference and
the operator set shared by test_burgers_geometry_cpu.py (oracle vs numpy) and
test_gpu_burgers_geometry.py (HIP kernels vs oracle).

`burgers_numpy` restates the forward map in plain numpy float64 from the
reference's rusanov.py:6-109 (SSPRK2, Rusanov flux, outflow ghosts, the
overshooting CFL loop) and utilities.py:44-109 (Riemann IC with a strict `<`,
Measurer = scale * np.trapz over searchsorted windows).  It calls neither the
oracle nor the library; the only thing it takes from a BurgersOperator is its
parameters.

The operators are rarefactions (left state -0.95, right state 0.9), so the
final state varies across the middle ~40 % of the domain and a window there
sees an index error; a shock would leave every window constant.
"""
import functools
import math

import numpy as np

_trapz = getattr(np, "trapezoid", None) or np.trapz


# ------------------------------------------------------------ numpy reference
def burgers_numpy(op, u, input_dtype=np.float64, windows=None):
    """(G, iters, v_final) of BurgersOperator `op` at u, float64 arithmetic in
    the reference's operation order.  input_dtype rounds theta0, u and the cell
    centres first (the values a float32 evaluation starts from; the strict `<`
    of the IC is discontinuous in them).  windows overrides op's (lo, hi)."""
    rd = lambda a: np.asarray(a, dtype=np.float64).astype(input_dtype).astype(np.float64)
    th, x, u = rd(op.theta0), rd(op.x), rd(u)
    left, right, jump = 1.0 + (th[0] + u[0]), th[1] + u[1], th[2] + u[2]
    w = np.where(x < jump, left, right)  # utilities.py:59-62 on every centre, ghosts included
    dx, nu = float(op.dx), float(op.nu)

    def rate(w):
        a, b = w[:-1], w[1:]
        # rusanov.py:92-96 with f(w) = .5 * w * w, f'(w) = w
        F = 0.5 * ((0.5 * a) * a + (0.5 * b) * b) - (0.5 * np.maximum(np.abs(a), np.abs(b))) * (b - a)
        r = np.zeros_like(w)
        r[1:-1] = (F[1:] - F[:-1]) / (-dx)  # rusanov.py:76-90
        if nu != 0.0:
            r[1:-1] = r[1:-1] + (nu / (dx * dx)) * ((w[2:] - (w[1:-1] + w[1:-1])) + w[:-2])
        return r

    def step(w, dt):  # rusanov.py:62-74
        ws = w + dt * rate(w)
        ws[0], ws[-1] = ws[1], ws[-2]
        ws = ws + dt * rate(ws)
        w = (w + ws) / 2
        w[0], w[-1] = w[1], w[-2]
        return w

    iters, valid = 0, True
    if op.dt_mode == "cfl":
        t = 0.0
        while t < op.T:  # rusanov.py:40-45, 102-109
            if iters >= op.max_iter:
                valid = False
                break
            dt = op.cfl * dx / np.max(np.abs(w[1:-1]))
            t += dt
            w = step(w, dt)
            iters += 1
    else:
        for _ in range(op.n_steps):
            if not np.max(np.abs(w[1:-1])) * op.dt <= op.cfl * dx:
                valid = False
                break
            w = step(w, op.dt)
            iters += 1
    v = w[1:-1]
    if windows is None:
        windows = list(zip(op.win_lo, op.win_hi))
    if valid:  # utilities.py:100-109
        G = np.array([op.meas_scale * _trapz(v[lo:hi], dx=op.meas_dx) for lo, hi in windows])
    else:
        G = np.full(len(windows), np.nan)
    return G, iters, v


# --------------------------------------------------------------- the windows
NT_CLASSES = (1, 7, 8, 9, 15, 16, 17, 24, 127, 128)  # and <= 0: the regimes and edges of the pairwise sum


def nt_classes(N):
    """The trapezoid-term counts nt = hi - lo - 1 a grid of N cells has room for."""
    return [nt for nt in NT_CLASSES if nt + 1 <= N]


def windows_for(N, q_mode="std"):
    """(lo, hi) cell windows: every nt class that fits, once around the middle
    (inside the rarefaction) and once elsewhere; a window starting at cell 0,
    one ending at cell N, the whole domain when it fits 129 cells, an empty
    (hi == lo), a one-cell (nt = 0) and a reversed (hi < lo) window, and a
    duplicate.  The windows around the middle overlap each other."""
    if q_mode == "one":
        c = min(N, 10)
        lo = (N - c) // 2
        return [(lo, lo + c)]
    cls = nt_classes(N)
    win = []
    for k, nt in enumerate(cls):
        c = nt + 1
        mid = (N - c) // 2
        win.append((mid, mid + c))
        off = ((N - c) * (2 * k + 1)) // (2 * len(cls))  # spread over the domain
        win.append((off, off + c))
    cmax = cls[-1] + 1
    win.append((0, cmax))
    c2 = (cls[-2] if len(cls) > 1 else cls[-1]) + 1
    win.append((N - c2, N))
    if N - 1 <= 128:
        win.append((0, N))
    a = N // 3
    win += [(a, a), (a, a + 1), (a + 2, a)]
    win.append(win[2 * (len(cls) - 1)])  # the middle window of the widest class again
    if q_mode == "max":  # kBurQMax windows: a 17-cell window slid across the domain
        k = 64 - len(win)
        win += [((N - 17) * i // (k - 1), (N - 17) * i // (k - 1) + 17) for i in range(k)]
    assert len(win) <= 64
    return win


def points_and_intervals(N, domain, windows):
    """Measurer arguments whose searchsorted limits are exactly `windows`:
    each edge lies on a cell face, half a cell from the nearest centres."""
    a, b = domain
    dxc = (b - a) / N
    face = lambda i: a + i * dxc
    pts = np.array([0.5 * (face(lo) + face(hi)) for lo, hi in windows])
    wid = np.array([face(hi) - face(lo) for lo, hi in windows])
    return pts, wid


# ------------------------------------------------------------- the operators
DEFAULT_DOMAIN = (-1.0, 1.0)
GRIDS = [(4, DEFAULT_DOMAIN), (8, DEFAULT_DOMAIN), (12, DEFAULT_DOMAIN), (16, DEFAULT_DOMAIN),
         (24, DEFAULT_DOMAIN), (64, (0.0, 3.0)), (68, DEFAULT_DOMAIN), (132, DEFAULT_DOMAIN),
         (136, DEFAULT_DOMAIN), (200, DEFAULT_DOMAIN), (264, DEFAULT_DOMAIN), (512, DEFAULT_DOMAIN)]
NU = 2e-3
CFL = 0.5


def _cases():
    out = []
    for g, (N, dom) in enumerate(GRIDS):
        scale = (10.0, 7.5, 0.3)[g % 3]
        nu_fixed = (0.0, NU) if g % 2 == 0 else (NU, 0.0)
        variants = [("cfl", "reference", 0.0), ("cfl", "fma", 0.0), ("cfl", "reference", NU), ("cfl", "fma", NU),
                    ("fixed", "reference", nu_fixed[0]), ("fixed", "fma", nu_fixed[1])]
        for mode, arith, nu in variants:
            out.append(dict(N=N, domain=dom, q_mode="std", dt_mode=mode, arith=arith, nu=nu, meas_scale=scale))
    for N, q_mode in ((8, "one"), (136, "one"), (264, "max"), (512, "max")):
        for arith, nu in (("reference", 0.0), ("fma", NU)):
            out.append(dict(N=N, domain=DEFAULT_DOMAIN, q_mode=q_mode, dt_mode="cfl", arith=arith, nu=nu,
                            meas_scale=2.5))
    for c in out:
        c["id"] = "N{N}-{q_mode}-{dt_mode}-{arith}-nu{nu:g}".format(**c) + ("-dom03" if c["domain"][0] == 0.0 else "")
    return out


CASES = _cases()
CASE_IDS = [c["id"] for c in CASES]


def case_by_id(cid):
    return CASES[CASE_IDS.index(cid)]


def base_u(domain):
    L = domain[1] - domain[0]
    return np.array([0.05, -0.1, 0.03 * L])


def operator_kwargs(case, **over):
    """BurgersOperator arguments of a case: prior mean (-2, 1, mid) and T =
    0.45 L/2 (the fan then spans about [mid - 0.18 L, mid + 0.23 L]); the fixed
    mode's dt keeps max|w| dt <= cfl dx up to max|w| = 1.25."""
    N, (a, b) = case["N"], case["domain"]
    L = b - a
    win = windows_for(N, case["q_mode"])
    pts, wid = points_and_intervals(N, (a, b), win)
    T = 0.45 * L / 2
    dt = 0.8 * CFL * (L / N)
    kw = dict(prior_mean=(-2.0, 1.0, 0.5 * (a + b)), domain=(a, b), N=N, T=T, points=pts, interval=wid,
              meas_scale=case["meas_scale"], dt_mode=case["dt_mode"], dt=dt, n_steps=int(math.ceil(T / dt)),
              cfl=CFL, nu=case["nu"], arith=case["arith"])
    kw.update(over)
    return kw


def make_operator(case, **over):
    from ip_mcmc_amd import BurgersOperator

    op = BurgersOperator(**operator_kwargs(case, **over))
    win = windows_for(case["N"], case["q_mode"])
    got = list(zip(op.win_lo.tolist(), op.win_hi.tolist()))
    assert got == win, (case["id"], got, win)  # searchsorted gave the intended cells
    return op


def _on_centre(op, i, dtype):
    """u[2] with theta0[2] + u[2] == x[i] in `dtype` (and exactly, so the
    float64 reference on the rounded inputs sees the same tie)."""
    th, xi = dtype(op.theta0[2]), dtype(op.x[i])
    u2 = dtype(xi - th)
    assert dtype(th + u2) == xi and float(th) + float(u2) == float(xi), (op.N, i, dtype)
    return float(u2)


def on_centre_cells(N):
    """Ghost-inclusive indices of the cells the jump is put on: in the right
    half (within a factor 2 of the domain (0, 3)'s midpoint, so x[i] - mid is
    exact) and the first interior cell left of it."""
    i = min(N, 1 + (6 * N) // 10)
    return sorted({i, max(1, i - 1)})


def input_rows(op, dtype=np.float64, seed=0):
    """[R, 3] float64 rows u (values of `dtype`): the base state, three random
    ones, the jump outside the domain on either side (a constant state), the
    jump exactly on a cell centre, and for dt_mode='fixed' one that trips the
    CFL guard."""
    L = op.N * float(op.dx)
    base = base_u((0.0, L))
    rng = np.random.default_rng(seed)
    rows = [base] + [base + np.array([0.05, 0.05, 0.05 * L]) * rng.normal(size=3) for _ in range(3)]
    rows += [np.array([base[0], base[1], -0.7 * L]), np.array([base[0], base[1], 0.7 * L])]
    for i in on_centre_cells(op.N):
        rows.append(np.array([base[0], base[1], _on_centre(op, i, dtype)]))
    if op.dt_mode == "fixed":
        rows.append(np.array([-1.0, base[1], base[2]]))  # left state -2: max|w| dt > cfl dx
    return np.asarray(rows, dtype=np.float64).astype(dtype).astype(np.float64)


@functools.lru_cache(maxsize=None)
def numpy_results(cid, dtype_name):
    """(rows, [burgers_numpy(row)]) of a case on inputs rounded to dtype: computed once, shared."""
    dtype = np.float32 if dtype_name == "float32" else np.float64
    op = make_operator(case_by_id(cid))
    rows = input_rows(op, dtype)
    return rows, [burgers_numpy(op, r, input_dtype=dtype) for r in rows]


# ------------------------------------------------------------------- layouts
def layout(N, lanes=0):
    """(cells per lane, lanes per group) the library runs N cells on, or None:
    8 cells per lane if N is a multiple of 8 and fits 64 lanes, else 4;
    lanes > 0 forces N / lanes cells per lane (4 or 8)."""
    def fit(c):
        if c <= 0 or N % c:
            return None
        for g in (16, 32, 64):
            if N // c <= g:
                return (c, g)
        return None

    if lanes > 0:
        return fit(N // lanes) if N % lanes == 0 and N // lanes in (4, 8) else None
    return fit(8) or fit(4)
