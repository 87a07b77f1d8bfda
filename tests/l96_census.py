"""The Lorenz-96 instantiation table restated in Python, and the census recipe
shared by test_l96_census_cpu.py (table vs ipmc_plan_sweep, oracle accept
counts) and test_gpu_l96_census.py (every compiled kernel vs the oracle).

ipmc_l96_dispatch.hpp compiles one kernel per state dim D of IPMC_L96_DIMS and
lanes per chain LPC in {1, 2, 4, 8, 16} with D % LPC == 0, M = D / LPC >= 2
components per lane and M * size <= 160 bytes, size being the storage of one
component: 8 for fp64 and for packed fp32 pairs (chains_per_lane = 2), 4 for
fp32.  The rule is written once, here; the CPU test pins it to the library.
"""
import functools

DIMS = (4, 6, 8, 10, 12, 16, 20, 24, 32, 36, 40, 48, 60, 64, 80, 128, 160, 256)
LPCS = (1, 2, 4, 8, 16)

# (dtype name, chains per lane group) -> bytes of storage per component
STORAGE = {("f64", 1): 8, ("f32", 1): 4, ("f32", 2): 8}
TABLE_SIZES = {("f64", 1): 46, ("f32", 1): 57, ("f32", 2): 46}


def compiled(D, lpc, size):
    return D in DIMS and lpc in LPCS and D % lpc == 0 and D // lpc >= 2 and (D // lpc) * size <= 160


def pairs(size):
    """Every compiled (D, LPC) at `size` bytes per component."""
    return [(D, lpc) for D in DIMS for lpc in LPCS if compiled(D, lpc, size)]


# the sweep census: every compiled (D, LPC, dtype name, chains per lane group)
SWEEP_CASES = [(D, lpc, dt, cpl) for (dt, cpl), size in STORAGE.items() for D, lpc in pairs(size)]
# the eval census: the eval kernels take their layout from the fp64 table
EVAL_CASES = [(D, lpc, dt) for dt in ("f64", "f32") for D, lpc in pairs(8)]

ARITHS = ("fma", "reference")

# the sweep recipe: 37 chains (a ragged last group at every LPC, a phantom
# partner in the packed layout), 7 RK4 steps (one unrolled iteration of 4 and
# a remainder of 3), 4 pCN steps
N_CHAINS, N_RK, BETA, SEED, STEP0, N_PCN = 37, 7, 0.25, 77, 5, 4


def case_id(case):
    return "-".join(str(x) for x in case)


def l96_op(D, arith, n_steps=N_RK):
    from ip_mcmc_amd import Lorenz96Operator

    return Lorenz96Operator(D, 8.0, dt=0.005, n_steps=n_steps, arith=arith)


def torch_dtype(dt):
    import torch

    return torch.float64 if dt == "f64" else torch.float32


@functools.lru_cache(maxsize=None)
def oracle_sweep(orc, D, dt, arith):
    """(operator, (U0, phi0, y, ginv, sq), the oracle's sweep) of the census
    recipe.  It depends on neither LPC nor the packing, so it is computed once
    per (D, dtype, arith) and shared, the oracle's outputs read-only."""
    from test_gpu_parity import _problem, _sweep_oracle

    op = l96_op(D, arith)
    dtype = torch_dtype(dt)
    prob = _problem(op, N_CHAINS, dtype, orc, seed=D)
    U0, phi0, y, ginv, sq = prob
    o = _sweep_oracle(orc, op, U0, phi0, y, ginv, sq, BETA, SEED, STEP0, N_PCN, dtype, want_sums=True)
    for a in o.values():
        a.setflags(write=False)
    return op, prob, o
