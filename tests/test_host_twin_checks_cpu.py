"""libipmc_host.so rejects what libipmc.so rejects, in the same words (include/ipmc_host.h).

Six entry points of the device library have a twin in the host library.  Each table below holds argument sets that
one of the checks the twins share turns down; every set goes to both libraries, and the two must answer with the
same status and, once the `ipmc_` / `ipmc_host_` prefix of the function name is taken off, the same message.
The device call also gets a workspace that is non-NULL and large enough, and a NULL stream, so only the shared
arguments decide.  Every set fails a check: nothing is launched and no pointer but `deltas` (host memory in both
libraries) is read, so the other pointers are dummies and no GPU is needed.
"""
import numpy as np
import pytest

from ip_mcmc_amd import _abi, _hostlib, _lib

DUMMY = 0x10000  # a non-NULL pointer that no call here dereferences
WS_BYTES = 1 << 20  # ipmc_smc_workspace asks for 16 * ceil(n / 1024) * n_deltas bytes: far less at n = 100
F64, F32 = _abi.F64, _abi.F32
NAN, INF = float("nan"), float("inf")


def _deltas(*values):
    return np.array(values, dtype=np.float64)


GOOD_DELTAS = _deltas(0.0, 0.5, 1.0)

# ipmc[_host]_pcn_draws(seed, chain_offset, n_chains, step0, n_steps, k, dtype, prior_sqrt, prior_chol, w, log_r, ..)
PCN_DRAWS = {
    "n_chains < 0": (1, 0, -1, 0, 4, 3, F64, DUMMY, None, DUMMY, DUMMY),
    "chain_offset < 0": (1, -1, 8, 0, 4, 3, F64, DUMMY, None, DUMMY, DUMMY),
    "n_steps < 0": (1, 0, 8, 0, -1, 3, F64, DUMMY, None, DUMMY, DUMMY),
    "k = 0": (1, 0, 8, 0, 4, 0, F64, DUMMY, None, DUMMY, DUMMY),
    "chain ids past 2^32": (1, 2**32 - 1, 2, 0, 4, 3, F64, DUMMY, None, DUMMY, DUMMY),
    "bad dtype": (1, 0, 8, 0, 4, 3, 7, DUMMY, None, DUMMY, DUMMY),
    "step0 + n_steps past 2^63": (1, 0, 8, 2**63 - 1, 2, 3, F64, DUMMY, None, DUMMY, DUMMY),
    "step0 past 2^63": (1, 0, 8, 2**63 + 1, 0, 3, F64, DUMMY, None, DUMMY, DUMMY),
    "w is NULL": (1, 0, 8, 0, 4, 3, F32, DUMMY, None, None, DUMMY),
    "both priors NULL": (1, 0, 8, 0, 4, 3, F64, None, None, DUMMY, DUMMY),
    "element count overflows": (1, 0, 2**32, 0, 2, 2**31 - 1, F64, DUMMY, None, DUMMY, DUMMY),
}

# ipmc[_host]_normal(seed, chain_offset, n_chains, step, k, dtype, out, ..)
NORMAL = {
    "k < 0": (1, 0, 8, 0, -1, F64, DUMMY),
    "n_chains < 0": (1, 0, -1, 0, 3, F64, DUMMY),
    "chain_offset < 0": (1, -1, 8, 0, 3, F64, DUMMY),
    "chain ids past 2^32": (1, 2**32, 1, 0, 3, F64, DUMMY),
    "bad dtype": (1, 0, 8, 0, 3, -1, DUMMY),
    "out is NULL": (1, 0, 8, 0, 3, F32, None),
}

# ipmc[_host]_uniform(seed, chain_offset, n_chains, step, out, ..)
UNIFORM = {
    "n_chains < 0": (1, 0, -1, 0, DUMMY),
    "chain_offset < 0": (1, -1, 8, 0, DUMMY),
    "chain ids past 2^32": (1, 1, 2**32, 0, DUMMY),
    "out is NULL": (1, 0, 8, 0, None),
}

# ipmc[_host]_temper_sums(phi, dtype, n, phi_ref, deltas, n_deltas, s1_out, s2_out, ..)
TEMPER_SUMS = {
    "n < 0": (DUMMY, F64, -1, 0.0, GOOD_DELTAS, 3, DUMMY, DUMMY),
    "n_deltas < 0": (DUMMY, F64, 100, 0.0, GOOD_DELTAS, -1, DUMMY, DUMMY),
    "n_deltas = 0": (DUMMY, F64, 100, 0.0, GOOD_DELTAS, 0, DUMMY, DUMMY),
    "n_deltas = 65": (DUMMY, F64, 100, 0.0, np.zeros(65), 65, DUMMY, DUMMY),
    "bad dtype": (DUMMY, 2, 100, 0.0, GOOD_DELTAS, 3, DUMMY, DUMMY),
    "phi is NULL": (None, F64, 100, 0.0, GOOD_DELTAS, 3, DUMMY, DUMMY),
    "deltas is NULL": (DUMMY, F32, 100, 0.0, None, 3, DUMMY, DUMMY),
    "s1_out is NULL": (DUMMY, F64, 100, 0.0, GOOD_DELTAS, 3, None, DUMMY),
    "s2_out is NULL": (DUMMY, F64, 100, 0.0, GOOD_DELTAS, 3, DUMMY, None),
    "deltas[0] < 0": (DUMMY, F64, 100, 0.0, _deltas(-0.25, 0.5, 1.0), 3, DUMMY, DUMMY),
    "deltas[2] is NaN": (DUMMY, F64, 100, 0.0, _deltas(0.0, 0.5, NAN), 3, DUMMY, DUMMY),
    "deltas[1] is inf": (DUMMY, F32, 100, 0.0, _deltas(0.0, INF, 1.0), 3, DUMMY, DUMMY),
}

# ipmc[_host]_temper_cumweights(phi, dtype, n, phi_ref, delta, cum_out, ..)
TEMPER_CUMWEIGHTS = {
    "n < 0": (DUMMY, F64, -1, 0.0, 0.5, DUMMY),
    "bad dtype": (DUMMY, 9, 100, 0.0, 0.5, DUMMY),
    "phi is NULL": (None, F64, 100, 0.0, 0.5, DUMMY),
    "cum_out is NULL": (DUMMY, F32, 100, 0.0, 0.5, None),
    "delta < 0": (DUMMY, F64, 100, 0.0, -1e-300, DUMMY),
    "delta is NaN": (DUMMY, F64, 100, 0.0, NAN, DUMMY),
    "delta is inf": (DUMMY, F32, 100, 0.0, INF, DUMMY),
}

# ipmc[_host]_systematic_ancestors(cum, n, u, n_out, anc_out, ..).  u = -0.0 lies in [0, 1): the set that carries it
# fails the check after the one on u
ANCESTORS = {
    "n < 0": (DUMMY, -1, 0.5, 10, DUMMY),
    "n_out < 0": (DUMMY, 10, 0.5, -1, DUMMY),
    "u = 1": (DUMMY, 10, 1.0, 10, DUMMY),
    "u < 0": (DUMMY, 10, -1e-300, 10, DUMMY),
    "u is NaN": (DUMMY, 10, NAN, 10, DUMMY),
    "u = -0.0, cum is NULL": (None, 10, -0.0, 10, DUMMY),
    "anc_out is NULL": (DUMMY, 10, 0.5, 10, None),
}

# name of the pair -> (table, what the device call takes after the shared arguments, the host call likewise)
PAIRS = {
    "pcn_draws": (PCN_DRAWS, (None,), (1,)),
    "normal": (NORMAL, (None,), ()),
    "uniform": (UNIFORM, (None,), ()),
    "temper_sums": (TEMPER_SUMS, (DUMMY, WS_BYTES, None), ()),
    "temper_cumweights": (TEMPER_CUMWEIGHTS, (DUMMY, WS_BYTES, None), ()),
    "systematic_ancestors": (ANCESTORS, (None,), ()),
}
CASES = [(pair, case) for pair, (table, _, _) in PAIRS.items() for case in table]


def _arg(a):
    return a.ctypes.data if isinstance(a, np.ndarray) else a


def _strip(message):
    return message.replace("ipmc_host_", "").replace("ipmc_", "")


@pytest.mark.parametrize("pair,case", CASES, ids=[f"{p}-{c}" for p, c in CASES])
def test_the_twins_reject_alike(pair, case):
    table, dev_tail, host_tail = PAIRS[pair]
    shared = tuple(_arg(a) for a in table[case])
    dev, host = _lib.lib(), _hostlib.lib()
    rc_dev = getattr(dev, "ipmc_" + pair)(*shared, *dev_tail)
    msg_dev = dev.ipmc_last_error().decode()
    rc_host = getattr(host, "ipmc_host_" + pair)(*shared, *host_tail)
    msg_host = host.ipmc_host_last_error().decode()
    assert rc_dev != _abi.OK and rc_dev == rc_host, (rc_dev, msg_dev, rc_host, msg_host)
    assert msg_dev and _strip(msg_dev) == _strip(msg_host)
