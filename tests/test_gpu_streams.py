"""Every entry point on a non-default stream, behind pending work.

include/ipmc.h promises that a call is asynchronous on the stream it is given
and never synchronises the host.  The rest of the suite calls on the null
stream with the device synchronised around each call, where a launch or memset
on the wrong stream cannot show.  Here every case goes through one harness
(_behind):

  stage    true inputs in src tensors; the buffers the entry point sees hold
           poison (NaN, -1, 0xFF bytes); device synchronised
  pend     on a non-blocking stream S: busy work (torch.mm on a fixed f64
           matrix), then in.copy_(src), then poison on every output, in/out
           accumulator, scratch and workspace, then the event `ready`
  call     with S's handle; `ready` must not have fired before the call (it
           was enqueued behind pending work) nor after it (it did not wait);
           wrappers that return host values are exempt from the second check
  snapshot clones of the outputs on S, S.synchronize() alone
  compare  bit for bit (unsigned views, NaN payloads count) with an independent
           twin (the CPU oracle, libipmc_host, numpy, backend="host") or with
           the same call on the null stream between two device synchronises

A leading memset or zero kernel on the wrong stream runs before the poison and
the counts come out poisoned; a trailing combine reads unwritten partials and
its output is poisoned afterwards; a middle launch reads poisoned scratch.
test_negative_control shows the method sees a launch on the null stream.

The forward maps' own constants (ipmc_model.x0 / theta0 / A, cached by
ObservationOperator.model) are staged before the busy work; everything else an
entry point reads is written on S.

Calibration (the `cal` fixture; nothing fixed in advance): the busy unit is
timed with events on S, the slowest enqueue on an idle stream with
time.perf_counter, and the busy work lasts at least 20 times that enqueue --
in fact 20 times the slowest enqueue of a whole case (its staging writes, the
event and the call), which is the longer of the two.  Measured on an MI355X
over five runs: busy unit (one 2048^2 f64 torch.mm) 0.27-0.32 ms; slowest
enqueue 0.10-0.14 ms (ipmc_pooled_sort, a memset and 27 launches; the others
0.009-0.026 ms); slowest staging + call 0.14-0.20 ms (the same case); busy
work 11-14 units = 2.9-4.2 ms per stream and case.

The streams are chosen, not taken as they come: the runtime spreads its
streams over a few hardware queues (four by default), and two streams on one queue
run in submission order, so a launch on the null stream is serialised into the
right place when S shares the null stream's queue -- the negative control then
does not differ (seen in a whole-suite run, where earlier tests had used up
other streams of torch's pool).  The fixture probes candidates and keeps two
that run beside the null stream and beside each other; it fails if there are
none.

What the Python tier can and cannot show: a wrapper that returns host values
(support, marginal_histograms, convergence, MCMCSampler.run, ...) or copies a
host array to the device first waits for S before its later launches, so a
launch of its own on the null stream may still come out right there; those
cases pin that the wrapper reads inputs produced on S and returns what the
default stream returns, and the C-ABI tier pins the launches.
"""
import ctypes as C
import functools
import math
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

BUSY_N = 2048  # the busy unit: one torch.mm of a BUSY_N x BUSY_N f64 matrix with itself
MARGIN = 20  # busy work lasts MARGIN x the slowest enqueue


# ----------------------------------------------------------------- plumbing
def _ipmc(name, *args):
    from ip_mcmc_amd._lib import call

    return call(name, *args)


def _abi():
    from ip_mcmc_amd import _abi

    return _abi


def _npd(dtype):
    return np.float32 if dtype == torch.float32 else np.float64


def _abi_dtype(dtype):
    return _abi().F32 if dtype == torch.float32 else _abi().F64


def _poison(t):
    if t.dtype.is_floating_point:
        t.fill_(float("nan"))
    elif t.dtype == torch.uint8:
        t.fill_(255)
    else:
        t.fill_(-1)


def _nan(shape, npd):
    """The poison of a float buffer as numpy (torch's NaN bits)."""
    return torch.full(shape, float("nan"), dtype=torch.float32 if npd == np.float32 else torch.float64).numpy()


def _bits(x):
    """An unsigned-integer view of a tensor, array or scalar: equality of these is equality of the bits."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    a = np.ascontiguousarray(np.asarray(x)).reshape(-1)
    if a.dtype == np.bool_:
        a = a.astype(np.uint8)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _flatten(r):
    """The tensors / arrays of a wrapper's return value, in a fixed order."""
    if r is None:
        return []
    if isinstance(r, dict):
        return [x for key in sorted(r) for x in _flatten(r[key])]
    if isinstance(r, (tuple, list)):
        return [x for part in r for x in _flatten(part)]
    if isinstance(r, (torch.Tensor, np.ndarray)):
        return [r]
    if hasattr(r, "particles") and hasattr(r, "temperatures"):  # smc.SMCResult
        return _flatten([r.particles, r.phi, r.temperatures, r.ess, r.log_evidence_increments, r.accept_rate,
                         r.n_stages])
    return [np.asarray(r)]


class _Case:
    """One call and its buffers.  copies: (buffer, src) pairs written on the stream behind the busy work;
    poison: what is poisoned there after them; outs: the device tensors compared (returns=True: what the
    call returns instead); host: page-locked host tensors compared; twin: () -> the expected arrays."""

    def __init__(self, dev):
        self.dev = dev
        self.copies, self.poison, self.outs, self.host, self.keep = [], [], [], [], []
        self.call = self.twin = None
        self.returns = False
        self.host_values = False  # the wrapper returns host values: it has to wait for the stream

    def inp(self, a, dtype=None):
        src = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        src = src.to(self.dev) if dtype is None else src.to(self.dev, dtype)
        buf = torch.empty_like(src)
        self.copies.append((buf, src))
        return buf

    def inout(self, a, dtype=None):
        buf = self.inp(a, dtype)
        self.outs.append(buf)
        return buf

    def scratch(self, shape, dtype):
        t = torch.empty(shape, dtype=dtype, device=self.dev)
        self.poison.append(t)
        return t

    def out(self, shape, dtype):
        t = self.scratch(shape, dtype)
        self.outs.append(t)
        return t


def _results(c, ret):
    return (_flatten(ret) if c.returns else list(c.outs))


def _write_inputs(c):
    """On the current stream: the true inputs into the buffers the call reads, poison into all it writes."""
    for dst, src in c.copies:
        dst.copy_(src)
    for t in c.poison:
        _poison(t)


def _serial(c):
    """The synchronous path the rest of the suite pins: the same buffers, the null stream, the device
    synchronised before and after.  Also loads the code objects before the timed call."""
    for h in c.host:
        _poison(h)
    _write_inputs(c)
    torch.cuda.synchronize()
    ret = c.call(0)
    torch.cuda.synchronize()
    return [_bits(x.clone() if isinstance(x, torch.Tensor) else x) for x in _results(c, ret) + c.host]


def _behind(cal, groups, handle=None, in_ctx=False):
    """The harness.  groups: [(stream, [cases])]; each stream gets its own busy work, the calls of the
    streams are interleaved from the host.  handle: the stream handle passed instead of the stream's own
    (the negative control).  in_ctx: call inside `with torch.cuda.stream(S)` (the Python tier).
    Returns {id(case): bit views of its outputs}."""
    # stage
    for _, cases in groups:
        for c in cases:
            for dst, _src in c.copies:
                _poison(dst)
            for h in c.host:
                _poison(h)
    torch.cuda.synchronize()
    # pend
    ready = []
    for S, cases in groups:
        with torch.cuda.stream(S):
            cal.busy(S)
            for c in cases:
                _write_inputs(c)
            ev = torch.cuda.Event()
            ev.record(S)
            ready.append(ev)
    # call
    order = [(S, cases[i]) for i in range(max(len(cs) for _, cs in groups)) for S, cases in groups
             if i < len(cases)]
    rets = {}
    assert not any(ev.query() for ev in ready), "the busy work drained before the call: nothing was pending"
    for S, c in order:
        h = S.cuda_stream if handle is None else handle
        if in_ctx:
            with torch.cuda.stream(S):
                rets[id(c)] = c.call(h)
        else:
            rets[id(c)] = c.call(h)
    if not any(c.host_values for _, c in order):
        assert not any(ev.query() for ev in ready), "the call returned after the stream drained: it waited"
    # snapshot
    snaps = {}
    for S, cases in groups:
        with torch.cuda.stream(S):
            for c in cases:
                snaps[id(c)] = [x.clone() if isinstance(x, torch.Tensor) and x.is_cuda else x
                                for x in _results(c, rets[id(c)])]
    for S, _ in groups:
        S.synchronize()
    # compare (the caller): bit views
    return {id(c): [_bits(x) for x in snaps[id(c)] + c.host] for _, c in order}


def _same(got, want):
    return len(got) == len(want) and all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


def _check(cal, c, in_ctx=False):
    sync = _serial(c)
    got = _behind(cal, [(cal.S, [c])], in_ctx=in_ctx)[id(c)]
    want = sync if c.twin is None else [_bits(x) for x in c.twin()]
    bad = [i for i in range(max(len(got), len(want)))
           if i >= len(got) or i >= len(want) or not _same([got[i]], [want[i]])]
    assert not bad, (f"outputs {bad} behind pending work differ from the "
                     f"{'synchronous path' if c.twin is None else 'twin'}; synchronous path == expected: "
                     f"{_same(sync, want)}")


# -------------------------------------------------------------- calibration
class _Calibration:
    def __init__(self, dev, orc):
        self.dev = dev
        self.a = torch.from_numpy(np.random.default_rng(0).random((BUSY_N, BUSY_N))).to(dev)
        self.flag = torch.zeros(8, device=dev)
        self.scratch = {}
        self.count = 8  # for the probes below only; set from the measurements afterwards
        self.S, self.S2 = self._pick_streams()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = 16
        with torch.cuda.stream(self.S):
            e0.record(self.S)
            for _ in range(reps):
                torch.mm(self.a, self.a, out=self.scratch[self.S.cuda_stream])
            e1.record(self.S)
        self.S.synchronize()
        self.unit_ms = e0.elapsed_time(e1) / reps
        # the slowest enqueue on an idle stream
        cands = {
            "ipmc_pooled_sort": _sort_case(dev, torch.float64),
            "ipmc_temper_cumweights": _cumweights_case(dev, torch.float64),
            "ipmc_hist1d": _hist1d_case(dev, torch.float64),
            "ipmc_pcn_run": _sweep_case(dev, orc, "l96_8", torch.float64, run=1),
            "ipmc_burn_in": _burn_in_case(dev, torch.float64),
        }
        self.enqueue_ms, self.case_ms = {}, {}
        for name, c in cands.items():
            _serial(c)
            worst = worst_case = 0.0
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                c.call(self.S.cuda_stream)
                worst = max(worst, time.perf_counter() - t0)
                # the whole enqueue of a case: its staging writes, the event and the call
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with torch.cuda.stream(self.S):
                    _write_inputs(c)
                    torch.cuda.Event().record(self.S)
                c.call(self.S.cuda_stream)
                worst_case = max(worst_case, time.perf_counter() - t0)
            self.enqueue_ms[name], self.case_ms[name] = 1e3 * worst, 1e3 * worst_case
        torch.cuda.synchronize()
        self.slowest_name = max(self.enqueue_ms, key=self.enqueue_ms.get)
        self.slowest_ms = self.enqueue_ms[self.slowest_name]
        self.slowest_case_ms = max(self.case_ms.values())
        # the pending work has to outlast the staging writes of a case as well as its call
        self.count = max(1, math.ceil(MARGIN * max(self.slowest_ms, self.slowest_case_ms) / self.unit_ms))
        print(f"\n[streams] busy unit {self.unit_ms:.4f} ms, slowest enqueue {self.slowest_ms:.4f} ms "
              f"({self.slowest_name}; all: {self.enqueue_ms}), slowest staging + call {self.slowest_case_ms:.4f} ms "
              f"({self.case_ms}), busy work {self.count} units = {self.count * self.unit_ms:.3f} ms")

    def _beside(self, busy_stream, other):
        """Does work on `other` run while busy work is pending on busy_stream?  The runtime spreads its
        streams over a few hardware queues; two streams on one queue run in submission order, and a launch
        on the wrong one of them would be serialised into the right place and go unseen."""
        torch.cuda.synchronize()
        with torch.cuda.stream(busy_stream):
            self.busy(busy_stream)
            ready = torch.cuda.Event()
            ready.record(busy_stream)
        with torch.cuda.stream(other):
            self.flag.fill_(1.0)
            probe = torch.cuda.Event()
            probe.record(other)
        beside = False
        while not ready.query():
            if probe.query():
                beside = True
                break
        torch.cuda.synchronize()
        return beside

    def _pick_streams(self):
        """Two streams of torch's pool that run beside the null stream and beside each other."""
        null = torch.cuda.default_stream(self.dev)
        picked, seen = [], set()
        for _ in range(64):
            s = torch.cuda.Stream(self.dev)
            if s.cuda_stream in seen:
                continue
            seen.add(s.cuda_stream)
            self.scratch[s.cuda_stream] = torch.empty_like(self.a)
            with torch.cuda.stream(s):  # load the GEMM and its workspace on this stream
                self.busy(s)
            if self._beside(s, null) and all(self._beside(s, p) and self._beside(p, s) for p in picked):
                picked.append(s)
                if len(picked) == 2:
                    break
        assert len(picked) == 2, ("found no two streams that run beside the null stream and each other: on "
                                  "streams that share a hardware queue the method cannot see a wrong stream")
        self.scratch = {s.cuda_stream: self.scratch[s.cuda_stream] for s in picked}
        print(f"\n[streams] picked 2 of {len(seen)} candidate streams ({len(seen) - 2} share a queue with the null "
              "stream or with the first pick)")
        return picked

    def busy(self, S):
        out = self.scratch[S.cuda_stream]
        for _ in range(self.count):
            torch.mm(self.a, self.a, out=out)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def cal(dev, orc):
    return _Calibration(dev, orc)


def test_calibration(cal):
    """The busy work is MARGIN x the slowest enqueue and really is pending when a case is enqueued."""
    assert cal.unit_ms > 0 and cal.slowest_ms > 0
    assert cal.count * cal.unit_ms >= MARGIN * cal.slowest_ms
    with torch.cuda.stream(cal.S):
        cal.busy(cal.S)
        ev = torch.cuda.Event()
        ev.record(cal.S)
    assert not ev.query()
    cal.S.synchronize()
    assert ev.query()


# -------------------------------------------------------------- C-ABI cases
@functools.lru_cache(maxsize=None)
def _op(name):
    from ip_mcmc_amd import (BurgersOperator, LinearOperator, Lorenz63Operator, Lorenz96Operator,
                             TwoScaleLorenz96Operator)

    rng = np.random.default_rng(3)
    if name == "lin":
        return LinearOperator(rng.normal(size=(3, 5)), rng.normal(size=5))
    if name == "l63":
        return Lorenz63Operator(x0=(1.0, 2.0, 20.0), dt=0.01, n_steps=40)
    if name == "l96_8":
        return Lorenz96Operator(8, 8.0, dt=0.005, n_steps=40)
    if name == "l96_40":
        return Lorenz96Operator(40, 8.0, dt=0.005, n_steps=40)
    if name == "burgers":
        return BurgersOperator(N=32, dt_mode="fixed", dt=5e-3, n_steps=40)
    if name == "ts":
        return TwoScaleLorenz96Operator(K=6, J=4, x0=rng.normal(size=30), dt=0.004, n_steps=40)
    raise KeyError(name)


OPS = ["lin", "l63", "l96_8", "l96_40", "burgers", "ts"]
FAMILIES = ["lin", "l63", "l96_8", "burgers", "ts"]
DTYPES = [torch.float64, torch.float32]


def _normal_case(dev, orc, dtype):
    c = _Case(dev)
    step = (1 << 33) + 7
    out = c.out((300, 7), dtype)
    c.call = lambda h: _ipmc("ipmc_normal", 99, 5, 300, step, 7, _abi_dtype(dtype), out.data_ptr(), h)
    c.twin = lambda: [orc.normals(99, 5, 300, step, 7).astype(_npd(dtype))]
    return c


def _uniform_case(dev, orc):
    c = _Case(dev)
    step = (1 << 33) + 7
    out = c.out((300,), torch.float64)
    c.call = lambda h: _ipmc("ipmc_uniform", 99, 5, 300, step, out.data_ptr(), h)
    c.twin = lambda: [orc.uniforms(99, 5, 300, step)]
    return c


def _draws_case(dev, dtype, chol):
    from ip_mcmc_amd import _hostlib

    c = _Case(dev)
    k, n, steps, npd = 5, 77, 3, _npd(dtype)
    rng = np.random.default_rng(5)
    sq = (0.5 + rng.random(k)).astype(npd)
    A = rng.normal(size=(k, k)) / np.sqrt(k)
    L = np.linalg.cholesky(0.3 * np.eye(k) + A @ A.T).astype(npd)
    p = c.inp(L if chol else sq)
    w = c.out((steps, n, k), dtype)
    lr = c.out((steps, n), torch.float64)
    c.call = lambda h: _ipmc("ipmc_pcn_draws", 17, 3, n, 41, steps, k, _abi_dtype(dtype),
                             None if chol else p.data_ptr(), p.data_ptr() if chol else None, w.data_ptr(),
                             lr.data_ptr(), h)
    c.twin = lambda: list(_hostlib.pcn_draws(17, 3, n, 41, steps, k, npd, None if chol else sq,
                                             L if chol else None))
    return c


def _eval_problem(orc, op, dtype, n=67):
    npd = _npd(dtype)
    rng = np.random.default_rng(11)
    U = (0.3 * rng.normal(size=(n, op.k))).astype(npd)
    y = (np.nan_to_num(orc.forward(op, U[:1], npd)[0].astype(np.float64)) + 0.1 * rng.normal(size=op.q)).astype(npd)
    ginv = (1.0 / (0.1 + rng.random(op.q))).astype(npd)
    return U, y, ginv


def _forward_case(dev, orc, name, dtype):
    op, c = _op(name), _Case(dev)
    U, _, _ = _eval_problem(orc, op, dtype)
    m, _ = op.model(dtype, dev)
    u = c.inp(U)
    g = c.out((U.shape[0], op.q), dtype)
    c.call = lambda h: _ipmc("ipmc_forward", C.byref(m), _abi_dtype(dtype), U.shape[0], u.data_ptr(), g.data_ptr(), h)
    c.twin = lambda: [orc.forward(op, U, _npd(dtype))]
    return c


def _potential_case(dev, orc, name, dtype):
    op, c = _op(name), _Case(dev)
    U, y, ginv = _eval_problem(orc, op, dtype)
    m, _ = op.model(dtype, dev)
    u, yt, gt = c.inp(U), c.inp(y), c.inp(ginv)
    phi = c.out((U.shape[0],), dtype)
    c.call = lambda h: _ipmc("ipmc_potential", C.byref(m), _abi_dtype(dtype), U.shape[0], u.data_ptr(), yt.data_ptr(),
                             gt.data_ptr(), phi.data_ptr(), h)
    c.twin = lambda: [orc.potential(op, U, y, ginv, _npd(dtype))]
    return c


def _init_phi_case(dev, orc, dtype):
    op, c = _op("l96_40"), _Case(dev)
    U, y, ginv = _eval_problem(orc, op, dtype, n=90)
    rs = np.linspace(0.5, 2.0, op.k).astype(_npd(dtype))
    m, _ = op.model(dtype, dev)
    u, yt, gt, rt = c.inp(U), c.inp(y), c.inp(ginv), c.inp(rs)
    phi = c.out((90,), dtype)
    s = _abi().IpmcSweep()
    s.dtype, s.n_chains, s.u, s.phi = _abi_dtype(dtype), 90, u.data_ptr(), phi.data_ptr()
    s.y, s.gamma_inv, s.reg_scale = yt.data_ptr(), gt.data_ptr(), rt.data_ptr()
    c.call = lambda h: _ipmc("ipmc_init_phi", C.byref(m), C.byref(s), h)
    c.twin = lambda: [orc.init_phi(op, U, y, ginv, reg_scale=rs)]
    return c


def _sweep_case(dev, orc, name, dtype, n_steps=3, spec=1, lanes=0, cpl=0, sums=False, sched=False, run=None):
    """ipmc_pcn_sweep of 77 chains, every in/out buffer non-trivial; run = 0 / 1: ipmc_pcn_run, 3 blocks of
    2 steps with sample_every = run."""
    op, c, npd, n = _op(name), _Case(dev), _npd(dtype), 77
    k = op.k
    rng = np.random.default_rng(7)
    U0 = (0.2 * rng.normal(size=(n, k))).astype(npd)
    g = np.nan_to_num(orc.forward(op, 0.1 * rng.normal(size=(1, k)))[0])
    y = (g + 0.05 * rng.normal(size=op.q)).astype(npd)
    ginv = np.full(op.q, 0.3 / 0.05).astype(npd)
    sq = (0.5 + rng.random(k)).astype(npd)
    phi0 = orc.potential(op, U0, y, ginv, npd)
    acc0 = (np.arange(n) % 4).astype(np.int64)
    calls0 = acc0 + 5
    total = 6 if run is not None else n_steps
    sch = None
    if sched:
        b = np.linspace(0.1, 0.4, max(total, 1))
        sch = np.ascontiguousarray(np.stack([b, np.sqrt(1 - b**2)], axis=1))
    sum0 = (rng.normal(size=(n, k)), rng.random((n, k))) if sums else None
    n_s = 1 if run is None else (3 if run == 0 else 6)

    m, _ = op.model(dtype, dev)
    u, phi, acc, calls = c.inout(U0), c.inout(phi0), c.inout(acc0), c.inout(calls0)
    yt, gt, st = c.inp(y), c.inp(ginv), c.inp(sq)
    samp = c.out((n, n_s, k), dtype)
    s = _abi().IpmcSweep()
    s.dtype, s.lanes_per_chain, s.chains_per_lane, s.spec_width = _abi_dtype(dtype), lanes, cpl, spec
    s.n_chains, s.chain_offset = n, 2
    s.u, s.phi, s.accepts, s.calls = u.data_ptr(), phi.data_ptr(), acc.data_ptr(), calls.data_ptr()
    s.y, s.gamma_inv, s.prior_sqrt = yt.data_ptr(), gt.data_ptr(), st.data_ptr()
    s.beta, s.contraction = 0.3, float(np.sqrt(1 - 0.3**2))
    if sch is not None:
        s.beta_schedule = c.inp(sch).data_ptr()
    s.seed, s.step0, s.n_steps = 1234, 10, n_steps
    s.sample_out, s.sample_stride = samp.data_ptr(), n_s * k
    if sums:
        su, su2 = c.inout(sum0[0]), c.inout(sum0[1])
        s.sum_u, s.sum_u2 = su.data_ptr(), su2.data_ptr()
    if run is None:
        c.call = lambda h: _ipmc("ipmc_pcn_sweep", C.byref(m), C.byref(s), h)
    else:
        s.sample_every, s.sample_step_stride = run, k
        c.call = lambda h: _ipmc("ipmc_pcn_run", C.byref(m), C.byref(s), 3, 2, (1 if run == 0 else 2) * k, h)
    c.keep += [m, s]

    def twin():
        U, ph, a, cl = U0.copy(), phi0.copy(), acc0.copy(), calls0.copy()
        sm = None if sum0 is None else (sum0[0].copy(), sum0[1].copy())
        if total == 0:  # the copy-only path: nothing moves, sample_out receives u
            return [U, ph, a, cl, U.reshape(n, 1, k)]
        smp = np.empty((n, n_s, k), dtype=npd)
        orc.pcn_sweep(op, U, ph, y, ginv, sq, 0.3, 1234, 10, total, accepts=a, calls=cl, chain_offset=2,
                      beta_schedule=sch, sums=sm, n_threads=8, samples=smp,
                      sample_every=0 if run is None else (2 if run == 0 else 1))
        return [U, ph, a, cl, smp] + ([] if sm is None else list(sm))

    c.twin = twin
    return c


def _d2h_case(dev):
    c = _Case(dev)
    rows, width, sp, dp = 10, 9, 12, 16  # 9 doubles of every row; pitches of 12 and 16 doubles
    a = np.random.default_rng(2).normal(size=(rows, sp))
    src = c.inp(a)
    dst = torch.empty((rows, dp), dtype=torch.float64, pin_memory=True)
    c.host.append(dst)
    c.call = lambda h: _ipmc("ipmc_copy_rows_d2h", dst.data_ptr(), dp * 8, src.data_ptr(), sp * 8, width * 8, rows, h)

    def twin():
        want = _nan((rows, dp), np.float64)
        want[:, :width] = a[:, :width]
        return [want]

    c.twin = twin
    return c


def _autocorr_case(dev, dtype, length):
    c = _Case(dev)
    x = np.cumsum(np.random.default_rng(length).normal(size=(3, length)), axis=1).astype(_npd(dtype))
    xt = c.inp(x)
    out = c.out((3, 50), torch.float64)
    c.call = lambda h: _ipmc("ipmc_autocorr", xt.data_ptr(), _abi_dtype(dtype), 3, length, length, 1, 50,
                             out.data_ptr(), h)
    return c


def _burn_in_case(dev, dtype):
    c = _Case(dev)
    rng = np.random.default_rng(8)
    t = np.arange(300)
    x = (3.0 * np.exp(-t / rng.uniform(5, 60, size=(8, 3, 1))) + 1.0 + 0.01 * rng.normal(size=(8, 3, 300)))
    xt = c.inp(x.astype(_npd(dtype)))
    flags = c.scratch((8 * ((300 + 31) // 32),), torch.int32)
    out = c.out((8,), torch.int64)
    c.call = lambda h: _ipmc("ipmc_burn_in", xt.data_ptr(), _abi_dtype(dtype), 8, 3, 300, 900, 300, 1, 50, 0.03,
                             flags.data_ptr(), out.data_ptr(), h)
    return c


ROWS = np.random.default_rng(13).normal(size=(2500, 7))


def _ordered_sum_case(dev):
    from ip_mcmc_amd import _hostlib

    c = _Case(dev)
    acc0 = np.arange(7, dtype=np.float64)
    rows, acc = c.inp(ROWS), c.inout(acc0)
    c.call = lambda h: _ipmc("ipmc_ordered_sum", rows.data_ptr(), 2500, 7, 7, 3.0, acc.data_ptr(), h)
    c.twin = lambda: [_hostlib.ordered_sum(ROWS, acc0.copy(), 3.0)]
    return c


def _block_sums_case(dev):
    from ip_mcmc_amd import _hostlib

    c = _Case(dev)
    rows = c.inp(ROWS)
    out = c.out((3, 7), torch.float64)
    c.call = lambda h: _ipmc("ipmc_block_sums", rows.data_ptr(), 2500, 7, 7, 1024, 3.0, out.data_ptr(), h)
    c.twin = lambda: [np.stack([_hostlib.ordered_sum(ROWS[b:b + 1024], np.zeros(7), 3.0)
                                for b in range(0, 2500, 1024)])]
    return c


def _centered_case(dev):
    c = _Case(dev)
    rows, cen = c.inp(ROWS), c.inp(ROWS.mean(axis=0))
    out = c.out((3, 7), torch.float64)
    c.call = lambda h: _ipmc("ipmc_centered_sq_block_sums", rows.data_ptr(), 2500, 7, 7, cen.data_ptr(), 1024,
                             out.data_ptr(), h)
    return c


def _samples(shape, dtype, seed=0):
    """(C, n, k) samples with a drift per chain, as numpy of the dtype."""
    rng = np.random.default_rng(seed + shape[1])
    return (rng.normal(size=shape) + rng.normal(size=(shape[0], 1, shape[2]))).astype(_npd(dtype))


def _geom(t, dtype, layout="time_vars"):
    """ipmc_split_stats' geometry of a contiguous 3-D tensor: (C, n, k) or, vars_time, (C, k, n)."""
    C_, a, b = t.shape
    if layout == "time_vars":
        return (t.data_ptr(), _abi_dtype(dtype), C_, a, b, a * b, b, 1)
    return (t.data_ptr(), _abi_dtype(dtype), C_, b, a, a * b, 1, b)


def _split_stats_case(dev, dtype, shape):
    c = _Case(dev)
    x = c.inp(_samples(shape, dtype))
    mean, var = c.out((2 * shape[0], shape[2]), torch.float64), c.out((2 * shape[0], shape[2]), torch.float64)
    c.call = lambda h: _ipmc("ipmc_split_stats", *_geom(x, dtype), mean.data_ptr(), var.data_ptr(), h)
    return c


def _split_means(a):
    C_, n, k = a.shape
    N = n // 2
    a = a.astype(np.float64)
    return np.concatenate([a[:, :N].mean(axis=1), a[:, N:2 * N].mean(axis=1)], axis=0)


def _mean_acov_case(dev, dtype, shape):
    c = _Case(dev)
    a = _samples(shape, dtype)
    x, mean = c.inp(a), c.inp(_split_means(a))
    out = c.out((1, 41, shape[2]), torch.float64)
    c.call = lambda h: _ipmc("ipmc_mean_acov", *_geom(x, dtype), mean.data_ptr(), 40, 1024, out.data_ptr(), h)
    return c


def _moments_case(dev):
    c = _Case(dev)
    rng = np.random.default_rng(4)
    a = rng.normal(size=(100, 300, 5)) + 2.0
    su, su2 = c.inp(a.sum(axis=0)), c.inp((a * a).sum(axis=0))
    mean, var = c.out((300, 5), torch.float64), c.out((300, 5), torch.float64)
    c.call = lambda h: _ipmc("ipmc_moments_stats", su.data_ptr(), su2.data_ptr(), 300, 5, 100, mean.data_ptr(),
                             var.data_ptr(), h)
    return c


def _minmax_case(dev, dtype, layout):
    c = _Case(dev)
    a = _samples((5, 33, 3), dtype)
    x = c.inp(a if layout == "time_vars" else np.ascontiguousarray(a.transpose(0, 2, 1)))
    lo, hi = c.out((3,), torch.float64), c.out((3,), torch.float64)
    scratch = c.scratch((2 * 1024 * 3,), torch.float64)
    c.call = lambda h: _ipmc("ipmc_minmax", *_geom(x, dtype, layout), lo.data_ptr(), hi.data_ptr(),
                             scratch.data_ptr(), h)
    af = a.astype(np.float64).reshape(-1, 3)
    c.twin = lambda: [af.min(axis=0), af.max(axis=0)]
    return c


def _hist1d_case(dev, dtype):
    from ip_mcmc_amd import marginal_histograms

    c = _Case(dev)
    a = _samples((5, 333, 3), dtype)
    want = marginal_histograms(a, bins=20, range=(-1.5, 1.0), backend="host")
    x, e = c.inp(a), c.inp(want["edges"])
    counts, below, above = c.out((3, 20), torch.int64), c.out((3,), torch.int64), c.out((3,), torch.int64)
    c.call = lambda h: _ipmc("ipmc_hist1d", *_geom(x, dtype), 20, e.data_ptr(), counts.data_ptr(), below.data_ptr(),
                             above.data_ptr(), h)
    c.twin = lambda: [want["counts"], want["below"], want["above"]]
    return c


def _histdd_case(dev, dtype, bins):
    from ip_mcmc_amd import histogramdd

    c = _Case(dev)
    a = _samples((5, 333, 4), dtype)
    comp = (3, 0, 2)
    want, edges = histogramdd(a, bins=bins, range=[(-1.5, 1.0)] * 3, components=comp, backend="host")
    x, e = c.inp(a), c.inp(np.concatenate(edges))
    counts = c.out((bins**3,), torch.int64)
    c_comp, c_bins = (C.c_int32 * 3)(*comp), (C.c_int32 * 3)(bins, bins, bins)
    c.keep += [c_comp, c_bins]
    c.call = lambda h: _ipmc("ipmc_histdd", *_geom(x, dtype), 3, C.addressof(c_comp), C.addressof(c_bins),
                             e.data_ptr(), counts.data_ptr(), h)
    c.twin = lambda: [want.reshape(-1)]
    return c


def _scatter_case(dev, dtype, shape, split):
    c = _Case(dev)
    a = _samples(shape, dtype)
    C_, n, k = shape
    x = c.inp(a)
    cen = c.inp(_split_means(a) if split else a.astype(np.float64).reshape(-1, k).mean(axis=0))
    nb = -(-C_ // 2)
    part = c.out((nb, k, k), torch.float64)
    dsum = c.out((nb, k), torch.float64) if split else None
    c.call = lambda h: _ipmc("ipmc_scatter", *_geom(x, dtype), cen.data_ptr(), 1 if split else 0, 2, part.data_ptr(),
                             None if dsum is None else dsum.data_ptr(), h)
    return c


def _sort_case(dev, dtype, fold=False):
    c = _Case(dev)
    S_ = _abi().SORT_TILE + 1
    a = _samples((1, S_, 3), dtype)
    x = c.inp(a)
    cen = c.inp(a.astype(np.float64).reshape(-1, 3).mean(axis=0)) if fold else None
    need = C.c_int64(0)
    _ipmc("ipmc_sort_workspace", 1, S_, 3, _abi_dtype(dtype), C.byref(need))
    ws = c.scratch((max(need.value, 8),), torch.uint8)
    srt, perm = c.out((3, S_), torch.float64), c.out((3, S_), torch.int32)
    c.call = lambda h: _ipmc("ipmc_pooled_sort", *_geom(x, dtype), None if cen is None else cen.data_ptr(),
                             srt.data_ptr(), perm.data_ptr(), ws.data_ptr(), need.value, h)
    return c


def _rank_scores_case(dev, mode):
    c = _Case(dev)
    C_, n, k = 3, 70, 2
    a = np.round(_samples((C_, n, k), torch.float64), 1)  # ties
    col = a.reshape(-1, k).T
    perm = np.argsort(col, axis=1, kind="stable")
    srt, pm = c.inp(np.take_along_axis(col, perm, axis=1)), c.inp(perm.astype(np.int32))
    out = c.out((C_, n, k), torch.float64)
    c.call = lambda h: _ipmc("ipmc_rank_scores", srt.data_ptr(), pm.data_ptr(), k, C_, n, mode, out.data_ptr(),
                             n * k, k, 1, None, 0, h)
    return c


def _phi_smc(dtype, n=1025):
    a = 1.0 + 10.0 * np.random.default_rng(1000 + n).random(n) ** 2
    a[3], a[1024] = np.inf, np.nan
    a = a.astype(_npd(dtype))
    return a, float(a[np.isfinite(a)].astype(np.float64).min())


def _smc_ws(c, n, nd):
    need = C.c_int64(0)
    _ipmc("ipmc_smc_workspace", n, nd, C.byref(need))
    return c.scratch((max(need.value, 8),), torch.uint8), need.value


def _temper_sums_case(dev, dtype):
    from ip_mcmc_amd import _hostlib

    c = _Case(dev)
    a, ref = _phi_smc(dtype)
    deltas = np.ascontiguousarray(np.concatenate([[0.0], np.geomspace(1e-4, 1.0, 14)]))
    phi = c.inp(a)
    ws, nbytes = _smc_ws(c, 1025, 15)
    s1, s2 = c.out((15,), torch.float64), c.out((15,), torch.float64)
    c.keep.append(deltas)
    c.call = lambda h: _ipmc("ipmc_temper_sums", phi.data_ptr(), _abi_dtype(dtype), 1025, ref, deltas.ctypes.data, 15,
                             s1.data_ptr(), s2.data_ptr(), ws.data_ptr(), nbytes, h)
    c.twin = lambda: list(_hostlib.temper_sums(a, ref, deltas))
    return c


def _cumweights_case(dev, dtype):
    from ip_mcmc_amd import _hostlib

    c = _Case(dev)
    a, ref = _phi_smc(dtype)
    phi = c.inp(a)
    ws, nbytes = _smc_ws(c, 1025, 1)
    cum = c.out((1025,), torch.float64)
    c.call = lambda h: _ipmc("ipmc_temper_cumweights", phi.data_ptr(), _abi_dtype(dtype), 1025, ref, 0.37,
                             cum.data_ptr(), ws.data_ptr(), nbytes, h)
    c.twin = lambda: [_hostlib.temper_cumweights(a, ref, 0.37)]
    return c


def _ancestors_case(dev):
    from ip_mcmc_amd import _hostlib

    c = _Case(dev)
    a, ref = _phi_smc(torch.float64)
    cum_np = _hostlib.temper_cumweights(a, ref, 0.37)
    cum = c.inp(cum_np)
    anc = c.out((2049,), torch.int64)
    c.call = lambda h: _ipmc("ipmc_systematic_ancestors", cum.data_ptr(), 1025, 0.5, 2049, anc.data_ptr(), h)
    c.twin = lambda: [_hostlib.systematic_ancestors(cum_np, 0.5, 2049)]
    return c


def _gather_case(dev, dtype):
    c = _Case(dev)
    npd, k, n_src, n_out, ss, ds = _npd(dtype), 3, 3001, 65, 6, 5
    a = np.random.default_rng(3).standard_normal((n_src, ss)).astype(npd)
    idx_np = np.sort(np.random.default_rng(4).integers(0, n_src, n_out)).astype(np.int64)
    src, idx = c.inp(a), c.inp(idx_np)
    dst = c.out((n_out, ds), dtype)
    c.call = lambda h: _ipmc("ipmc_gather_rows", src.data_ptr(), _abi_dtype(dtype), n_src, k, ss, idx.data_ptr(),
                             n_out, dst.data_ptr(), ds, h)

    def twin():
        want = _nan((n_out, ds), npd)  # the padding keeps the poison
        want[:, :k] = a[idx_np, :k]
        return [want]

    c.twin = twin
    return c


# ----------------------------------------------------------- negative control
def test_negative_control_a_launch_on_the_null_stream_is_seen(dev, cal):
    """ipmc_block_sums through the harness with stream handle 0: the launch runs ahead of the copy of its
    input (a read of poison, all memory valid) and its output is poisoned after it, so the snapshot has to
    differ from the twin.  If it did not, no case below would prove anything."""
    c = _block_sums_case(dev)
    want = [_bits(x) for x in c.twin()]
    assert _same(_serial(c), want)
    got = _behind(cal, [(cal.S, [c])], handle=0)[id(c)]
    assert not _same(got, want), "a launch on the null stream went unnoticed"
    torch.cuda.synchronize()
    _check(cal, c)  # and the same case on the stream itself passes


# ---------------------------------------------------------------- C-ABI tier
@pytest.mark.parametrize("dtype", DTYPES)
def test_draws(dev, cal, orc, dtype):
    _check(cal, _normal_case(dev, orc, dtype))
    _check(cal, _uniform_case(dev, orc))
    for chol in (False, True):
        _check(cal, _draws_case(dev, dtype, chol))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", OPS)
def test_forward_and_potential(dev, cal, orc, name, dtype):
    _check(cal, _forward_case(dev, orc, name, dtype))
    _check(cal, _potential_case(dev, orc, name, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_init_phi_with_regularizer(dev, cal, orc, dtype):
    _check(cal, _init_phi_case(dev, orc, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("spec", [1, 2])
@pytest.mark.parametrize("name", FAMILIES)
def test_sweep(dev, cal, orc, name, spec, dtype):
    _check(cal, _sweep_case(dev, orc, name, dtype, spec=spec))


def test_sweep_packed_f32_lorenz96(dev, cal, orc):
    _check(cal, _sweep_case(dev, orc, "l96_8", torch.float32, lanes=2, cpl=2, sums=True))


@pytest.mark.parametrize("dtype", DTYPES)
def test_sweep_sums_samples_schedule(dev, cal, orc, dtype):
    _check(cal, _sweep_case(dev, orc, "l96_40", dtype, sums=True, sched=True))
    _check(cal, _sweep_case(dev, orc, "lin", dtype, spec=2, sums=True, sched=True))


@pytest.mark.parametrize("dtype", DTYPES)
def test_sweep_zero_steps_copies_the_state(dev, cal, orc, dtype):
    _check(cal, _sweep_case(dev, orc, "l96_8", dtype, n_steps=0))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sample_every", [0, 1])
def test_pcn_run(dev, cal, orc, sample_every, dtype):
    _check(cal, _sweep_case(dev, orc, "l96_8", dtype, run=sample_every, sums=True, sched=True))


def test_copy_rows_d2h(dev, cal):
    _check(cal, _d2h_case(dev))


@pytest.mark.parametrize("dtype", DTYPES)
def test_autocorr_and_burn_in(dev, cal, dtype):
    for length in (500, 9001):
        _check(cal, _autocorr_case(dev, dtype, length))
    _check(cal, _burn_in_case(dev, dtype))


def test_row_sums(dev, cal):
    _check(cal, _ordered_sum_case(dev))
    _check(cal, _block_sums_case(dev))
    _check(cal, _centered_case(dev))
    _check(cal, _moments_case(dev))


@pytest.mark.parametrize("dtype", DTYPES)
def test_split_stats_and_mean_acov(dev, cal, dtype):
    for shape in ((3, 64, 40), (2, 200, 2)):
        _check(cal, _split_stats_case(dev, dtype, shape))
    for shape in ((3, 128, 2), (3, 130, 2), (1, 16386, 1)):  # N = 64, 65 and 8193
        _check(cal, _mean_acov_case(dev, dtype, shape))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ["time_vars", "vars_time"])
def test_minmax(dev, cal, layout, dtype):
    _check(cal, _minmax_case(dev, dtype, layout))


@pytest.mark.parametrize("dtype", DTYPES)
def test_hist1d(dev, cal, dtype):
    _check(cal, _hist1d_case(dev, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bins", [20, 21])  # 8000 cells in LDS, 9261 in global memory
def test_histdd(dev, cal, bins, dtype):
    _check(cal, _histdd_case(dev, dtype, bins))


@pytest.mark.parametrize("dtype", DTYPES)
def test_scatter(dev, cal, dtype):
    _check(cal, _scatter_case(dev, dtype, (3, 64, 40), True))
    _check(cal, _scatter_case(dev, dtype, (4, 40, 130), False))


@pytest.mark.parametrize("dtype", DTYPES)
def test_pooled_sort(dev, cal, dtype):
    _check(cal, _sort_case(dev, dtype))
    _check(cal, _sort_case(dev, dtype, fold=True))


@pytest.mark.parametrize("mode", [0, 1])
def test_rank_scores(dev, cal, mode):
    _check(cal, _rank_scores_case(dev, mode))


@pytest.mark.parametrize("dtype", DTYPES)
def test_temper_sums(dev, cal, dtype):
    _check(cal, _temper_sums_case(dev, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_temper_cumweights(dev, cal, dtype):
    _check(cal, _cumweights_case(dev, dtype))


def test_systematic_ancestors(dev, cal):
    _check(cal, _ancestors_case(dev))


@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_rows(dev, cal, dtype):
    _check(cal, _gather_case(dev, dtype))


# --------------------------------------------------------------- Python tier
def _py_case(dev, fn, inputs, twin=None, host_values=False):
    """fn(*device tensors written on the stream) under `with torch.cuda.stream(S)`."""
    c = _Case(dev)
    bufs = [c.inp(a) for a in inputs]
    c.call = lambda h: fn(h, *bufs)
    c.returns, c.host_values, c.twin = True, host_values, twin
    return c


def test_python_draws_and_block_sums(dev, cal, orc):
    from ip_mcmc_amd import device as D

    step = (1 << 33) + 7
    _check(cal, _py_case(dev, lambda h: D.normals(99, 5, 300, step, 7, torch.float32, dev), [],
                         lambda: [orc.normals(99, 5, 300, step, 7).astype(np.float32)]), in_ctx=True)
    _check(cal, _py_case(dev, lambda h: D.uniforms(99, 5, 300, step, dev), [],
                         lambda: [orc.uniforms(99, 5, 300, step)]), in_ctx=True)
    _check(cal, _py_case(dev, lambda h, rows: D.block_sums(rows, 1024, 3.0), [ROWS], _block_sums_case(dev).twin),
           in_ctx=True)


@pytest.mark.parametrize("explicit", [False, True])
def test_torch_ops(dev, cal, orc, explicit):
    """torch.ops.ipmc through stream=None inside the stream's context, and with stream=S.cuda_stream from
    the default-stream context."""
    from ip_mcmc_amd import torch_ops

    torch_ops.load()
    op = _op("l96_8")
    st = (lambda h: h) if explicit else (lambda h: None)
    for dtype in DTYPES:
        npd = _npd(dtype)
        U, y, ginv = _eval_problem(orc, op, dtype)
        op.model(dtype, dev)
        _check(cal, _py_case(dev, lambda h, u: torch_ops.forward(op, u, stream=st(h)), [U],
                             lambda: [orc.forward(op, U, npd)]), in_ctx=not explicit)
        _check(cal, _py_case(dev, lambda h, u, yt, gt: torch_ops.potential(op, u, yt, gt, stream=st(h)),
                             [U, y, ginv], lambda: [orc.potential(op, U, y, ginv, npd)]), in_ctx=not explicit)
        sq = np.linspace(0.5, 1.5, op.k).astype(npd)
        phi0 = orc.potential(op, U, y, ginv * npd(0.3), npd)
        acc0 = np.arange(U.shape[0], dtype=np.int64)
        c = _Case(dev)
        u, phi, acc = c.inout(U), c.inout(phi0), c.inout(acc0)
        yt, gt, sqt = c.inp(y), c.inp(ginv * npd(0.3)), c.inp(sq)
        c.call = lambda h: torch_ops.pcn_sweep(op, u, phi, acc, yt, gt, sqt, 0.3, 5, 7, 3, stream=st(h))

        def twin():
            Uo, po, ao = U.copy(), phi0.copy(), acc0.copy()
            orc.pcn_sweep(op, Uo, po, y, ginv * npd(0.3), sq, 0.3, 5, 7, 3, accepts=ao, n_threads=8)
            return [Uo, po, ao]

        c.twin = twin
        _check(cal, c, in_ctx=not explicit)


def test_python_posterior(dev, cal):
    from ip_mcmc_amd import histogramdd, marginal_histograms, support

    a = _samples((5, 333, 3), torch.float64)
    _check(cal, _py_case(dev, lambda h, x: support(x), [a], lambda: _flatten(support(a, backend="host")),
                         host_values=True), in_ctx=True)
    _check(cal, _py_case(dev, lambda h, x: marginal_histograms(x, bins=20), [a],
                         lambda: _flatten(marginal_histograms(a, bins=20, backend="host")), host_values=True),
           in_ctx=True)
    _check(cal, _py_case(dev, lambda h, x: histogramdd(x, bins=7), [a],
                         lambda: _flatten(histogramdd(a, bins=7, backend="host")), host_values=True), in_ctx=True)


def test_python_convergence_and_covariance(dev, cal):
    from ip_mcmc_amd import convergence, posterior_covariance, rank_convergence

    a = np.random.default_rng(9).normal(size=(6, 200, 3))  # independent draws: the pair sums end early
    for fn in (convergence, rank_convergence, posterior_covariance):
        _check(cal, _py_case(dev, lambda h, x, fn=fn: fn(x), [a], host_values=True), in_ctx=True)


def test_python_autocorr_and_burn_in(dev, cal):
    from ip_mcmc_amd.diagnostics import autocorr, burn_in_lengths

    x = np.cumsum(np.random.default_rng(1).normal(size=(3, 500)), axis=1)
    _check(cal, _py_case(dev, lambda h, t: autocorr(t, 50), [x]), in_ctx=True)
    t = np.arange(300)
    b = 3.0 * np.exp(-t / np.array([5.0, 20.0, 60.0]).reshape(1, 3, 1)) + 1.0 + np.zeros((4, 1, 1))
    b = b + 0.01 * np.random.default_rng(2).normal(size=b.shape)
    _check(cal, _py_case(dev, lambda h, t_: burn_in_lengths(t_), [b]), in_ctx=True)


def test_python_smc_pieces(dev, cal):
    from ip_mcmc_amd import systematic_resample, tempering_sums

    a, ref = _phi_smc(torch.float64)
    deltas = np.linspace(0.0, 1.0, 15)
    _check(cal, _py_case(dev, lambda h, p: tempering_sums(p, None, deltas), [a],
                         lambda: _flatten(tempering_sums(a, None, deltas, backend="host")), host_values=True),
           in_ctx=True)
    _check(cal, _py_case(dev, lambda h, p: systematic_resample(p, ref, 0.37, 0.5, n_out=2049), [a],
                         lambda: [systematic_resample(a, ref, 0.37, 0.5, n_out=2049, backend="host")]),
           in_ctx=True)


def _linear_sampler(dtype):
    """The 4-parameter linear problem of tests/test_gpu_sampler_edges.py."""
    from ip_mcmc_amd import (ConstSteppCNProposer, CountedAccepter, EvolutionPotential, GaussianDistribution,
                             LinearOperator, MCMCSampler, pCNAccepter)

    g = np.array([3.0, 1.0, 4.0, 1.0])
    pot = EvolutionPotential(LinearOperator(g), np.array([30.0]), GaussianDistribution(0, 0.25))
    acc = CountedAccepter(pCNAccepter(pot))
    return MCMCSampler(ConstSteppCNProposer(0.5, GaussianDistribution(np.zeros(4), np.eye(4))), acc, 3,
                       dtype=dtype), acc


@pytest.mark.parametrize("case", ["samples", "moments_device", "sample_file", "overlapped_f32"])
def test_sampler_run(dev, cal, case, tmp_path, monkeypatch):
    """MCMCSampler.run inside the stream's context, u_0 a device tensor written behind the busy work: the
    same run on the default stream (the copy streams of the sample file and of the overlapped copy order
    themselves against the stream the sweeps are on)."""
    from ip_mcmc_amd import sampler as S_

    dtype = np.float32 if case == "overlapped_f32" else np.float64
    if case == "overlapped_f32":
        monkeypatch.setattr(S_, "OVERLAP_COPY_MIN_BYTES", 0)
    u0 = 0.1 * np.random.default_rng(6).normal(size=(7, 4))
    n_file = [0]

    def run(h, u):
        s, acc = _linear_sampler(dtype)
        kw = dict(n_samples=10, burn_in=4, sample_interval=2)
        if case == "moments_device":
            kw.update(keep="moments", results="device")
        if case == "sample_file":
            n_file[0] += 1
            kw.update(sample_file=str(tmp_path / f"s{n_file[0]}.npy"), flush_every=3)
        out = s.run(u, **kw)
        if case == "overlapped_f32":
            assert s.last_run_timing["copy_overlapped"]
        if case == "sample_file":
            out = np.array(out)
        return [out, np.asarray(acc.accepts), np.asarray(acc.calls), s.state.phi, s.state.accepts]

    _check(cal, _py_case(dev, run, [u0], host_values=True), in_ctx=True)


def test_tempered_smc_run(dev, cal):
    from ip_mcmc_amd import EvolutionPotential, GaussianDistribution, LinearOperator, TemperedSMC

    def run(h):
        prior = GaussianDistribution(np.zeros(4), np.eye(4))
        pot = EvolutionPotential(LinearOperator(np.array([3.0, 1.0, 4.0, 1.0])), np.array([30.0]),
                                 GaussianDistribution(np.zeros(1), 0.25 * np.eye(1)))
        r = TemperedSMC(prior, pot, beta=0.25, rng=11).run(n_particles=1500, steps_per_stage=3, results="device")
        assert r.last_path == "device" and r.particles.is_cuda and r.n_stages >= 2
        return r

    _check(cal, _py_case(dev, run, [], host_values=True), in_ctx=True)


# ------------------------------------------------------- two streams at once
def test_two_streams_interleaved(dev, cal, orc):
    """A Lorenz-96 sweep and ipmc_pooled_sort on one stream, ipmc_hist1d and ipmc_temper_cumweights on
    another, each stream behind its own busy work, the calls interleaved from the host, every call on its
    own buffers: all four equal their serial results (the library keeps no device state between calls)."""
    a = [_sweep_case(dev, orc, "l96_40", torch.float64, sums=True), _sort_case(dev, torch.float64)]
    b = [_hist1d_case(dev, torch.float64), _cumweights_case(dev, torch.float64)]
    serial = {id(c): _serial(c) for c in a + b}
    got = _behind(cal, [(cal.S, a), (cal.S2, b)])
    for c in a + b:
        assert _same(got[id(c)], serial[id(c)]), (a + b).index(c)
        if c.twin is not None:
            assert _same(got[id(c)], [_bits(x) for x in c.twin()]), (a + b).index(c)
