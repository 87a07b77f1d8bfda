"""ipmc_scatter through covariance.posterior_covariance / multivariate_rhat on
the device against the host definition (backend="host", numpy float64), on
the shapes of tests/test_covariance_cpu.py:

  k = 1 and k = 3            a single partial tile
  k = 17                     tile remainder
  k = 40                     the headline
  k = 256 with 2 chains      every tile pair, mirrored
  (70, 8, 5), 16 per block   a short last block
  (1, 2, 1)                  the minimum

The device differs from the host in the order of the adds alone: covariances
agree within 1e-10 sqrt(diag_i diag_j) (the device-against-host tolerance of
tests/test_gpu_convergence.py), means within 1e-13 |mean|."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from ip_mcmc_amd import _abi, multivariate_rhat, posterior_covariance
from ip_mcmc_amd._lib import call
from ip_mcmc_amd.posterior import _geom
from test_covariance_cpu import IDS, SHAPES, assert_cov_close, make_samples

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def on_gpu(x):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0")


def assert_same_cov(dev, host):
    assert_cov_close(dev["cov"], host["cov"], 1e-10)
    assert np.all(np.abs(dev["mean"] - host["mean"]) <= 1e-13 * np.abs(host["mean"]))
    assert np.array_equal(dev["cov"], dev["cov"].T)
    assert dev["n"] == host["n"]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("layout", ["time_vars", "vars_time"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_device_equals_host_definition(shape, layout, dtype):
    C, n, k, block = shape
    x = make_samples(C, n, k, seed=k + n, dtype=dtype, layout=layout)
    host = posterior_covariance(x, layout=layout, backend="host", block_chains=block)
    dev = posterior_covariance(on_gpu(x), layout=layout, backend="device", block_chains=block)
    print("cov", np.abs((dev["cov"] - host["cov"]) / np.sqrt(np.outer(np.diag(host["cov"]), np.diag(host["cov"])))).max(),
          "mean", np.abs((dev["mean"] - host["mean"]) / host["mean"]).max())
    assert_same_cov(dev, host)
    assert np.all(np.abs(dev["corr"] - host["corr"]) <= 1e-9)
    assert np.array_equal(np.diag(dev["corr"]), np.ones(k))
    if n < 4:
        return
    hr = multivariate_rhat(x, layout=layout, backend="host", block_chains=block)
    dr = multivariate_rhat(on_gpu(x), layout=layout, backend="device", block_chains=block)
    for key in ("W", "Bn"):
        scale = np.sqrt(np.outer(np.diag(hr[key]), np.diag(hr[key])))
        print(key, (np.abs(dr[key] - hr[key]) / scale).max())
        assert_cov_close(dr[key], hr[key], 1e-10)
        assert np.array_equal(dr[key], dr[key].T)
    assert np.all(np.abs(dr["rhat"] - hr["rhat"]) <= 1e-9)


@pytest.mark.parametrize("shape", [(5, 13, 3, None), (70, 8, 5, 16), (40, 24, 17, None), (32, 40, 40, 5), (6, 9, 1, None)],
                         ids=["5-13-3", "70-8-5", "40-24-17", "32-40-40", "6-9-1"])
def test_rhat_mv_equals_host_on_well_conditioned_w(shape):
    """λ_max moves by about cond(W) times the relative change of W and Bn (2e-10): inputs with
    cond(W) < 100 give 1e-7 relative with room to spare."""
    C, n, k, block = shape
    x = make_samples(C, n, k, seed=3 * k + C, sd_lo=1.0)
    hr = multivariate_rhat(x, backend="host", block_chains=block)
    assert np.linalg.cond(hr["W"]) < 100
    dr = multivariate_rhat(on_gpu(x), backend="device", block_chains=block)
    print("rhat_mv", dr["rhat_mv"], hr["rhat_mv"])
    assert abs(dr["rhat_mv"] - hr["rhat_mv"]) <= 1e-7 * hr["rhat_mv"]
    assert abs(dr["lambda_max"] - hr["lambda_max"]) <= 1e-7 * hr["rhat_mv"] ** 2
    assert dr["rhat_mv"] >= dr["rhat"].max() - 1e-12


@pytest.mark.parametrize("layout", ["time_vars", "vars_time"])
def test_strided_views_are_processed_in_place(layout):
    """A burn-in slice x[:, 3:, :] and a transposed view go to the kernels by their strides."""
    x = make_samples(9, 15, 17, seed=21, layout=layout)
    t = on_gpu(x)
    tv, xv = (t[:, 3:], x[:, 3:]) if layout == "time_vars" else (t[:, :, 3:], x[:, :, 3:])
    assert not tv.is_contiguous()
    ptr = tv.data_ptr()
    assert_same_cov(posterior_covariance(tv, layout=layout, backend="device"),
                    posterior_covariance(xv, layout=layout, backend="host"))
    hr = multivariate_rhat(xv, layout=layout, backend="host")
    dr = multivariate_rhat(tv, layout=layout, backend="device")
    assert_cov_close(dr["W"], hr["W"], 1e-10)
    assert_cov_close(dr["Bn"], hr["Bn"], 1e-10)
    # the same memory read through the other layout's transposed view
    other = "vars_time" if layout == "time_vars" else "time_vars"
    tt, xt = tv.transpose(1, 2), xv.transpose(0, 2, 1)
    assert not tt.is_contiguous() and tt.data_ptr() == ptr
    assert_same_cov(posterior_covariance(tt, layout=other, backend="device"),
                    posterior_covariance(xt, layout=other, backend="host"))
    assert tv.data_ptr() == ptr and tt.data_ptr() == ptr and tv.data_ptr() == t.data_ptr() + 3 * t.element_size() * (
        17 if layout == "time_vars" else 1)


def test_two_calls_give_the_same_bits():
    x = on_gpu(make_samples(300, 12, 40, seed=22))
    a, b = posterior_covariance(x, backend="device"), posterior_covariance(x, backend="device")
    for key in ("mean", "cov", "corr"):
        assert np.array_equal(a[key], b[key])
    assert np.array_equal(a["cov"], a["cov"].T)
    ra, rb = multivariate_rhat(x, backend="device"), multivariate_rhat(x, backend="device")
    for key in ("W", "Bn", "rhat"):
        assert np.array_equal(ra[key], rb[key])
    assert ra["rhat_mv"] == rb["rhat_mv"]


@pytest.mark.parametrize("layout", ["time_vars", "vars_time"])
def test_chunked_host_input_gives_the_bits_of_one_chunk(layout):
    x = make_samples(70, 8, 5, seed=23, layout=layout)
    per_block = 16 * 8 * 5 * 8
    one = posterior_covariance(x, layout=layout, backend="device", block_chains=16)
    three = posterior_covariance(x, layout=layout, backend="device", block_chains=16, chunk_bytes=2 * per_block)
    for key in ("mean", "cov", "corr"):
        assert np.array_equal(one[key], three[key])
    r1 = multivariate_rhat(x, layout=layout, backend="device", block_chains=16)
    r3 = multivariate_rhat(x, layout=layout, backend="device", block_chains=16, chunk_bytes=2 * per_block)
    for key in ("W", "Bn", "rhat"):
        assert np.array_equal(r1[key], r3[key])
    assert_same_cov(one, posterior_covariance(x, layout=layout, backend="host", block_chains=16))


def _scatter(t, center, mode, block, with_dsum=True, layout="time_vars"):
    """ipmc_scatter on a 3-D device tensor, (C, n, k) or (C, k, n) with layout="vars_time", f64 or
    f32, contiguous or a view: it goes to the kernel by the geometry covariance.py passes
    (posterior._geom), never copied.  Returns (scatter [nb, k, k], dsum [nb, k] or None); both
    are NaN where the kernel wrote nothing."""
    geom = _geom(t, layout)
    C, k = geom[2], geom[4]
    nb = -(-C // block)
    out = torch.full((nb, k, k), np.nan, dtype=torch.float64, device=t.device)
    ds = torch.full((nb, k), np.nan, dtype=torch.float64, device=t.device) if with_dsum else None
    call("ipmc_scatter", *geom, center.data_ptr(), mode, block, out.data_ptr(), None if ds is None else ds.data_ptr(),
         torch.cuda.current_stream(t.device).cuda_stream)
    return out.cpu().numpy(), None if ds is None else ds.cpu().numpy()


@pytest.mark.parametrize("shape", [(5, 37, 40, 2), (3, 21, 256, 2), (4, 1100, 3, 4)], ids=["k40", "k256", "k3"])
def test_integer_samples_give_numpys_integers(shape):
    """Small integers with an asymmetric pattern: every product and sum is exact in f64 (at most
    4 400 rows of |d| <= 13), so any order of the adds gives numpy's integers, and a
    misplaced tile, thread tile or mirror shows as a wrong entry."""
    C, n, k, block = shape
    rng = np.random.default_rng(k)
    x = rng.integers(-5, 6, size=(C, n, k)).astype(np.float64)
    x += (np.arange(k) % 7)[None, None, :]  # means that differ between components: an asymmetric pattern
    t = on_gpu(x)
    center = np.arange(k, dtype=np.float64) % 3
    got, ds = _scatter(t, on_gpu(center), _abi.CENTER_SHARED, block)
    for b in range(got.shape[0]):
        d = (x[b * block:(b + 1) * block] - center).reshape(-1, k)
        assert np.array_equal(got[b], d.T @ d), b
        assert np.array_equal(ds[b], d.sum(axis=0)), b
    # split centres: integers per split chain
    mu = rng.integers(-2, 3, size=(2 * C, k)).astype(np.float64)
    got, _ = _scatter(t, on_gpu(mu), _abi.CENTER_SPLIT, block, with_dsum=False)
    N = n // 2
    for b in range(got.shape[0]):
        c0, c1 = b * block, min(C, (b + 1) * block)
        d = np.concatenate([x[c0:c1, :N] - mu[c0:c1, None], x[c0:c1, N:2 * N] - mu[C + c0:C + c1, None]],
                           axis=1).reshape(-1, k)
        assert np.array_equal(got[b], d.T @ d), b


def test_config1_posterior_covariance_end_to_end():
    """Config 1 (g = [3, 1, 4, 1], γ = 0.5) through MCMCSampler.run with 512 chains: the pooled
    covariance is within 0.1 sqrt(Σ_ii Σ_jj) of the exact Σ, entry by entry (the margin
    tests/test_gpu_examples.py uses for the variances), and the largest off-diagonal
    correlation of the exact posterior has the right sign."""
    spec = importlib.util.spec_from_file_location("stuart_examples", os.path.join(REPO, "examples", "stuart_examples.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    gamma = 0.5
    g = ex.digits(np.pi, 4).astype(float)
    r = ex.run_example("config1", g.reshape(1, 4), ex.digits(np.e, 4).astype(float), gamma,
                       ex.GaussianDistribution(mean=0, covariance=gamma**2), chains=512, n_samples=200)
    cov, exact = np.array(r["posterior_cov"]), np.array(r["exact_cov"])
    scale = np.sqrt(np.outer(np.diag(exact), np.diag(exact)))
    print("config 1 covariance error / scale", np.abs(cov - exact).max(), (np.abs(cov - exact) / scale).max())
    assert np.all(np.abs(cov - exact) <= 0.1 * scale), (cov, exact)
    corr = exact / scale
    off = np.abs(corr - np.diag(np.diag(corr)))
    i, j = np.unravel_index(np.argmax(off), off.shape)
    assert (i, j) in ((0, 2), (2, 0)) and corr[i, j] < 0
    assert np.sign(cov[i, j]) == np.sign(exact[i, j])
