"""Pooled posterior histograms on the device (ipmc_minmax, ipmc_hist1d,
ipmc_histdd through ip_mcmc_amd.posterior) against the host definition
(backend="host": np.searchsorted on the same values widened to float64) and
against numpy's own np.histogram / np.histogramdd.

Everything compared here is an integer count or a min / max of the inputs:
the comparison is np.array_equal, there is no tolerance.
"""
import functools
import importlib.util
import os

import numpy as np
import pytest

from ip_mcmc_amd import histogramdd, marginal_histograms, support, wasserstein_to_point

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LO, HI = -1.0, 1.5

# (C, n, k): k = 1, a dense k = 3 run, k = 40, the largest k (two component tiles at 20 bins),
# many short chains, and one with ~90 workgroups per component tile (3 MB in f64)
SHAPES = [(3, 7, 1), (5, 33, 3), (2, 130, 40), (1, 9, 256), (300, 5, 17), (64, 2001, 3)]


def on_gpu(x):
    import torch

    return torch.tensor(np.ascontiguousarray(x), device="cuda")  # a copy: the cached inputs are read-only


@functools.lru_cache(maxsize=None)
def adversarial(shape, dtype, bins=20):
    """(C, n, k) samples of `dtype` around [LO, HI] holding every edge of np.linspace(LO, HI, bins + 1),
    its neighbours one ulp (of dtype) to either side, values outside both ends, +-inf and NaN."""
    rng = np.random.default_rng(sum(shape) + bins)
    x = rng.normal(0.2, 0.8, size=shape).astype(dtype)
    e = np.linspace(LO, HI, bins + 1).astype(dtype)
    special = np.concatenate([e, np.nextafter(e, dtype(-np.inf)), np.nextafter(e, dtype(np.inf)),
                              np.array([LO - 1, HI + 1, -np.inf, np.inf, np.nan, np.nan], dtype=dtype)])
    flat = x.reshape(-1)
    # the f64 edges themselves where dtype can hold them, so "on the edge" is exact in f64 too
    pos = rng.integers(0, flat.size, size=max(len(special), flat.size // 3))
    flat[pos] = rng.choice(special, size=len(pos))
    flat[:min(len(special), flat.size)] = special[:flat.size]
    x.setflags(write=False)
    return x


def laid_out(x, layout):
    return x if layout == "time_vars" else np.ascontiguousarray(x.transpose(0, 2, 1))


def assert_same_hist(got, ref):
    for key in ("counts", "below", "above", "edges"):
        assert np.array_equal(got[key], ref[key]), key
    assert got["n"] == ref["n"]
    assert got["counts"].dtype == np.int64


@pytest.mark.parametrize("layout", ["time_vars", "vars_time"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", SHAPES)
def test_marginals_and_support_equal_the_host_definition(shape, dtype, layout):
    x = laid_out(adversarial(shape, dtype), layout)
    t = on_gpu(x)
    ref = marginal_histograms(x, bins=20, range=(LO, HI), layout=layout, backend="host")
    assert_same_hist(marginal_histograms(t, bins=20, range=(LO, HI), layout=layout, backend="device"), ref)
    # every sample is somewhere or NaN
    k = shape[2]
    cnk = x if layout == "time_vars" else x.transpose(0, 2, 1)
    nan = np.isnan(cnk).reshape(-1, k).sum(axis=0)
    assert np.array_equal(ref["counts"].sum(axis=1) + ref["below"] + ref["above"] + nan, np.full(k, ref["n"]))
    assert np.array_equal(support(t, layout=layout, backend="device"), support(x, layout=layout, backend="host"))


@pytest.mark.parametrize("layout", ["time_vars", "vars_time"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_range_none_takes_the_data_support(dtype, layout):
    """range=None: min and max per component on the device, NaN skipped, a constant
    component widened by 0.5 to either side; equal to np.histogram on each component."""
    rng = np.random.default_rng(5)
    x = rng.normal(size=(5, 33, 3)).astype(dtype)
    x[..., 1] = dtype(0.3)  # a constant component: every sample in one bin
    x[2, 5, 0] = np.nan
    xl = laid_out(x, layout)
    got = marginal_histograms(on_gpu(xl), bins=20, layout=layout, backend="device")
    assert_same_hist(got, marginal_histograms(xl, bins=20, layout=layout, backend="host"))
    for v in range(3):
        col = x[..., v].reshape(-1).astype(np.float64)
        col = col[~np.isnan(col)]
        counts, edges = np.histogram(col, bins=20)
        assert np.array_equal(got["counts"][v], counts) and np.array_equal(got["edges"][v], edges)
    assert got["counts"][1].max() == 5 * 33


@pytest.mark.parametrize("layout", ["time_vars", "vars_time"])
def test_strided_view_is_binned_in_place(layout):
    """A burn-in slice samples[:, 3:] of a device tensor goes to the kernels by its strides."""
    x = laid_out(adversarial((300, 5, 17), np.float64), layout)
    t = on_gpu(x)
    tv, xv = (t[:, 3:], x[:, 3:]) if layout == "time_vars" else (t[:, :, 3:], x[:, :, 3:])
    assert not tv.is_contiguous()
    ref = marginal_histograms(xv, bins=20, range=(LO, HI), layout=layout, backend="host")
    assert_same_hist(marginal_histograms(tv, bins=20, range=(LO, HI), layout=layout, backend="device"), ref)
    assert np.array_equal(support(tv, layout=layout, backend="device"), support(xv, layout=layout, backend="host"))
    H, _ = histogramdd(tv, bins=(5, 6, 7), range=[(LO, HI)] * 3, components=(0, 8, 16), layout=layout,
                       backend="device")
    Href, _ = histogramdd(xv, bins=(5, 6, 7), range=[(LO, HI)] * 3, components=(0, 8, 16), layout=layout,
                          backend="host")
    assert np.array_equal(H, Href)


@pytest.mark.parametrize("bins", [1, 4096])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_fewest_and_most_bins(bins, dtype):
    """B = 1, and B = 4096 (one component per tile) with samples on every edge and one ulp off."""
    x = adversarial((5, 33, 3) if bins == 1 else (2, 6200, 3), dtype, bins)
    ref = marginal_histograms(x, bins=bins, range=(LO, HI), backend="host")
    assert_same_hist(marginal_histograms(on_gpu(x), bins=bins, range=(LO, HI), backend="device"), ref)
    if bins == 4096:
        assert np.count_nonzero(ref["counts"]) > 3 * 2000  # the values reach most of the bins


def test_every_sample_in_one_bin():
    """The worst contention: one counter per component takes every add (several workgroups)."""
    x = np.full((64, 2001, 3), 0.25)
    got = marginal_histograms(on_gpu(x), bins=20, range=(LO, HI), backend="device")
    assert_same_hist(got, marginal_histograms(x, bins=20, range=(LO, HI), backend="host"))
    assert np.array_equal(got["counts"].max(axis=1), np.full(3, 64 * 2001))
    H, _ = histogramdd(on_gpu(x), bins=20, range=[(LO, HI)] * 3, backend="device")
    assert H.sum() == H.max() == 64 * 2001


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_histogramdd_lds_and_global_paths_equal_numpy(dtype):
    """20^3 cells are counted in LDS, 128^3 (2^21) by integer adds in global memory;
    components=(0, 2) of k = 3; all equal np.histogramdd (and the host definition)."""
    x = adversarial((64, 2001, 3), dtype)
    t = on_gpu(x)
    flat = x.reshape(-1, 3).astype(np.float64)
    rng3 = [(LO, HI)] * 3
    for bins in (20, 128):
        H, edges = histogramdd(t, bins=bins, range=rng3, backend="device")
        Hnp, enp = np.histogramdd(flat[~np.isnan(flat).any(axis=1)], bins=bins, range=rng3)
        assert H.dtype == np.int64 and H.shape == (bins,) * 3
        assert np.array_equal(H, Hnp)
        assert all(np.array_equal(a, b) for a, b in zip(edges, enp))
        assert np.array_equal(H, histogramdd(x, bins=bins, range=rng3, backend="host")[0])
    H, _ = histogramdd(t, bins=(20, 7), range=rng3[:2], components=(0, 2), backend="device")
    sel = flat[:, [0, 2]]
    assert np.array_equal(H, np.histogramdd(sel[~np.isnan(sel).any(axis=1)], bins=(20, 7), range=rng3[:2])[0])


@pytest.mark.parametrize("layout", ["time_vars", "vars_time"])
def test_histogramdd_four_components_range_none(layout):
    rng = np.random.default_rng(9)
    x = rng.normal(size=(300, 5, 17))
    xl = laid_out(x, layout)
    H, edges = histogramdd(on_gpu(xl), bins=(3, 4, 5, 6), components=(1, 5, 7, 16), layout=layout, backend="device")
    Hnp, enp = np.histogramdd(x.reshape(-1, 17)[:, [1, 5, 7, 16]], bins=(3, 4, 5, 6))
    assert np.array_equal(H, Hnp) and H.sum() == 1500
    assert all(np.array_equal(a, b) for a, b in zip(edges, enp))


def test_host_input_in_three_chunks_gives_the_one_chunk_result():
    x = adversarial((5, 33, 3), np.float64)
    three = 2 * 33 * 3 * 8  # two chains per chunk: 2 + 2 + 1
    one = marginal_histograms(x, bins=20, range=(LO, HI), backend="device")
    assert_same_hist(marginal_histograms(x, bins=20, range=(LO, HI), backend="device", chunk_bytes=three), one)
    assert_same_hist(one, marginal_histograms(x, bins=20, range=(LO, HI), backend="host"))
    clean = np.nan_to_num(x, nan=0.0, posinf=2.0, neginf=-2.0)
    assert np.array_equal(support(clean, backend="device", chunk_bytes=three), support(clean, backend="device"))
    assert_same_hist(marginal_histograms(clean, bins=20, backend="device", chunk_bytes=three),
                     marginal_histograms(clean, bins=20, backend="host"))
    H3, _ = histogramdd(x, bins=20, range=[(LO, HI)] * 3, backend="device", chunk_bytes=three)
    H1, _ = histogramdd(x, bins=20, range=[(LO, HI)] * 3, backend="device")
    assert np.array_equal(H3, H1)
    assert np.array_equal(H1, histogramdd(x, bins=20, range=[(LO, HI)] * 3, backend="host")[0])


def test_burgers_wasserstein_example_at_reduced_size():
    """examples/burgers_wasserstein.py (burgers_wasserstein_chain.py through the public API) with
    256 chains x 320 steps on N = 32 cells: every segment's joint histogram holds each of its
    samples but the dropped ones, and every W1 is finite and >= 0."""
    spec = importlib.util.spec_from_file_location("burgers_wasserstein",
                                                  os.path.join(REPO, "examples", "burgers_wasserstein.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    recs = ex.study(chains=256, steps=320, N=32)
    assert [r["chain_length"] for r in recs] == [159, 79, 39, 19]
    for r in recs:
        assert r["samples"] == 256 * r["chain_length"]
        assert r["counts_sum"] == r["samples"] - r["dropped"]
        assert np.isfinite(r["w1"]) and r["w1"] >= 0
        assert r["w1"] == wasserstein_to_point(np.asarray(r["counts"]), r["intervals"], r["truth"])
