"""The reference's chain-length study of the Burgers posterior
(report/scripts/burgers/burgers_wasserstein_chain.py:164-268) on the GPU, with
many chains pooled instead of one.

Same problem and sampler as examples/burgers_beta.py (Burgers' equation on
(-1, 1) to T = 1, perturbed Riemann initial condition (δ1, δ2, σ0) with truth
(0.025, -0.025, -0.02), five windowed measurements, noise std 0.05, prior
N((1.5, 0.25, -0.5), 0.25² I), VarStepStandardRWProposer with
PWLinear(0.1, 0.001, 250) and StandardRWAccepter, u_0 = 0, every step recorded).

As create_data does (_chain.py:261-266), the samples are cut into four nested
segments: the last half of the chain (from index l + 1), then the last half of
what is left, and so on, so the segments are ever earlier and shorter pieces.
Every chain contributes its piece to the segment's pool.  The support is the
min and max over all segments (_chain.py:171-175), here widened where needed
to hold the truth, since a short run may not have reached it and the distance
to a point outside the grid is not defined; each segment is binned into one
joint 20³ histogram on the device (ip_mcmc_amd.histogramdd) and compared with
the histogram of the ground truth by helpers.wasserstein_distance's W1
(ip_mcmc_amd.wasserstein_to_point: transport to a point mass has a closed form,
POT is not needed).

  python examples/burgers_wasserstein.py [chains] [steps] [N]

Prints one JSON line per segment: its chain length, pooled sample count,
the samples outside the intervals (dropped), W1 to the truth, and the
fraction of the mass in the truth's cell.
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ip_mcmc_amd import (BurgersOperator, CountedAccepter, EvolutionPotential, GaussianDistribution,  # noqa: E402
                         MCMCSampler, PWLinear, StandardRWAccepter, VarStepStandardRWProposer, histogramdd, support,
                         wasserstein_to_point)

N_BINS = 20
N_SEGMENTS = 4


def study(chains=1024, steps=5000, N=128):
    """-> one record per segment, longest first."""
    prior_mean = np.array([1.5, 0.25, -0.5])
    truth = np.array([0.025, -0.025, -0.02])
    G = BurgersOperator(prior_mean=prior_mean, N=N, T=1.0, dt_mode="cfl")
    y = G(truth - prior_mean)  # noise-free data, as the reference
    noise = GaussianDistribution(np.zeros(5), 0.05**2 * np.eye(5))
    prior = GaussianDistribution(prior_mean, 0.25**2 * np.eye(3))
    acc = CountedAccepter(StandardRWAccepter(EvolutionPotential(G, y, noise), prior))
    sampler = MCMCSampler(VarStepStandardRWProposer(PWLinear(0.1, 0.001, 250), prior), acc, np.random.default_rng(2))
    t0 = time.perf_counter()
    samples = sampler.run(np.zeros((chains, 3)), n_samples=steps, burn_in=0, sample_interval=1)  # (C, steps, 3)
    wall = time.perf_counter() - t0
    samples = samples + prior_mean  # _chain.py:258-259

    segments = []
    for _ in range(N_SEGMENTS):  # _chain.py:261-266
        half = samples.shape[1] // 2
        segments.append(samples[:, half + 1:])
        samples = samples[:, :half]

    # the support of the data (_chain.py:171-175): per-segment min and max on the device, combined
    sup = np.stack([support(seg) for seg in segments])
    intervals = np.stack([np.minimum(sup[:, :, 0].min(axis=0), truth), np.maximum(sup[:, :, 1].max(axis=0), truth)],
                         axis=1)
    records = []
    for seg in segments:
        counts, _ = histogramdd(seg, bins=N_BINS, range=intervals)  # one joint 20³ histogram per segment
        flat = seg.reshape(-1, 3)
        dropped = int(np.count_nonzero(~np.all((flat >= intervals[:, 0]) & (flat <= intervals[:, 1]), axis=1)))
        p = counts / counts.sum()
        truth_cell = np.unravel_index(np.argmax(np.histogramdd(truth[None], bins=N_BINS, range=intervals)[0]),
                                      counts.shape)
        records.append({
            "study": "W1 to the truth by chain length (burgers_wasserstein_chain.py)",
            "chains": chains,
            "chain_length": seg.shape[1],
            "samples": flat.shape[0],
            "dropped": dropped,
            "counts_sum": int(counts.sum()),
            "w1": wasserstein_to_point(counts, intervals, truth),
            "mass_in_truth_cell": float(p[truth_cell]),
            "intervals": intervals.tolist(),
            "truth": truth.tolist(),
            "counts": counts.tolist(),
            "accept_rate": float(np.mean(acc.ratio())),
            "sampling_wall_s": wall,
        })
    return records


def main():
    args = [int(a) for a in sys.argv[1:4]]
    chains, steps, N = (args + [1024, 5000, 128][len(args):])
    for r in study(chains, steps, N):
        r = dict(r)
        del r["counts"]  # 8 000 numbers: kept for callers of study(), not printed
        print(json.dumps(r))


if __name__ == "__main__":
    main()
