"""The Burgers study of examples/burgers_beta.py through tempered SMC instead of independent chains.

Same problem: Burgers' equation on (-1, 1) with N = 128 cells to T = 1 by the reference's Rusanov scheme
(CFL time stepping), perturbed Riemann initial condition (δ1, δ2, σ0) with truth (0.025, -0.025, -0.02),
five windowed measurements, noise-free data, noise std 0.05, prior N((1.5, 0.25, -0.5), 0.25² I).  The
plain pCN chains of burgers_beta.py start at the prior mean and 27 % of them end within 0.05 of the truth
after 5 000 steps; the others stay in other minima of the misfit.  Here the particles start as draws from
the prior and the temperature ladder carries them to the posterior (TemperedSMC, pCN mutations with the
report's β = 0.15).

  python examples/burgers_smc.py [particles] [steps_per_stage]

Prints one JSON line: the ladder, the log-evidence, the share of particles within 0.05 of the truth, the
posterior mean and standard deviation of (δ1, δ2, σ0), the accept rates and the wall time.
"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ip_mcmc_amd import BurgersOperator, EvolutionPotential, GaussianDistribution, TemperedSMC  # noqa: E402


def main():
    particles = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    prior_mean = np.array([1.5, 0.25, -0.5])
    truth = np.array([0.025, -0.025, -0.02])
    G = BurgersOperator(prior_mean=prior_mean, N=128, T=1.0, dt_mode="cfl")
    y = G(truth - prior_mean)  # noise-free data, as the reference (burgers_beta.py:118)
    pot = EvolutionPotential(G, y, GaussianDistribution(np.zeros(5), 0.05**2 * np.eye(5)))
    prior = GaussianDistribution(np.zeros(3), 0.25**2 * np.eye(3))

    smc = TemperedSMC(prior, pot, beta=0.15, rng=2)
    t0 = time.perf_counter()
    res = smc.run(n_particles=particles, steps_per_stage=steps, ess_frac=0.5, results="host")
    wall = time.perf_counter() - t0
    post = res.particles + prior_mean
    near = np.max(np.abs(post - truth), axis=1) < 0.05
    print(json.dumps({
        "study": "tempered SMC, pCN beta 0.15",
        "particles": particles,
        "steps_per_stage": steps,
        "stages": res.n_stages,
        "temperatures": res.temperatures.tolist(),
        "ess": res.ess.tolist(),
        "log_evidence": res.log_evidence,
        "fraction_of_particles_near_truth": float(near.mean()),
        "posterior_mean_d1_d2_s0": post.mean(axis=0).tolist(),
        "posterior_std_d1_d2_s0": post.std(axis=0).tolist(),
        "truth_d1_d2_s0": truth.tolist(),
        "accept_rate": res.accept_rate.tolist(),
        "invalid_particles": int((~np.isfinite(res.phi)).sum()),
        "path": res.last_path,
        "wall_s": wall,
    }))


if __name__ == "__main__":
    main()
