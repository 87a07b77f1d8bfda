// The speculative pCN sweep of a chain whose state is three parameters
// replicated on every lane: one chain's whole launch.  The chain owns S slots
// of L consecutive lanes, G = S·L <= 64 lanes of one wave; slot n is node n of
// the speculation tree for the chain's recent acceptance rate and the chain
// walks the tree along the real decisions (ipmc_sweep_common.hpp) --
// bit-identical to S = 1, the sequential chain.
//
// l96ts_sweep_kernel runs on it.  burgers_sweep_kernel keeps its own copy of
// the round, with its block-wide rounds: on a shared body with a compile-time
// block-wide flag it was bit-exact but measured slower in five of fourteen
// Burgers timings, one by 14 % (profiles/r15/README.md).
//
// The kernel supplies its geometry -- chain, r (the lane's index among the
// chain's G lanes), L and cbase (the chain's first lane in the wave) -- its LDS
// and Φ; every lane of a live chain calls this, idle lanes have returned.
//
// Cross-lane reads.  On gfx950 a __shfl (ds_bpermute) from a lane whose EXEC
// bit is off reads 0, so a cross-lane read is executed only by lanes whose
// source lanes share their control flow.  The reads of this body
// -- the origin's proposal and Φ, the winner's proposal and Φ -- sit at the top
// level of the round loop, which every lane of the chain runs for the same
// number of rounds (st, S, tb and the round's outcome are uniform per chain),
// and their sources are lanes of the chain; the ballots of the decision are
// wave-wide and masked to the chain.  The recorded states are read from the LDS
// park: no cross-lane read inside the replay's data-dependent loop.
#pragma once

#include "ipmc_sweep_common.hpp"

namespace ipmc {

// vpk: the park, three rows for the proposals of the block's BLK lanes.
// phi_of(v) -> Φ(v) without the regulariser, valid on every lane of the slot;
// the lanes of an evaluated slot call it together.
// s is taken by value: through a reference to the kernel's argument every
// instantiation of l96ts_sweep_kernel needed 2-5 more VGPRs (its fields were
// loaded once and kept instead of re-read from the kernel arguments), which
// cost four of them an occupancy step and others scratch.
template <typename T, bool FM, int BLK, class Phi>
__device__ __forceinline__ void spec_sweep3(const ipmc_sweep s, int S, int64_t chain, int r, int L, int cbase,
                                            T (*vpk)[BLK], Phi&& phi_of) {
  const int t = threadIdx.x, lane = t & 63;
  const int G = S * L, slot = r / L;
  const bool first = r == slot * L;  // the slot's first lane casts its ballots
  const int t0 = t - r;              // the chain's first thread in the block
  const uint64_t gid = (uint64_t)(s.chain_offset + chain);
  T* u = (T*)s.u + chain * 3;
  T ur[3] = {u[0], u[1], u[2]};  // every lane of the chain keeps the chain state
  const T* sq = (const T*)s.prior_sqrt;
  const T* chol = (const T*)s.prior_chol;
  const T beta = (T)s.beta, contr = (T)s.contraction;
  const bool rw = s.proposal == IPMC_PROPOSAL_RW;
  T* phi = (T*)s.phi;
  T phu = phi[chain];
  const unsigned long long gmask = (G >= 64) ? ~0ull : ((1ull << G) - 1);
  const bool rec = s.sum_u || s.sample_every > 0;  // uniform per chain (only lane r == 0 keeps the clock)
  int nacc = 0, ncalls = 0;
  SampleClock clk(s);
  int64_t st = 0;
  SpecGuess guess(spec_accept_prior(s, chain));  // the speculation tree (ipmc_sweep_common.hpp)
  while (st < s.n_steps) {
    const int64_t left = s.n_steps - st;
    const int tb = S > 1 ? guess.bucket() : 0;
    const SpecNode nd = kSpecTrees.nd[tb][slot];
    const int maxlvl = kSpecTrees.maxlvl[tb][S];
    const bool act = nd.depth < left;  // uniform per slot
    const int64_t tt = st + nd.depth;
    const int ol = cbase + (nd.orig < 0 ? 0 : nd.orig) * L;  // the origin slot's first lane
    bool ok = false;
    T phv = (T)0;
    double lr = 0.0;
    const uint64_t step = s.step0 + (uint64_t)tt;
    T w[3];
    if (act) pcn_noise<T, 3>(sq, s.seed, gid, step, 0, w, chol, 3);
    const T bs = (act && s.beta_schedule) ? (T)s.beta_schedule[2 * tt] : beta;
    const T cs = (act && s.beta_schedule) ? (T)s.beta_schedule[2 * tt + 1] : contr;
    // the proposals level by level (every lane of a slot holds its proposal):
    // a node's origin was formed one level before
    T v[3] = {(T)0, (T)0, (T)0};
    for (int lv = 0; lv <= maxlvl; ++lv) {
      T o[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) o[j] = __shfl(v[j], ol, 64);
      if (act && nd.lvl == lv) {
#pragma unroll
        for (int j = 0; j < 3; ++j) v[j] = propose_one<T>(rw, nd.orig < 0 ? ur[j] : o[j], w[j], cs, bs);
      }
    }
    if (act) {  // uniform per slot
      ok = box_valid<T, 3, 1>(s, 0, v, lane);
      if (ok) {
        phv = phi_of(v);
        if (s.reg_scale) phv = phv + regularizer<T, 3, 1, FM>((const T*)s.reg_scale, v, lane);
        lr = det_log(accept_uniform(s.seed, gid, step));
      }
    }
    // pcn_accept against the state this node proposed from: the chain's, or
    // its origin node's proposal (whose Φ that slot's lanes hold)
    const T pho = __shfl(phv, ol, 64);
    const bool acc = ok && (double)((nd.orig < 0 ? phu : pho) - phv) > lr;
    const SpecWaveRound wr = spec_wave_round(acc, ok, first, cbase, gmask, S, L, tb, slot, act);
    const SpecRound rd = wr.rd;
    // the new state: the winner's proposal and Φ
    const int wl = cbase + (rd.win >= 0 ? rd.win : 0) * L;
    T vf[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) vf[j] = __shfl(v[j], wl, 64);
    const T phf = __shfl(phv, wl, 64);
    if (rec) {
      // the states after each settled step, in step order: the same path
      // again, the proposals read from the LDS park (every lane of the chain
      // reads, lane r == 0 records)
#pragma unroll
      for (int j = 0; j < 3; ++j) vpk[j][t] = v[j];
      wave_sync_lds();
      const bool sums = s.sum_u && r == 0;
      RoundSums<3> rsum(sums ? s.sum_u + chain * 3 : nullptr, (sums && s.sum_u2) ? s.sum_u2 + chain * 3 : nullptr,
                        sums ? 3 : 0);
      spec_path_replay(wr.path, wr.accm, [&](int q, int la) {
        T vq[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) vq[j] = vpk[j][t0 + (la >= 0 ? la : 0) * L];
        if (r == 0) {
          if (sums) {
#pragma unroll
            for (int j = 0; j < 3; ++j) rsum.add(j, la >= 0 ? (double)vq[j] : (double)ur[j]);
          }
          if (s.sample_every > 0 && clk.next == st + q) {
            // the state after step st+q is a sample
            const int64_t sl = clk.take(clk.next);
            T* so = (T*)s.sample_out + chain * s.sample_stride + sl * s.sample_step_stride;
#pragma unroll
            for (int j = 0; j < 3; ++j) so[j] = la >= 0 ? vq[j] : ur[j];
          }
        }
      });
      if (sums) rsum.store();
      wave_sync_lds();  // the park is rewritten next round
    }
    if (rd.win >= 0) {
#pragma unroll
      for (int j = 0; j < 3; ++j) ur[j] = vf[j];
      phu = phf;
    }
    nacc += rd.nar;
    ncalls += rd.calls;
    guess.settle(rd.nar, rd.used);
    st += rd.used;
  }
  if (r == 0) {
    phi[chain] = phu;
    if (s.accepts) s.accepts[chain] += nacc;
    if (s.calls) s.calls[chain] += ncalls;
#pragma unroll
    for (int j = 0; j < 3; ++j) u[j] = ur[j];
    if (s.sample_out && s.sample_every == 0) {
      T* so = (T*)s.sample_out + chain * s.sample_stride;
#pragma unroll
      for (int j = 0; j < 3; ++j) so[j] = ur[j];
    }
  }
}

}  // namespace ipmc
