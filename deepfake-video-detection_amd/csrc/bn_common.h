// What the BatchNorm sources share (k_bn.hip, k_frame.hip, k_se.hip, bnfin.h, k_mbconv7.hip): the per-channel
// finalize arithmetic and the channel grouping of the reductions.  The epilogues take loaded values and store
// nothing: each kernel keeps its own loads (before its reduction, where it has one) and stores.
#pragma once
#include "common.h"

namespace dfd {

// channel groups of <= 16 eight-channel vectors, as EVEN as possible: C = 144 (18 vectors) is two
// groups of 9, not 16 + 2 (whose second group's workgroups ran a full-length loop with 2 of 16
// vectors busy: 2x the time of the layer's data on blocks.2.x)
inline void bn_vpg_groups(int C, int& vpg, int& groups) {
  const int nv = C / 8;
  groups = cdiv(nv, 16);
  vpg = cdiv(nv, groups);
}

// Forward finalize of one channel.  Training: from its fp64 mean m and clamped (>= 0) biased variance
// var over count elements, with the momentum update (rm, rv) of the running pair (unbiased variance)
// where run is set.  Eval: from the running pair.  scale and shift follow both in ONE place: shift is
// a fused multiply-subtract only while its product sits next to it.
struct BnFwdCoef { float mu, is, sc, sh, rm, rv; };
__device__ __forceinline__ BnFwdCoef bn_fwd_epilogue(double m, double var, int64_t count, float gamma, float beta,
                                                   float run_mean, float run_var, float momentum, float eps,
                                                   int training, bool run) {
  BnFwdCoef o{};
  if (training) {
    o.mu = (float)m;
    o.is = (float)(1.0 / sqrt(var + (double)eps));
    if (run) {
      const double n = (double)count;
      const double unb = count > 1 ? var * n / (n - 1.0) : var;  // n - 1.0 is exact: count < 2^53
      o.rm = (float)((1.0 - momentum) * run_mean + momentum * m);
      o.rv = (float)((1.0 - momentum) * run_var + momentum * unb);
    }
  } else {
    o.mu = run_mean;
    o.is = 1.0f / sqrtf(run_var + eps);
  }
  o.sc = gamma * o.is;
  o.sh = beta - o.mu * o.sc;
  return o;
}

// Backward finalize of one channel from s = sum g and q = sum g*xhat (fp64): db, dg and the coefficients
// of dy = k1*g + k2*y + k3 (centred: k3 without the k2*mean term, dy = k1*g + k2*(y - mean) + k3).
// Eval (training == 0): k2 = k3 = 0.
struct BnBwdCoef { float db, dg, k1, k2, k3; };
__device__ __forceinline__ BnBwdCoef bn_bwd_epilogue(double s, double q, float gamma, float invstd, float mean,
                                                    int64_t count, int training, int centred) {
  const double gm = gamma, is = invstd;
  const double k1 = gm * is;
  double k2 = 0.0, k3 = 0.0;
  if (training) {
    const double n = (double)count;
    k2 = -gm * is * is * q / n;
    k3 = -gm * is * s / n;
    if (!centred) k3 += gm * is * is * (double)mean * q / n;
  }
  return BnBwdCoef{(float)s, (float)q, (float)k1, (float)k2, (float)k3};
}

}  // namespace dfd
