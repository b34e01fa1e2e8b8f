// Serving an EnsembleDetector on gfx950: the combination of the members' outputs (src/pretrained_detector.py:196-216)
// and the fp32 arithmetic of the app's decision step (app.py:2090-2094, 2130-2143; the enhanced agent's softmaxes,
// src/enhanced_decision_agent.py:115-138) for a batch of videos in ONE launch, so the host reads one small block
// back per batch instead of M + 2 scalars per video after running every member twice.
//
//   member logits (M, V, 2), member frame scores (M, V, T), raw ensemble weights (M) or null
//     -> ensemble logits (V, 2)   average: sum over m in the order of torch's CPU sum (below), then / M: torch's mean
//                                 weighted: w = softmax(weights) (max-subtracted, expf), sum over m of z_m * w_m with
//                                           the product and the sum rounded separately (no contraction: Makefile)
//                                 voting: one-hot of the modal argmax; argmax ties -> class 0 (z1 > z0 votes 1),
//                                         mode ties -> class 0 (2 * votes1 > M picks 1), as torch.argmax / torch.mode
//        ensemble scores (V, T)   weighted: the weighted sum; average and voting: the mean over the members
//        decision block (V, 5 + 2M), fp32 words per video:
//          0 prob_fake = softmax(ensemble logits)[fake_idx]        1 prob_real = softmax(ensemble logits)[1 - fake_idx]
//          2 softmax(ensemble logits / temperature)[fake_idx]      3 the modal argmax of the members (0.0 or 1.0)
//          4 M as a float (layout check)
//          5 + m      softmax(z_m)[fake_idx]                  (the app's ind_probs)
//          5 + M + m  softmax(z_m / temperature)[fake_idx]    (the agent's individual_probs)
//
// Everything past these fp32 values (np.std, agreement, thresholds, the formatted strings) is Python-float (double)
// arithmetic in the reference and stays on the host.  The grid is tiny (one thread per video, V * T score elements
// strided over the same threads): 256-thread workgroups, no LDS, no cross-lane traffic, every global store a plain
// per-lane vector store.
#include "kernels.h"

namespace dfd {

struct Softmax2 {
  float p0, p1;
};

// torch's softmax over 2 values: subtract the maximum, expf, divide by the sum
__device__ __forceinline__ Softmax2 softmax2(float z0, float z1) {
  const float mx = fmaxf(z0, z1);
  const float e0 = expf(z0 - mx), e1 = expf(z1 - mx);
  const float s = e0 + e1;
  return {e0 / s, e1 / s};
}

__global__ __launch_bounds__(256) void ensemble_decide_kernel(const float* __restrict__ zl, const float* __restrict__ zs,
                                                              const float* __restrict__ weights, int M, int64_t V,
                                                              int T, int method, int fake_idx, float temperature,
                                                              float* __restrict__ logits, float* __restrict__ scores,
                                                              float* __restrict__ block) {
  float w[kEnsembleMaxMembers];
  if (method == kEnsembleWeighted) {
    float mx = weights[0];
    for (int m = 1; m < M; ++m) mx = fmaxf(mx, weights[m]);
    float sum = 0.f;
    for (int m = 0; m < M; ++m) {
      w[m] = expf(weights[m] - mx);
      sum += w[m];
    }
    for (int m = 0; m < M; ++m) w[m] = w[m] / sum;
  }
  const int64_t stride = (int64_t)gridDim.x * 256;
  const int64_t first = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const float fM = (float)M;
  const int words = kEnsembleBlockBase + 2 * M;
  // The order of the adds over the members is torch's CPU sum over dim 0 of the (M, V, 2) tensor (cascade_sum,
  // 8-float vectors), so that the average is the bits of torch.mean, the host contract: the 2V output columns in
  // front of `bulk` (whole groups of 4 vectors; below one vector, whole groups of 4 columns) add the members in
  // order, the tail columns add them as four interleaved partial sums (members 0, 4 / 1, 5 / 2, 6 / 3, 7; members
  // past the last whole quad go to partial 0), then ((p0 + p1) + p2) + p3.  With M < 4 the two orders are the same.
  const int64_t cols = 2 * V;
  const int64_t bulk = cols >= 8 ? (cols / 32) * 32 : (cols / 4) * 4;

  for (int64_t v = first; v < V; v += stride) {
    float* __restrict__ b = block + v * words;
    // four partial sums per class: member m adds to partial m & 3 on torch's tail order, to partial 0 otherwise
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, c0 = 0.f, c1 = 0.f, c2 = 0.f, c3 = 0.f;
    const int quads = 2 * v >= bulk ? (M & ~3) : 0;  // members below `quads` are interleaved
    int votes1 = 0;
    for (int m = 0; m < M; ++m) {
      const float* __restrict__ z = zl + ((int64_t)m * V + v) * 2;  // a caller's view may be only 4-byte aligned
      const float z0 = z[0], z1 = z[1];
      const float t0 = method == kEnsembleWeighted ? z0 * w[m] : z0;
      const float t1 = method == kEnsembleWeighted ? z1 * w[m] : z1;
      const int k = m < quads ? (m & 3) : 0;
      if (k == 0) {
        a0 += t0;
        c0 += t1;
      } else if (k == 1) {
        a1 += t0;
        c1 += t1;
      } else if (k == 2) {
        a2 += t0;
        c2 += t1;
      } else {
        a3 += t0;
        c3 += t1;
      }
      votes1 += z1 > z0 ? 1 : 0;
      const Softmax2 p = softmax2(z0, z1);
      const Softmax2 pt = softmax2(z0 / temperature, z1 / temperature);
      b[kEnsembleBlockBase + m] = fake_idx ? p.p1 : p.p0;
      b[kEnsembleBlockBase + M + m] = fake_idx ? pt.p1 : pt.p0;
    }
    const float s0 = ((a0 + a1) + a2) + a3, s1 = ((c0 + c1) + c2) + c3;
    const int mode = 2 * votes1 > M ? 1 : 0;
    float e0, e1;
    if (method == kEnsembleAverage) {
      e0 = s0 / fM;
      e1 = s1 / fM;
    } else if (method == kEnsembleWeighted) {
      e0 = s0;
      e1 = s1;
    } else {
      e0 = mode ? 0.f : 1.f;
      e1 = mode ? 1.f : 0.f;
    }
    logits[v * 2] = e0;
    logits[v * 2 + 1] = e1;
    const Softmax2 p = softmax2(e0, e1);
    const Softmax2 pt = softmax2(e0 / temperature, e1 / temperature);
    b[0] = fake_idx ? p.p1 : p.p0;
    b[1] = fake_idx ? p.p0 : p.p1;
    b[2] = fake_idx ? pt.p1 : pt.p0;
    b[3] = (float)mode;
    b[4] = fM;
  }

  const int64_t n = V * T;
  for (int64_t i = first; i < n; i += stride) {
    float s = 0.f;
    if (method == kEnsembleWeighted) {
      for (int m = 0; m < M; ++m) s += zs[(int64_t)m * n + i] * w[m];
    } else {
      for (int m = 0; m < M; ++m) s += zs[(int64_t)m * n + i];
      s = s / fM;
    }
    scores[i] = s;
  }
}

int64_t ensemble_decide_floats(int M) {
  if (M < 1 || M > kEnsembleMaxMembers) {
    set_error("ensemble_decide_floats: needs 1 <= M <= 8", __FILE__, __LINE__);
    return -1;
  }
  return kEnsembleBlockBase + 2 * (int64_t)M;
}

int ensemble_decide(hipStream_t s, const float* member_logits, const float* member_scores, const float* weights, int M,
                    int64_t V, int C, int T, int method, int fake_idx, float temperature, float* logits, float* scores,
                    float* block) {
  if (M < 1 || M > kEnsembleMaxMembers || C != 2 || T < 1 || T > kEnsembleMaxFrames || V < 1 ||
      V > ((int64_t)1 << 40)) {
    set_error("ensemble_decide: needs 1 <= M <= 8 members, C == 2 classes, 1 <= T <= 64 frames and V >= 1 videos",
              __FILE__, __LINE__);
    return -1;
  }
  if (method != kEnsembleAverage && method != kEnsembleWeighted && method != kEnsembleVoting) {
    set_error("ensemble_decide: method must be 0 (average), 1 (weighted) or 2 (voting)", __FILE__, __LINE__);
    return -1;
  }
  if ((fake_idx != 0 && fake_idx != 1) || !(temperature > 0.f) || !(temperature < INFINITY)) {
    set_error("ensemble_decide: needs fake_idx 0 or 1 and a finite temperature > 0", __FILE__, __LINE__);
    return -1;
  }
  if (!member_logits || !member_scores || !logits || !scores || !block) {
    set_error("ensemble_decide: null argument", __FILE__, __LINE__);
    return -1;
  }
  if (method == kEnsembleWeighted && !weights) {
    set_error("ensemble_decide: the weighted method needs the ensemble's weight vector", __FILE__, __LINE__);
    return -1;
  }
  const int gx = (int)std::min<int64_t>(cdiv64(V * T, 256), 1024);
  hipLaunchKernelGGL(ensemble_decide_kernel, dim3(gx), dim3(256), 0, s, member_logits, member_scores, weights, M, V, T,
                     method, fake_idx, temperature, logits, scores, block);
  DFD_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace dfd
