// Epoch metrics of a binary classifier (2 logits) on gfx950: the scores of an epoch stay on the device and are
// reduced there, so the host synchronises once per epoch instead of once per step (the reference's
// EnsembleTrainer reads loss.item() and three .cpu() copies after every step, src/ensemble_trainer.py:203-211,
// 266-273).
//
//   metrics_append   : one launch per step, one workgroup striding over the B rows.  Row r goes to position
//                      offset + r: the fake-class probability softmax(z)[1] in fp32 (max-subtracted, expf) and a
//                      one-byte tag, bit 0 the label, bit 1 the argmax prediction (z1 > z0; a tie is class 0, as
//                      torch.argmax), bit 2 "labelled" (label 0 or 1).  Any other label (train.py:155 writes -1
//                      for an unlabelled clip) is stored with bit 2 clear and skipped by the finalize, so the
//                      host's row count never depends on device data.  The launcher refuses rows past the
//                      buffers' capacity (rows, passed by the caller).  Thread 0 adds the step's loss (a device
//                      scalar) to two fp64 sums, loss and loss * B: appends run in stream order and each makes
//                      one fp64 add, the sum Python's `total += loss.item()` makes from the same fp32 losses.
//   metrics_finalize : an async memset of the int64 result block, then two kernels over the N stored rows.
//                      counts: n_pos, n_neg, the confusion counts of the argmax predictions and, per threshold,
//                      the true and false positives of `prob >= thr` in fp32 -- registers, wave64 shuffle
//                      reduce, LDS, one integer atomic per counter per workgroup.
//                      auc: U2 = sum over (i positive, j negative) of 2 [p_i > p_j] + [p_i == p_j], the exact
//                      Mann-Whitney count doubled, over 256 x 256 tiles; AUC = U2 / (2 n_pos n_neg) on the host.
//                      Integer adds commute: the block is the same bits on every run.
//
// Result block (int64 words): 0 n_pos, 1 n_neg, 2 tn, 3 fp, 4 fn, 5 tp, 6 U2, 7 unused, 8 + t tp_t, 40 + t fp_t.
#include "kernels.h"

namespace dfd {

constexpr int kTagLabel = 1, kTagPred = 2, kTagValid = 4;
constexpr int kMetricsCounters = 6 + 2 * kMetricsMaxThresholds;  // per-workgroup integer counters of the counts kernel

struct MetricsThresholds {
  float v[kMetricsMaxThresholds];  // +inf past the caller's count: `prob >= inf` holds for no stored probability
};

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void metrics_append_kernel(const float* __restrict__ z,
                                                             const int64_t* __restrict__ y,
                                                             const float* __restrict__ loss, int B, int64_t offset,
                                                             float* __restrict__ probs, uint8_t* __restrict__ tags,
                                                             double* __restrict__ sums) {
  for (int r = threadIdx.x; r < B; r += 256) {
    const float z0 = z[2 * (int64_t)r], z1 = z[2 * (int64_t)r + 1];
    const float mx = fmaxf(z0, z1);
    const float e0 = expf(z0 - mx), e1 = expf(z1 - mx);
    const int64_t lab = y[r];
    probs[offset + r] = e1 / (e0 + e1);
    tags[offset + r] = (uint8_t)((lab == 1 ? kTagLabel : 0) | (z1 > z0 ? kTagPred : 0) |
                                 (lab == 0 || lab == 1 ? kTagValid : 0));
  }
  if (threadIdx.x == 0 && loss) {
    const double l = (double)loss[0];
    sums[0] += l;
    sums[1] += l * (double)B;
  }
}

// c[0..5] = n_pos, n_neg, tn, fp, fn, tp; c[6 + t] = tp_t, c[6 + 32 + t] = fp_t
__global__ __launch_bounds__(256) void metrics_counts_kernel(const float* __restrict__ probs,
                                                             const uint8_t* __restrict__ tags, int64_t N,
                                                             MetricsThresholds thr,
                                                             unsigned long long* __restrict__ result) {
  __shared__ unsigned part[4][kMetricsCounters];
  unsigned c[kMetricsCounters];
#pragma unroll
  for (int k = 0; k < kMetricsCounters; ++k) c[k] = 0;
  // a thread visits at most N / 256 + 1 rows: 32-bit counters hold up to N = 2^40
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
    const int t = tags[i];
    if (!(t & kTagValid)) continue;
    const float p = probs[i];
    const unsigned pos = t & kTagLabel, neg = pos ^ 1u, pred = (t & kTagPred) ? 1u : 0u;
    c[0] += pos;
    c[1] += neg;
    c[2] += neg & (pred ^ 1u);
    c[3] += neg & pred;
    c[4] += pos & (pred ^ 1u);
    c[5] += pos & pred;
#pragma unroll
    for (int k = 0; k < kMetricsMaxThresholds; ++k) {
      const unsigned hit = p >= thr.v[k] ? 1u : 0u;
      c[6 + k] += hit & pos;
      c[6 + kMetricsMaxThresholds + k] += hit & neg;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kMetricsCounters; ++k) {
    const unsigned s = wave_sum_u32(c[k]);
    if (lane == 0) part[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < kMetricsCounters) {
    const int k = threadIdx.x;
    const unsigned long long s = (unsigned long long)part[0][k] + part[1][k] + part[2][k] + part[3][k];
    const int word = k < 6 ? k : k < 6 + kMetricsMaxThresholds ? 8 + (k - 6) : 40 + (k - 6 - kMetricsMaxThresholds);
    if (s) atomicAdd(&result[word], s);
  }
}

// Tile (ti, tj): thread t owns row i = 256 ti + t and walks the tile's 256 rows j in LDS.  The tags are folded into
// the staged probabilities: a row that is not a labelled positive (as i) or not a labelled negative (as j), or lies
// past N, is staged as NaN, and both comparisons are false on a NaN -- the inner loop reads no tag.
__global__ __launch_bounds__(256) void metrics_auc_kernel(const float* __restrict__ probs,
                                                          const uint8_t* __restrict__ tags, int64_t N,
                                                          unsigned long long* __restrict__ result) {
  __shared__ __attribute__((aligned(16))) float pj[256];
  __shared__ unsigned long long part[4];
  const int64_t nt = (N + 255) / 256;
  unsigned long long acc = 0;
  for (int64_t ti = blockIdx.x; ti < nt; ti += gridDim.x) {
    const int64_t i = ti * 256 + threadIdx.x;
    float pi = NAN;
    if (i < N) {
      const int t = tags[i];
      if ((t & kTagValid) && (t & kTagLabel)) pi = probs[i];
    }
    for (int64_t tj = blockIdx.y; tj < nt; tj += gridDim.y) {
      const int64_t j = tj * 256 + threadIdx.x;
      float v = NAN;
      if (j < N) {
        const int t = tags[j];
        if ((t & kTagValid) && !(t & kTagLabel)) v = probs[j];
      }
      __syncthreads();  // the previous tile's readers are done
      pj[threadIdx.x] = v;
      __syncthreads();
      unsigned u = 0;  // at most 2 * 256 per tile
#pragma unroll 8
      for (int k = 0; k < 256; k += 4) {
        const float4 q = *reinterpret_cast<const float4*>(&pj[k]);
        u += (pi > q.x ? 2u : 0u) + (pi == q.x ? 1u : 0u);
        u += (pi > q.y ? 2u : 0u) + (pi == q.y ? 1u : 0u);
        u += (pi > q.z ? 2u : 0u) + (pi == q.z ? 1u : 0u);
        u += (pi > q.w ? 2u : 0u) + (pi == q.w ? 1u : 0u);
      }
      acc += u;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long s = part[0] + part[1] + part[2] + part[3];
    if (s) atomicAdd(&result[6], s);
  }
}

int metrics_append(hipStream_t s, const float* logits, const int64_t* labels, const float* loss, int B, int64_t offset,
                   int64_t capacity, float* probs, uint8_t* tags, double* loss_sums) {
  if (B <= 0 || offset < 0 || capacity - offset < B) {
    set_error("metrics_append: needs B >= 1 and 0 <= offset <= capacity - B", __FILE__, __LINE__);
    return -1;
  }
  if (!logits || !labels || !probs || !tags || !loss_sums) {
    set_error("metrics_append: null argument", __FILE__, __LINE__);
    return -1;
  }
  hipLaunchKernelGGL(metrics_append_kernel, dim3(1), dim3(256), 0, s, logits, labels, loss, B, offset, probs, tags,
                     loss_sums);
  DFD_HIP_CHECK(hipGetLastError());
  return 0;
}

int metrics_finalize(hipStream_t s, const float* probs, const uint8_t* tags, int64_t N, const float* thresholds,
                     int n_thresholds, int64_t* result) {
  if (N < 0 || n_thresholds < 0 || n_thresholds > kMetricsMaxThresholds) {
    set_error("metrics_finalize: needs N >= 0 and at most 32 thresholds", __FILE__, __LINE__);
    return -1;
  }
  if (!probs || !tags || !result || (n_thresholds > 0 && !thresholds)) {
    set_error("metrics_finalize: null argument", __FILE__, __LINE__);
    return -1;
  }
  DFD_HIP_CHECK(hipMemsetAsync(result, 0, kMetricsResultWords * sizeof(int64_t), s));
  if (N == 0) return 0;
  MetricsThresholds thr;
  for (int k = 0; k < kMetricsMaxThresholds; ++k) thr.v[k] = k < n_thresholds ? thresholds[k] : INFINITY;
  unsigned long long* r = reinterpret_cast<unsigned long long*>(result);
  const int gx = (int)std::min<int64_t>(cdiv64(N, 256), 1024);
  hipLaunchKernelGGL(metrics_counts_kernel, dim3(gx), dim3(256), 0, s, probs, tags, N, thr, r);
  const int gt = (int)std::min<int64_t>(cdiv64(N, 256), 1024);
  hipLaunchKernelGGL(metrics_auc_kernel, dim3(gt, gt), dim3(256), 0, s, probs, tags, N, r);
  DFD_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace dfd
