// Focal and label-smoothed classification losses on gfx950: the two criteria of the reference's
// ImprovedTrainer (src/train_improved.py:29-78 FocalLoss, :136-150 nn.CrossEntropyLoss(weight,
// label_smoothing)), forward and backward.
//
//   focal : q = eps/(C-1) everywhere (0 if C == 1), 1-eps at the label;  L = -sum_c q_c log p_c;
//           pt = sum_c q_c p_c;  loss_b = w[y_b] (1-pt)^gamma L;  mean = sum / B (not weight-normalised).
//           0 < gamma < 1 with pt rounding to 1 is undefined (inf * 0 in the gradient), as in the reference.
//   ce    : loss_b = (1-eps) w[y_b] (-log p_y) + (eps/C) sum_c w_c (-log p_c), 0 on ignore_index rows;
//           mean = sum / sum of w[y_b] over the rows that are not ignored (torch's cross_entropy).
//
// Forward: one wave per row, lanes striding over the classes (C <= 1024: at most 16 logits per lane, kept
// in registers so the row is read once); the wave reductions are xor butterflies, the same order on every
// run.  It saves the row softmax p and per row (L, pt) -- in ce mode (loss_b, S = sum_c q_c) -- and the
// applied weight w[y_b], so the backward reads no logits and makes no label-indexed read.  mean / sum are a
// second one-workgroup launch that adds the row losses in a fixed order (no floating-point atomics).
// Backward: one launch, one thread per logit; the upstream gradient is read from device memory.
//
// Labels: w[y] and the label's logit are only touched when 0 <= y < C.  A row whose label is outside that
// range (and, in ce mode, is not ignore_index) gets a NaN loss and a zero gradient; in ce mode it counts
// as ignored in the mean's denominator.
#include "kernels.h"

namespace dfd {

constexpr int kLossPerLane = kLossMaxClasses / 64;

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// work (floats): p[B*C] | L[B] | pt[B] | wrow[B] | rows[B] | den[1]
struct LossWork {
  float *p, *L, *pt, *wrow, *rows, *den;
};
static LossWork loss_work(float* w, int64_t B, int64_t C) {
  LossWork k;
  k.p = w;
  k.L = k.p + B * C;
  k.pt = k.L + B;
  k.wrow = k.pt + B;
  k.rows = k.wrow + B;
  k.den = k.rows + B;
  return k;
}
int64_t loss_work_floats(int B, int C) { return (int64_t)B * C + 4 * (int64_t)B + 1; }

__global__ __launch_bounds__(256) void loss_rows_kernel(LossDesc d, const float* __restrict__ z,
                                                        const int64_t* __restrict__ y, const float* __restrict__ w,
                                                        LossWork k, float* __restrict__ rows) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= d.B) return;  // whole waves leave; the kernel has no workgroup barrier
  const int C = d.C;
  const bool focal = d.mode == LOSS_FOCAL;
  const int64_t lab = y[b];
  const bool ignored = !focal && lab == d.ignore;
  const bool valid = !ignored && lab >= 0 && lab < C;
  const float* zb = z + b * C;
  float zr[kLossPerLane];
  float mx = -INFINITY;
#pragma unroll
  for (int i = 0; i < kLossPerLane; ++i) {
    const int c = lane + 64 * i;
    zr[i] = c < C ? zb[c] : -INFINITY;
    mx = fmaxf(mx, zr[i]);
  }
  mx = wave_max(mx);
  float se = 0.f;
#pragma unroll
  for (int i = 0; i < kLossPerLane; ++i)
    if (lane + 64 * i < C) se += expf(zr[i] - mx);
  const float lse = logf(wave_sum(se));
  const float wy = valid ? (w ? w[lab] : 1.f) : 0.f;
  // focal: a0 = sum q_c log p_c, a1 = sum q_c p_c;  ce: a0 = sum w_c log p_c, a1 = sum w_c, a2 = log p_y
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
  for (int i = 0; i < kLossPerLane; ++i) {
    const int c = lane + 64 * i;
    if (c < C) {
      const float lp = zr[i] - mx - lse;
      const float pk = expf(lp);
      k.p[b * C + c] = pk;
      if (focal) {
        const float q = c == lab ? d.q_on : d.q_off;
        a0 += q * lp;
        a1 += q * pk;
      } else {
        const float wc = w ? w[c] : 1.f;
        a0 += wc * lp;
        a1 += wc;
        if (c == lab) a2 = lp;
      }
    }
  }
  a0 = wave_sum(a0);
  a1 = wave_sum(a1);
  a2 = wave_sum(a2);
  if (lane != 0) return;
  float loss, s0, s1;
  if (focal) {
    s0 = -a0;
    s1 = a1;
    loss = wy * powf(1.f - a1, d.gamma) * s0;
  } else {
    s1 = d.q_on * wy + d.q_off * a1;
    loss = ignored ? 0.f : d.q_on * wy * -a2 + d.q_off * -a0;
    s0 = loss;
  }
  if (!valid && !ignored) loss = NAN;
  k.L[b] = s0;
  k.pt[b] = s1;
  k.wrow[b] = wy;
  rows[b] = loss;
  if (b == 0 && d.reduction == LOSS_REDUCE_NONE) k.den[0] = 1.f;
}

// mean / sum of the row losses: one workgroup, thread t adds rows t, t + 256, ... in fp64, then a fixed tree
__global__ __launch_bounds__(256) void loss_reduce_kernel(LossDesc d, LossWork k, float* __restrict__ out) {
  __shared__ double sn[256], sd[256];
  double num = 0.0, den = 0.0;
  for (int64_t b = threadIdx.x; b < d.B; b += 256) {
    num += (double)k.rows[b];
    den += (double)k.wrow[b];
  }
  sn[threadIdx.x] = num;
  sd[threadIdx.x] = den;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      sn[threadIdx.x] += sn[threadIdx.x + o];
      sd[threadIdx.x] += sd[threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double div = d.reduction == LOSS_REDUCE_SUM ? 1.0 : d.mode == LOSS_FOCAL ? (double)d.B : sd[0];
    out[0] = (float)(sn[0] / div);
    k.den[0] = (float)div;
  }
}

// d loss_b / d z_k.  focal, S = sum_c q_c:
//   w [ (1-pt)^gamma (p_k S - q_k) - gamma (1-pt)^(gamma-1) p_k (q_k - pt) L ]   (second term exactly 0 at gamma = 0)
// ce, q'_k = (eps/C) w_k + [k = y] (1-eps) w_y, S = sum_k q'_k:   p_k S - q'_k
__global__ __launch_bounds__(256) void loss_bwd_kernel(LossDesc d, const int64_t* __restrict__ y,
                                                       const float* __restrict__ w, LossWork k,
                                                       const float* __restrict__ gout, float* __restrict__ dz) {
  const int64_t n = (int64_t)d.B * d.C;
  const bool focal = d.mode == LOSS_FOCAL;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / d.C;
    const int c = (int)(i - b * d.C);
    const int64_t lab = y[b];
    if (lab < 0 || lab >= d.C || (!focal && lab == d.ignore)) {
      dz[i] = 0.f;
      continue;
    }
    const float g = d.reduction == LOSS_REDUCE_NONE ? gout[b] : gout[0] / k.den[0];
    const float p = k.p[i], wy = k.wrow[b];
    float t;
    if (focal) {
      const float q = c == lab ? d.q_on : d.q_off;
      const float S = d.q_on + (float)(d.C - 1) * d.q_off;
      const float pt = k.pt[b], base = 1.f - pt;
      t = powf(base, d.gamma) * (p * S - q);
      if (d.gamma != 0.f) t -= d.gamma * powf(base, d.gamma - 1.f) * p * (q - pt) * k.L[b];
      t *= wy;
    } else {
      const float q = d.q_off * (w ? w[c] : 1.f) + (c == lab ? d.q_on * wy : 0.f);
      t = p * k.pt[b] - q;
    }
    dz[i] = g * t;
  }
}

static int loss_check(const LossDesc& d) {
  if (d.B < 1 || d.C < 1 || d.C > kLossMaxClasses) {
    set_error("classification loss: needs B >= 1 and 1 <= C <= 1024", __FILE__, __LINE__);
    return -1;
  }
  if ((d.mode != LOSS_FOCAL && d.mode != LOSS_CE) || d.reduction < LOSS_REDUCE_NONE || d.reduction > LOSS_REDUCE_SUM) {
    set_error("classification loss: unknown mode or reduction", __FILE__, __LINE__);
    return -1;
  }
  return 0;
}

int loss_forward(hipStream_t s, const LossDesc& d, const float* z, const int64_t* y, const float* w, float* work,
                 float* out) {
  DFD_TRY(loss_check(d));
  const LossWork k = loss_work(work, d.B, d.C);
  const bool none = d.reduction == LOSS_REDUCE_NONE;
  hipLaunchKernelGGL(loss_rows_kernel, dim3(cdiv(d.B, 4)), dim3(256), 0, s, d, z, y, w, k, none ? out : k.rows);
  if (!none) hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), dim3(256), 0, s, d, k, out);
  DFD_HIP_CHECK(hipGetLastError());
  return 0;
}

int loss_backward(hipStream_t s, const LossDesc& d, const int64_t* y, const float* w, const float* work,
                  const float* gout, float* dz) {
  DFD_TRY(loss_check(d));
  const LossWork k = loss_work(const_cast<float*>(work), d.B, d.C);
  const int gx = (int)std::min<int64_t>(cdiv64((int64_t)d.B * d.C, 256), 65536);
  hipLaunchKernelGGL(loss_bwd_kernel, dim3(gx), dim3(256), 0, s, d, y, w, k, gout, dz);
  DFD_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace dfd
