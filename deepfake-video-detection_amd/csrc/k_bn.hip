// BatchNorm (training batch statistics / eval running statistics) and SiLU kernels for the
// EfficientNet-B0 hot path on gfx950: forward finalize / eval / apply, backward reduce / finalize /
// apply.  (The per-frame reductions are in k_frame.hip, the SE excitation in k_se.hip, the slab
// reducer in k_reduce.hip; the finalize arithmetic all of them share is in bn_common.h.)
//
// Replaces aten batch_norm + silu (timm BatchNormAct2d) reached from
// src/pretrained_detector.py:116, forward and backward.  Every BN statistic is a
// deterministic two-level reduction: producers write per-workgroup partial rows
// [rows][2][C] and bn_finalize sums them in a fixed order (fp64) -- no float atomics in HBM.
#include "kernels.h"

#include <mutex>
#include <utility>
#include <vector>

namespace dfd {

// ------------------------------------------------------------------ partial-row reduction
// Sums rows of a [rows][2][C] slab for channels [blockIdx.x*CH, +CH) in fp64: 1024 threads = CH
// channels x (1024 / CH) row lanes; the row lanes of a wave are added by shuffles, the 16 waves by
// threads 0..CH-1 in wave order (deterministic; one barrier instead of a 6-level LDS tree).  Valid
// in threads 0..CH-1 (channel tid).  CH (16, 8 or 4) is chosen per launch so that each row lane
// reads at most 8 rows (one batch of loads in flight): the producers of the high-resolution maps
// write up to 1,024 partial rows of few channels, where 16 channels per workgroup left one or two
// workgroups walking 16 rows per lane in two dependent batches (10-12 us finalizes).
template <int CH>
__device__ void reduce_stat_rows(const float* __restrict__ stats, int rows, int C, double& s, double& q,
                                 double* sh_s, double* sh_q) {
  constexpr int FIN_CH = CH, FIN_RL = 1024 / CH;
  const int tid = threadIdx.x, cl = tid % FIN_CH, rl = tid / FIN_CH;
  const int c = blockIdx.x * FIN_CH + cl;
  double a = 0.0, b = 0.0;
  if (c < C) {
    // loads of 8 rows issued before their adds (same summation order as one row at a time)
    int r = rl;
    for (; r + 7 * FIN_RL < rows; r += 8 * FIN_RL) {
      float va[8], vb[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        va[u] = stats[((int64_t)(r + u * FIN_RL) * 2 + 0) * C + c];
        vb[u] = stats[((int64_t)(r + u * FIN_RL) * 2 + 1) * C + c];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) { a += va[u]; b += vb[u]; }
    }
    for (; r < rows; r += FIN_RL) {
      a += stats[((int64_t)r * 2 + 0) * C + c];
      b += stats[((int64_t)r * 2 + 1) * C + c];
    }
  }
  // lanes l, l^CH, l^2CH, ... of a wave hold the same channel
#pragma unroll
  for (int o = CH; o < 64; o <<= 1) {
    a += __shfl_xor(a, o, 64);
    b += __shfl_xor(b, o, 64);
  }
  const int wave = tid >> 6;
  if ((tid & 63) < FIN_CH) {
    sh_s[wave * FIN_CH + cl] = a;
    sh_q[wave * FIN_CH + cl] = b;
  }
  __syncthreads();
  s = 0.0;
  q = 0.0;
  if (tid < FIN_CH) {
    for (int w = 0; w < 1024 / 64; ++w) {
      s += sh_s[w * FIN_CH + tid];
      q += sh_q[w * FIN_CH + tid];
    }
  }
}

// channels per finalize workgroup: at most 8 rows per row lane (reduce_stat_rows)
static int fin_ch(int rows) { return rows <= 8 * 64 ? 16 : (rows <= 8 * 128 ? 8 : 4); }

// chan_rows > 0: the rows are centred tile partials (sum, M2 about the tile's own mean) of
// consecutive chan_rows-row tiles (the conv epilogue, k_conv.hip): var = (sum M2 + sum_t n_t
// (mean_t - mean)^2) / n, the second term from a pass over the tile sums once the mean is known
template <int CH>
__device__ void chan_between(const float* __restrict__ stats, int rows, int C, int64_t count, int chan_rows,
                             double* sh_m, double& out, double* sh) {
  constexpr int FIN_RL = 1024 / CH;
  const int tid = threadIdx.x, cl = tid % CH, rl = tid / CH;
  const int c = blockIdx.x * CH + cl;
  double a = 0.0;
  if (c < C) {
    const double m = sh_m[cl];
    for (int r = rl; r < rows; r += FIN_RL) {
      const int64_t left = count - (int64_t)r * chan_rows, nt = left < chan_rows ? left : chan_rows;
      const double d = (double)stats[((int64_t)r * 2 + 0) * C + c] / (double)nt - m;
      a += (double)nt * d * d;
    }
  }
#pragma unroll
  for (int o = CH; o < 64; o <<= 1) a += __shfl_xor(a, o, 64);
  const int wave = tid >> 6;
  if ((tid & 63) < CH) sh[wave * CH + cl] = a;
  __syncthreads();
  out = 0.0;
  if (tid < CH)
    for (int w = 0; w < 1024 / 64; ++w) out += sh[w * CH + tid];
}

template <int FIN_CH>
__global__ __launch_bounds__(1024) void bn_finalize_kernel(const float* __restrict__ stats, int rows, int64_t count,
                                                           int C, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float* run_mean,
                                                           float* run_var, float momentum, float eps, int training,
                                                           float* mean, float* invstd, float* scale, float* shift,
                                                           int chan_rows) {
  __shared__ double sh_s[1024 / 64 * FIN_CH], sh_q[1024 / 64 * FIN_CH], sh_m[FIN_CH];
  const int tid = threadIdx.x;
  const int c = blockIdx.x * FIN_CH + tid;
  // the channel's parameters and running buffers, loaded before the reduction (their latency under
  // the stat-row loads instead of after them: the kernel is a chain of dependent memory round trips)
  float p_g = 0.f, p_b = 0.f, p_rm = 0.f, p_rv = 0.f;
  if (tid < FIN_CH && c < C) {
    p_g = gamma[c];
    p_b = beta[c];
    if (run_mean) { p_rm = run_mean[c]; p_rv = run_var[c]; }
  }
  double s = 0.0, q = 0.0, between = 0.0;
  if (training) reduce_stat_rows<FIN_CH>(stats, rows, C, s, q, sh_s, sh_q);
  if (training && chan_rows > 0) {
    if (tid < FIN_CH) sh_m[tid] = s / (double)count;
    __syncthreads();
    chan_between<FIN_CH>(stats, rows, C, count, chan_rows, sh_m, between, sh_s);
  }
  if (tid < FIN_CH && c < C) {
    double m = 0.0, var = 0.0;
    if (training) {
      m = s / (double)count;
      var = chan_rows > 0 ? (q + between) / (double)count : q / (double)count - m * m;
      if (var < 0.0) var = 0.0;
    }
    const bool run = training && run_mean;
    const BnFwdCoef o = bn_fwd_epilogue(m, var, count, p_g, p_b, p_rm, p_rv, momentum, eps, training, run);
    if (run) { run_mean[c] = o.rm; run_var[c] = o.rv; }
    mean[c] = o.mu;
    invstd[c] = o.is;
    scale[c] = o.sc;
    shift[c] = o.sh;
  }
}

// Many centred partial rows (the CNN-LSTM's early convolutions: up to 200k rows of 64-row tiles): the
// single-pass form over row chunks.  With S = sum_t s_t, Q = sum_t M2_t and P = sum_t s_t^2 / n_t,
// sum_t n_t (mean_t - mean)^2 = P - S^2 / count, so one pass gives every term: chunk partials (S, Q, P)
// in fp64 over CHUNK rows per workgroup (4 row lanes x 64 channels, lanes added in order), then one
// thread per channel adds the chunks in order (deterministic) and finalizes as bn_finalize_kernel.
constexpr int BNF_CHUNK = 512;
// the chunk partials' scratch (< 1 MB at 200k rows): one buffer per (device, stream), kept and grown on
// demand (a stream's finalize calls are ordered on it; hipMallocAsync / hipFreeAsync per call measured
// ~2 ms per step of allocator traffic in the bf16 ensemble step).  The device is part of the key: the
// default stream is handle 0 on every device.
static double* bn_chunk_scratch(hipStream_t s, size_t bytes) {
  static std::mutex mu;
  static std::vector<std::pair<std::pair<int, hipStream_t>, std::pair<void*, size_t>>> bufs;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { set_error("bn finalize: no current device", __FILE__, __LINE__); return nullptr; }
  const std::pair<int, hipStream_t> key{dev, s};
  const std::lock_guard<std::mutex> lk(mu);
  for (auto& b : bufs)
    if (b.first == key) {
      if (b.second.second >= bytes) return static_cast<double*>(b.second.first);
      if (hipStreamSynchronize(s) != hipSuccess || hipFree(b.second.first) != hipSuccess) {
        set_error("bn finalize: scratch release failed", __FILE__, __LINE__);
        return nullptr;
      }
      b.second = {nullptr, 0};
      if (hipMalloc(&b.second.first, bytes) != hipSuccess) {
        set_error("bn finalize: scratch allocation failed", __FILE__, __LINE__);
        return nullptr;
      }
      b.second.second = bytes;
      return static_cast<double*>(b.second.first);
    }
  void* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) {
    set_error("bn finalize: scratch allocation failed", __FILE__, __LINE__);
    return nullptr;
  }
  bufs.push_back({key, {p, bytes}});
  return static_cast<double*>(p);
}
__global__ __launch_bounds__(256) void bn_chan_chunks_kernel(const float* __restrict__ stats, int rows, int64_t count,
                                                             int C, int chan_rows, double* __restrict__ part) {
  __shared__ double sh[3][4][64];
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int c = blockIdx.y * 64 + cl;
  const int r0 = blockIdx.x * BNF_CHUNK, r1 = min(rows, r0 + BNF_CHUNK);
  double S = 0.0, Q = 0.0, P = 0.0;
  if (c < C)
    for (int r = r0 + rl; r < r1; r += 4) {
      const int64_t left = count - (int64_t)r * chan_rows, nt = left < chan_rows ? left : chan_rows;
      const double st = stats[((int64_t)r * 2 + 0) * C + c];
      S += st;
      Q += (double)stats[((int64_t)r * 2 + 1) * C + c];
      P += st * st / (double)nt;
    }
  sh[0][rl][cl] = S;
  sh[1][rl][cl] = Q;
  sh[2][rl][cl] = P;
  __syncthreads();
  if (rl == 0 && c < C) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double v = ((sh[k][0][cl] + sh[k][1][cl]) + sh[k][2][cl]) + sh[k][3][cl];
      part[((int64_t)blockIdx.x * 3 + k) * C + c] = v;
    }
  }
}
__global__ void bn_chan_final_kernel(const double* __restrict__ part, int nchunks, int64_t count, int C,
                                     const float* __restrict__ gamma, const float* __restrict__ beta, float* run_mean,
                                     float* run_var, float momentum, float eps, float* mean, float* invstd,
                                     float* scale, float* shift) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double S = 0.0, Q = 0.0, P = 0.0;
  for (int k = 0; k < nchunks; ++k) {
    S += part[((int64_t)k * 3 + 0) * C + c];
    Q += part[((int64_t)k * 3 + 1) * C + c];
    P += part[((int64_t)k * 3 + 2) * C + c];
  }
  const double m = S / (double)count;
  double between = P - S * m;
  if (between < 0.0) between = 0.0;
  double var = (Q + between) / (double)count;
  if (var < 0.0) var = 0.0;
  const bool run = run_mean != nullptr;
  const BnFwdCoef o = bn_fwd_epilogue(m, var, count, gamma[c], beta[c], run ? run_mean[c] : 0.f,
                                      run ? run_var[c] : 0.f, momentum, eps, 1, run);
  if (run) { run_mean[c] = o.rm; run_var[c] = o.rv; }
  mean[c] = o.mu;
  invstd[c] = o.is;
  scale[c] = o.sc;
  shift[c] = o.sh;
}

int launch_bn_finalize(hipStream_t s, const float* stats, int rows, int64_t count, int C, const float* gamma,
                       const float* beta, float* run_mean, float* run_var, float momentum, float eps, bool training,
                       float* mean, float* invstd, float* scale, float* shift, int chan_rows) {
  if (training && chan_rows > 0 && rows > 4 * BNF_CHUNK) {
    const int nch = cdiv(rows, BNF_CHUNK);
    double* part = bn_chunk_scratch(s, sizeof(double) * (size_t)nch * 3 * C);
    if (!part) return -1;
    hipLaunchKernelGGL(bn_chan_chunks_kernel, dim3((unsigned)nch, (unsigned)cdiv(C, 64)), dim3(256), 0, s, stats, rows,
                       count, C, chan_rows, part);
    DFD_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(bn_chan_final_kernel, dim3((unsigned)cdiv(C, 256)), dim3(256), 0, s, part, nch, count, C, gamma,
                       beta, run_mean, run_var, momentum, eps, mean, invstd, scale, shift);
    DFD_HIP_CHECK(hipGetLastError());
    return 0;
  }
  const int ch = training ? fin_ch(rows) : 16;
#define DFD_FIN(CH)                                                                                                 \
  hipLaunchKernelGGL((bn_finalize_kernel<CH>), dim3(cdiv(C, CH)), dim3(1024), 0, s, stats, rows, count, C, gamma, beta, \
                     run_mean, run_var, momentum, eps, training ? 1 : 0, mean, invstd, scale, shift, chan_rows)
  if (ch == 16) DFD_FIN(16);
  else if (ch == 8) DFD_FIN(8);
  else DFD_FIN(4);
#undef DFD_FIN
  DFD_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_bn_finalize_fin(hipStream_t s, const BnFwdFin& f, int C) {
  return launch_bn_finalize(s, f.stats, f.rows, f.count, C, f.gamma, f.beta, f.run_mean, f.run_var, f.momentum, f.eps,
                            true, f.mean, f.invstd, f.scale, f.shift);
}

// Eval mode: every BatchNorm of a plan from its running statistics in ONE launch (workgroup = layer):
// the same operations as bn_finalize_kernel's eval branch; one ~5 us launch instead of 49 per forward
__global__ __launch_bounds__(256) void bn_eval_all_kernel(const float* __restrict__ P, const float* __restrict__ bnb,
                                                          float* __restrict__ wsf, EvalBnTable t, float eps) {
  const EvalBnEntry e = t.e[blockIdx.x];
  for (int c = threadIdx.x; c < e.C; c += 256) {
    const float mu = bnb[e.rm + c];
    const float is = 1.0f / sqrtf(bnb[e.rv + c] + eps);
    const float sc = P[e.w + c] * is;
    wsf[e.mean + c] = mu;
    wsf[e.invstd + c] = is;
    wsf[e.scale + c] = sc;
    wsf[e.shift + c] = P[e.b + c] - mu * sc;
  }
}

int launch_bn_eval_all(hipStream_t s, const float* P, const float* bnb, float* wsf, const EvalBnTable& t, float eps) {
  if (t.n <= 0 || t.n > kEvalBnMax) { set_error("bn eval: table size", __FILE__, __LINE__); return -1; }
  hipLaunchKernelGGL(bn_eval_all_kernel, dim3(t.n), dim3(256), 0, s, P, bnb, wsf, t, eps);
  DFD_HIP_CHECK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ elementwise grid
// "Channel-stationary" grid-stride: the launch uses a block count whose thread total is a
// multiple of the row width cv (in 8-vectors), so a thread's channel vector -- and every
// per-channel coefficient it needs -- is loop-invariant and the loop has no division.
static int gcd_int(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }
static int cs_grid(int64_t nvec, int cv) {
  const int unit = cv / gcd_int(cv, 256);
  const int64_t want = std::max<int64_t>(1, std::min<int64_t>(cdiv64(nvec, 256), 4096));
  return (int)std::max<int64_t>(unit, (want / unit) * unit);
}

// ------------------------------------------------------------------ BN apply (+ residual)
template <typename T, bool RES>
__global__ __launch_bounds__(256) void bn_apply_kernel(const T* __restrict__ Y, const float* __restrict__ scale,
                                                       const float* __restrict__ shift, const T* __restrict__ R,
                                                       T* __restrict__ X, int64_t nvec, int cv) {
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nvec) return;
  const int64_t step = (int64_t)gridDim.x * 256;  // multiple of cv (cs_grid)
  const int c = (int)(i % cv) * 8;
  float sc[8], sh[8];
  ld8f(scale + c, sc);
  ld8f(shift + c, sh);
  for (; i < nvec; i += step) {
    float y[8];
    ld8(Y + i * 8, y);
    if constexpr (RES) {
      float r[8];
      ld8(R + i * 8, r);
#pragma unroll
      for (int j = 0; j < 8; ++j) y[j] = y[j] * sc[j] + sh[j] + r[j];
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) y[j] = y[j] * sc[j] + sh[j];
    }
    st8(X + i * 8, y);
  }
}

template <typename T>
int launch_bn_apply(hipStream_t s, const T* Y, const float* scale, const float* shift, const T* R, T* X, int64_t M,
                    int C) {
  const int64_t nvec = M * C / 8;
  const int gx = cs_grid(nvec, C / 8);
  if (R)
    hipLaunchKernelGGL((bn_apply_kernel<T, true>), dim3(gx), dim3(256), 0, s, Y, scale, shift, R, X, nvec, C / 8);
  else
    hipLaunchKernelGGL((bn_apply_kernel<T, false>), dim3(gx), dim3(256), 0, s, Y, scale, shift, R, X, nvec, C / 8);
  DFD_HIP_CHECK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ BN backward
// g = dA * act'(z),  z = y*scale + shift,  dA = dZ*gate + bc*bc_scale
// FL: compile-time presence flags of the optional inputs (one kernel instance per combination)
enum { BF_DZ = 1, BF_GATE = 2, BF_BC = 4, BF_SILU = 8 };
static int bn_flags(const BnBwdIn& in) {
  return (in.dZ ? BF_DZ : 0) | (in.gate ? BF_GATE : 0) | (in.bc ? BF_BC : 0) | (in.silu ? BF_SILU : 0);
}

// per-thread channel constants of the backward
struct BnBwdCh {
  float sc[8], sh[8];
};

template <typename T, int FL>
__device__ __forceinline__ void bn_bwd_g8(const BnBwdIn& in, const T* __restrict__ Y, int64_t row, uint32_t frame,
                                          int c, int C, const BnBwdCh& ch, float (&g)[8], float (&y)[8]) {
  ld8(Y + row * C + c, y);
  float da[8];
  if constexpr ((FL & BF_DZ) != 0) {
    ld8(reinterpret_cast<const T*>(in.dZ) + row * C + c, da);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) da[j] = 0.f;
  }
  if constexpr ((FL & BF_GATE) != 0) {
    float gt[8];
    ld8f(in.gate + (int64_t)frame * C + c, gt);
#pragma unroll
    for (int j = 0; j < 8; ++j) da[j] *= gt[j];
  }
  if constexpr ((FL & BF_BC) != 0) {
    float b[8];
    ld8f(in.bc + (int64_t)frame * C + c, b);
#pragma unroll
    for (int j = 0; j < 8; ++j) da[j] += b[j] * in.bc_scale;
  }
  if constexpr ((FL & BF_SILU) != 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) g[j] = da[j] * dsiluf_(y[j] * ch.sc[j] + ch.sh[j]);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) g[j] = da[j];
  }
}

template <int FL>
__device__ __forceinline__ void bn_bwd_ch(const BnBwdIn& in, int c, BnBwdCh& ch) {
  if constexpr ((FL & BF_SILU) != 0) {
    ld8f(in.scale + c, ch.sc);
    ld8f(in.shift + c, ch.sh);
  }
}

template <int FL>
__device__ __forceinline__ uint32_t bn_frame(const BnBwdIn& in, int64_t row) {
  if constexpr ((FL & (BF_GATE | BF_BC)) != 0) return (uint32_t)row / (uint32_t)in.rows_per_frame;
  return 0u;
}

// grid (gx, cdiv(C/8, VPG)); threads: vec = tid % vpg, rl = tid / vpg
template <typename T, int FL>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(BnBwdIn in, const T* __restrict__ Y, int64_t M, int C,
                                                            float* __restrict__ stats, int vpg) {
  __shared__ float sh[2][256][8];
  const int tid = threadIdx.x;
  const int vec = tid % vpg, rl = tid / vpg, nrl = 256 / vpg;
  const int c = (blockIdx.y * vpg + vec) * 8;
  float as[8], aq[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { as[j] = 0.f; aq[j] = 0.f; }
  if (rl < nrl && c < C) {
    float mu[8], is[8];
    BnBwdCh ch;
    bn_bwd_ch<FL>(in, c, ch);
    ld8f(in.mean + c, mu);
    ld8f(in.invstd + c, is);
    // rows in pairs (both rows' loads issued before either is summed; same summation order)
    const int64_t rs = (int64_t)gridDim.x * nrl;
    int64_t r = (int64_t)blockIdx.x * nrl + rl;
    for (; r < M; r += 2 * rs) {
      float g[2][8], y[2][8];
      const bool two = r + rs < M;
      bn_bwd_g8<T, FL>(in, Y, r, bn_frame<FL>(in, r), c, C, ch, g[0], y[0]);
      if (two) bn_bwd_g8<T, FL>(in, Y, r + rs, bn_frame<FL>(in, r + rs), c, C, ch, g[1], y[1]);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (u == 1 && !two) break;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          as[j] += g[u][j];
          aq[j] += g[u][j] * (y[u][j] - mu[j]) * is[j];
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) { sh[0][tid][j] = as[j]; sh[1][tid][j] = aq[j]; }
  __syncthreads();
  if (tid < vpg && c < C) {
    for (int r = 1; r < nrl; ++r) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        as[j] += sh[0][r * vpg + tid][j];
        aq[j] += sh[1][r * vpg + tid][j];
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      stats[((int64_t)blockIdx.x * 2 + 0) * C + c + j] = as[j];
      stats[((int64_t)blockIdx.x * 2 + 1) * C + c + j] = aq[j];
    }
  }
}

template <typename T>
int launch_bn_bwd_reduce(hipStream_t s, const BnBwdIn& in, const T* Y, int64_t M, int C, float* stats, int* stat_rows,
                         int max_rows) {
  if (M > (int64_t)UINT32_MAX) { set_error("bn: more than 2^32 rows", __FILE__, __LINE__); return -1; }
  int vpg, groups;
  bn_vpg_groups(C, vpg, groups);
  const int nrl = 256 / vpg;
  const int64_t rows_needed = cdiv64(M, nrl * 4);
  int gx = (int)std::max<int64_t>(1, std::min<int64_t>(rows_needed, std::max(1, 1024 / groups)));
  if (max_rows > 0) gx = std::min(gx, max_rows);
  switch (bn_flags(in)) {
#define DFD_BNR(F) case F: hipLaunchKernelGGL((bn_bwd_reduce_kernel<T, F>), dim3(gx, groups), dim3(256), 0, s, in, Y, M, C, stats, vpg); break;
    DFD_BNR(0) DFD_BNR(1) DFD_BNR(2) DFD_BNR(3) DFD_BNR(4) DFD_BNR(5) DFD_BNR(6) DFD_BNR(7)
    DFD_BNR(8) DFD_BNR(9) DFD_BNR(10) DFD_BNR(11) DFD_BNR(12) DFD_BNR(13) DFD_BNR(14) DFD_BNR(15)
#undef DFD_BNR
  }
  DFD_HIP_CHECK(hipGetLastError());
  *stat_rows = gx;
  return 0;
}

template <int FIN_CH>
__global__ __launch_bounds__(1024) void bn_bwd_finalize_kernel(const float* __restrict__ stats, int rows, int64_t count,
                                                              int C, const float* __restrict__ gamma,
                                                              const float* __restrict__ mean,
                                                              const float* __restrict__ invstd, int training,
                                                              float* dgamma, float* dbeta, int accumulate,
                                                              float* coef, int centred) {
  __shared__ double sh_s[1024 / 64 * FIN_CH], sh_q[1024 / 64 * FIN_CH];
  const int tid = threadIdx.x;
  const int c = blockIdx.x * FIN_CH + tid;
  // per-channel operands loaded before the reduction (see bn_finalize_kernel)
  float p_g = 0.f, p_is = 0.f, p_mu = 0.f, p_db = 0.f, p_dg = 0.f;
  if (tid < FIN_CH && c < C) {
    p_g = gamma[c];
    p_is = invstd[c];
    if (!centred) p_mu = mean[c];
    if (accumulate) { p_db = dbeta[c]; p_dg = dgamma[c]; }
  }
  double s = 0.0, q = 0.0;
  reduce_stat_rows<FIN_CH>(stats, rows, C, s, q, sh_s, sh_q);
  if (tid < FIN_CH && c < C) {
    const BnBwdCoef o = bn_bwd_epilogue(s, q, p_g, p_is, p_mu, count, training, centred);
    if (accumulate) { dbeta[c] = p_db + o.db; dgamma[c] = p_dg + o.dg; }
    else { dbeta[c] = o.db; dgamma[c] = o.dg; }
    coef[c] = o.k1;
    coef[C + c] = o.k2;
    coef[2 * C + c] = o.k3;
  }
}

int launch_bn_bwd_finalize(hipStream_t s, const float* stats, int rows, int64_t count, int C, const float* gamma,
                           const float* mean, const float* invstd, bool training, float* dgamma, float* dbeta,
                           bool accumulate, float* coef, bool centred) {
#define DFD_FIN(CH)                                                                                                \
  hipLaunchKernelGGL((bn_bwd_finalize_kernel<CH>), dim3(cdiv(C, CH)), dim3(1024), 0, s, stats, rows, count, C, gamma, \
                     mean, invstd, training ? 1 : 0, dgamma, dbeta, accumulate ? 1 : 0, coef, centred ? 1 : 0)
  const int ch = fin_ch(rows);
  if (ch == 16) DFD_FIN(16);
  else if (ch == 8) DFD_FIN(8);
  else DFD_FIN(4);
#undef DFD_FIN
  DFD_HIP_CHECK(hipGetLastError());
  return 0;
}

template <typename T, int FL>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(BnBwdIn in, const T* __restrict__ Y,
                                                           const float* __restrict__ coef, T* dY, int64_t nvec, int C) {
  const int cv = C / 8;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nvec) return;
  const int64_t step = (int64_t)gridDim.x * 256;  // multiple of cv (cs_grid)
  const int64_t rstep = step / cv;
  int64_t row = i / cv;
  const int c = (int)(i - row * cv) * 8;
  float k1[8], k2[8], k3[8];
  BnBwdCh ch;
  bn_bwd_ch<FL>(in, c, ch);
  ld8f(coef + c, k1);
  ld8f(coef + C + c, k2);
  ld8f(coef + 2 * C + c, k3);
  for (; i < nvec; i += step, row += rstep) {
    float g[8], y[8];
    bn_bwd_g8<T, FL>(in, Y, row, bn_frame<FL>(in, row), c, C, ch, g, y);
#pragma unroll
    for (int j = 0; j < 8; ++j) g[j] = k1[j] * g[j] + k2[j] * y[j] + k3[j];
    st8(dY + i * 8, g);
  }
}

template <typename T>
int launch_bn_bwd_apply(hipStream_t s, const BnBwdIn& in, const T* Y, const float* coef, T* dY, int64_t M, int C) {
  if (M > (int64_t)UINT32_MAX) { set_error("bn: more than 2^32 rows", __FILE__, __LINE__); return -1; }
  const int64_t nvec = M * C / 8;
  const int gx = cs_grid(nvec, C / 8);
  switch (bn_flags(in)) {
#define DFD_BNA(F) case F: hipLaunchKernelGGL((bn_bwd_apply_kernel<T, F>), dim3(gx), dim3(256), 0, s, in, Y, coef, dY, nvec, C); break;
    DFD_BNA(0) DFD_BNA(1) DFD_BNA(2) DFD_BNA(3) DFD_BNA(4) DFD_BNA(5) DFD_BNA(6) DFD_BNA(7)
    DFD_BNA(8) DFD_BNA(9) DFD_BNA(10) DFD_BNA(11) DFD_BNA(12) DFD_BNA(13) DFD_BNA(14) DFD_BNA(15)
#undef DFD_BNA
  }
  DFD_HIP_CHECK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ BN backward finalize + apply
// The finalize (bn_bwd_finalize_kernel) and the apply pass in ONE launch where the producer wrote few
// stat rows: every workgroup owns 64 channels and a chunk of rows; it first reduces the stat rows of
// its channels (16 row lanes x 16 float4 columns, fp64, lanes added in a fixed order -- the same k1..k3
// in every workgroup of the channel group), the row-chunk-0 workgroup also stores dbeta / dgamma /
// coef, then it applies dY = k1*g + k2*y + k3 over its rows.  Saves the ~5 us finalize launch per BN
// backward; the reduction costs each workgroup rows / 16 x 2 loads per thread (used for rows <= 256).
constexpr int BAF_CH = 64, BAF_RL = 16, BAF_ROWS_MAX = 256;
constexpr int64_t BAF_M_MAX = 16384;
struct BnFinArgs {
  int64_t count;
  const float *gamma, *mean, *invstd;
  int training, accumulate;
  float *dgamma, *dbeta, *coef;
};

template <typename T, int FL>
__global__ __launch_bounds__(256) void bn_bwd_apply_fin_kernel(BnBwdIn in, const T* __restrict__ Y, int64_t M, int C,
                                                               const float* __restrict__ stats, int rows, BnFinArgs fa,
                                                               T* dY, int64_t rows_per_wg) {
  __shared__ double sh[2][BAF_RL][BAF_CH];
  __shared__ float kc[3][BAF_CH];
  const int tid = threadIdx.x;
  const int c0 = blockIdx.y * BAF_CH;
  const int nch = min(BAF_CH, C - c0);
  {
    const int c4 = tid & 15, rl = tid >> 4;
    const int c = c0 + 4 * c4;
    double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
    if (4 * c4 < nch) {
      int r = rl;
      for (; r + 7 * BAF_RL < rows; r += 8 * BAF_RL) {  // 16 loads in flight, added in row order
        float4 vs[8], vq[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          vs[u] = *reinterpret_cast<const float4*>(stats + ((int64_t)(r + u * BAF_RL) * 2 + 0) * C + c);
          vq[u] = *reinterpret_cast<const float4*>(stats + ((int64_t)(r + u * BAF_RL) * 2 + 1) * C + c);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          s[0] += vs[u].x; s[1] += vs[u].y; s[2] += vs[u].z; s[3] += vs[u].w;
          q[0] += vq[u].x; q[1] += vq[u].y; q[2] += vq[u].z; q[3] += vq[u].w;
        }
      }
      for (; r < rows; r += BAF_RL) {
        const float4 vs = *reinterpret_cast<const float4*>(stats + ((int64_t)r * 2 + 0) * C + c);
        const float4 vq = *reinterpret_cast<const float4*>(stats + ((int64_t)r * 2 + 1) * C + c);
        s[0] += vs.x; s[1] += vs.y; s[2] += vs.z; s[3] += vs.w;
        q[0] += vq.x; q[1] += vq.y; q[2] += vq.z; q[3] += vq.w;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      sh[0][rl][4 * c4 + j] = s[j];
      sh[1][rl][4 * c4 + j] = q[j];
    }
  }
  __syncthreads();
  if (tid < nch) {
    double s = 0.0, q = 0.0;
#pragma unroll
    for (int l = 0; l < BAF_RL; ++l) { s += sh[0][l][tid]; q += sh[1][l][tid]; }
    const int c = c0 + tid;
    const BnBwdCoef o =
        bn_bwd_epilogue(s, q, fa.gamma[c], fa.invstd[c], fa.training ? fa.mean[c] : 0.f, fa.count, fa.training, 0);
    kc[0][tid] = o.k1;
    kc[1][tid] = o.k2;
    kc[2][tid] = o.k3;
    if (blockIdx.x == 0) {
      fa.dbeta[c] = fa.accumulate ? fa.dbeta[c] + o.db : o.db;
      fa.dgamma[c] = fa.accumulate ? fa.dgamma[c] + o.dg : o.dg;
      if (fa.coef) {
        fa.coef[c] = o.k1;
        fa.coef[C + c] = o.k2;
        fa.coef[2 * C + c] = o.k3;
      }
    }
  }
  __syncthreads();
  // apply: 8 channel vectors x 32 row lanes, two rows' loads in flight
  const int v = tid & 7, rl = tid >> 3;
  const int cl = 8 * v, c = c0 + cl;
  if (cl >= nch) return;
  float k1[8], k2[8], k3[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { k1[j] = kc[0][cl + j]; k2[j] = kc[1][cl + j]; k3[j] = kc[2][cl + j]; }
  BnBwdCh ch;
  bn_bwd_ch<FL>(in, c, ch);
  const int64_t rb = (int64_t)blockIdx.x * rows_per_wg, re = min(M, rb + rows_per_wg);
  int64_t row = rb + rl;
  for (; row + 32 < re; row += 64) {
    float g[2][8], y[2][8];
    bn_bwd_g8<T, FL>(in, Y, row, bn_frame<FL>(in, row), c, C, ch, g[0], y[0]);
    bn_bwd_g8<T, FL>(in, Y, row + 32, bn_frame<FL>(in, row + 32), c, C, ch, g[1], y[1]);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
#pragma unroll
      for (int j = 0; j < 8; ++j) g[u][j] = k1[j] * g[u][j] + k2[j] * y[u][j] + k3[j];
      st8(dY + (row + 32 * u) * C + c, g[u]);
    }
  }
  if (row < re) {
    float g[8], y[8];
    bn_bwd_g8<T, FL>(in, Y, row, bn_frame<FL>(in, row), c, C, ch, g, y);
#pragma unroll
    for (int j = 0; j < 8; ++j) g[j] = k1[j] * g[j] + k2[j] * y[j] + k3[j];
    st8(dY + row * C + c, g);
  }
}

// 1: launched; 0: not covered (too many stat rows, or C % 8): the caller runs finalize + apply
template <typename T>
int launch_bn_bwd_apply_fin(hipStream_t s, const BnBwdIn& in, const T* Y, int64_t M, int C, const float* stats, int rows,
                            int64_t count, const float* gamma, const float* mean, const float* invstd, bool training,
                            float* dgamma, float* dbeta, bool accumulate, float* coef, T* dY) {
  // the small late-stage tensors only: at 50,176 rows x 480-672 channels the fused pass measured
  // 45 us against 30 + 5 us for apply + finalize (trace r05 C) -- its channel-group-major grid streams
  // worse than the channel-stationary apply, which the saved launch repays only on short passes
  if (rows < 1 || rows > BAF_ROWS_MAX || (C & 7) || M <= 0 || M > BAF_M_MAX) return 0;
  if (M > (int64_t)UINT32_MAX) { set_error("bn: more than 2^32 rows", __FILE__, __LINE__); return -1; }
  const int G = cdiv(C, BAF_CH);
  // >= 128 rows per workgroup (4 per row lane), <= ~2048 workgroups
  const int64_t rc = std::max<int64_t>(1, std::min<int64_t>(cdiv64(M, 128), std::max(1, 2048 / G)));
  const int64_t rpw = cdiv64(M, rc);
  const BnFinArgs fa{count, gamma, mean, invstd, training ? 1 : 0, accumulate ? 1 : 0, dgamma, dbeta, coef};
  const dim3 grid((unsigned)cdiv64(M, rpw), (unsigned)G);
  switch (bn_flags(in)) {
#define DFD_BAF(F) case F: hipLaunchKernelGGL((bn_bwd_apply_fin_kernel<T, F>), grid, dim3(256), 0, s, in, Y, M, C, stats, rows, fa, dY, rpw); break;
    DFD_BAF(0) DFD_BAF(1) DFD_BAF(2) DFD_BAF(3) DFD_BAF(4) DFD_BAF(5) DFD_BAF(6) DFD_BAF(7)
    DFD_BAF(8) DFD_BAF(9) DFD_BAF(10) DFD_BAF(11) DFD_BAF(12) DFD_BAF(13) DFD_BAF(14) DFD_BAF(15)
#undef DFD_BAF
  }
  DFD_HIP_CHECK(hipGetLastError());
  return 1;
}

#define DFD_BN_INST(T)                                                                                               \
  template int launch_bn_apply<T>(hipStream_t, const T*, const float*, const float*, const T*, T*, int64_t, int);    \
  template int launch_bn_bwd_reduce<T>(hipStream_t, const BnBwdIn&, const T*, int64_t, int, float*, int*, int);     \
  template int launch_bn_bwd_apply<T>(hipStream_t, const BnBwdIn&, const T*, const float*, T*, int64_t, int);       \
  template int launch_bn_bwd_apply_fin<T>(hipStream_t, const BnBwdIn&, const T*, int64_t, int, const float*, int,  \
                                          int64_t, const float*, const float*, const float*, bool, float*, float*, \
                                          bool, float*, T*);
DFD_BN_INST(float)
DFD_BN_INST(bf16)
DFD_BN_INST(f16)
#undef DFD_BN_INST

}  // namespace dfd
