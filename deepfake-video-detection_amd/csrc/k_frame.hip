// Per-frame reductions of the EfficientNet-B0 hot path on gfx950: the SE squeeze, the global average
// pool and the one-pass SE + BN backward sums with their finalize, and the conv_pw BN-fold helpers
// (bn_fold_pw, pw_wgrad_bn_combine, col_sums).
//
// Replaces the SE module's mean(2,3) and adaptive_avg_pool2d+flatten reached from
// src/pretrained_detector.py:116, forward and backward (the excitation itself is k_se.hip).
#include "kernels.h"

namespace dfd {

static int ew_grid(int64_t nvec) { return (int)std::max<int64_t>(1, std::min<int64_t>(cdiv64(nvec, 256), 4096)); }

// ------------------------------------------------------------------ per-frame channel sums
// part[q][h][f][c] = sum over pixel chunk h of frame f of val_q(p, c), for the per-frame reductions
// of the SE module (one kernel, OP selects the values):
//   FR_SQUEEZE (Q = 1): silu(y*scale+shift); with s_out the activation is also stored (rounded to
//                       T): the late-stage conv_pwl forward and weight gradient read it instead of
//                       recomputing it per N tile
//   FR_SEBN    (Q = 5): the one-pass SE + BN backward sums D, P1..P4 (below)
// Work split: vpg 8-channel vectors x npl = 256/vpg pixel lanes per workgroup, the lanes being fpb
// frames x pl lanes per frame.  Small maps (7x7: 49 pixels) put several frames in one workgroup so a
// lane still walks ~8 pixels (one frame per workgroup left 3 pixels per lane and a workgroup's
// launch and reduction dominated); large maps split a frame into hsplit chunks.  A lane's pixels go
// in groups of FR_U (4; 2 for the register-heavy FR_SEBN) with every load of a group issued first; the pl lanes of a frame are added in
// lane order through LDS (fixed summation order: bit-reproducible).
enum { FR_SQUEEZE = 0, FR_SEBN = 2 };
struct FrGeom {
  int frames, HW, C, hsplit, vpg, pl, fpb;
};
struct FrCoef {
  const float *scale, *shift, *mean, *invstd;
};

// FIN (squeeze only): the BN's train-mode finalize from its producer's stat rows inside the launch
// (bnfin.h): every workgroup reduces the rows of its channel slice; blockIdx.x == 0 stores the
// constants and the running statistics
template <typename T, int OP, bool FIN = false>
__global__ __launch_bounds__(256) void frame_reduce_kernel(const T* __restrict__ dZ, const T* __restrict__ Y, FrCoef cf,
                                                           FrGeom g, float* __restrict__ part, T* __restrict__ s_out,
                                                           BnFwdFin fin) {
  constexpr int Q = OP == FR_SEBN ? 5 : 1;
  constexpr int FR_U = OP == FR_SEBN ? 2 : 4;  // the five FR_SEBN sums: 2 pixels in flight (occupancy)
  __shared__ float sh[Q][256][8];
  __shared__ double fscr[FIN ? kBnFinScratch : 1];
  __shared__ float fss[2][FIN ? 128 : 1];
  const int tid = threadIdx.x;
  const int vec = tid % g.vpg, l = tid / g.vpg;
  const int fi = l / g.pl, li = l - fi * g.pl;
  const int f = (blockIdx.x / g.hsplit) * g.fpb + fi, h = blockIdx.x % g.hsplit;
  const int c = (blockIdx.y * g.vpg + vec) * 8;
  const int cw0 = blockIdx.y * g.vpg * 8;  // this workgroup's channel slice
  if constexpr (FIN) {
    const int ncw = g.C - cw0 < g.vpg * 8 ? g.C - cw0 : g.vpg * 8;
    bn_fin_wg(fin, g.C, cw0, ncw, blockIdx.x == 0, fss[0], fss[1], fscr);
  }
  const bool act = fi < g.fpb && f < g.frames && c < g.C;
  const int chunk = (g.HW + g.hsplit - 1) / g.hsplit;
  const int p0 = h * chunk, p1 = min(g.HW, p0 + chunk);
  float acc[Q][8];
#pragma unroll
  for (int q = 0; q < Q; ++q)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[q][j] = 0.f;
  if (act) {
    float sc[8], shf[8], mu[8], is[8];
    if constexpr (FIN) {
#pragma unroll
      for (int j = 0; j < 8; ++j) { sc[j] = fss[0][c - cw0 + j]; shf[j] = fss[1][c - cw0 + j]; }
    } else {
      ld8f(cf.scale + c, sc);
      ld8f(cf.shift + c, shf);
    }
    if constexpr (OP == FR_SEBN) {
      ld8f(cf.mean + c, mu);
      ld8f(cf.invstd + c, is);
    }
    const int64_t fbase = (int64_t)f * g.HW;
    auto one = [&](int64_t row, float (&y)[8], const float (&d)[8]) {
      if constexpr (OP == FR_SEBN) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float z = y[j] * sc[j] + shf[j];
          const float sg = sigmoidf_(z);
          const float sp = sg * (1.0f + z * (1.0f - sg));
          const float xh = (y[j] - mu[j]) * is[j];
          const float dsp = d[j] * sp;
          acc[0][j] += d[j] * (z * sg);
          acc[1][j] += dsp;
          acc[2 % Q][j] += sp;
          acc[3 % Q][j] += dsp * xh;
          acc[4 % Q][j] += sp * xh;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) y[j] = siluf_(y[j] * sc[j] + shf[j]);
        if (s_out) st8(s_out + row * g.C + c, y);
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[0][j] += y[j];
      }
    };
    int p = p0 + li;
    for (; p + (FR_U - 1) * g.pl < p1; p += FR_U * g.pl) {
      float y[FR_U][8], d[FR_U][8];
#pragma unroll
      for (int u = 0; u < FR_U; ++u) {
        const int64_t row = fbase + p + u * g.pl;
        ld8(Y + row * g.C + c, y[u]);
        if constexpr (OP != FR_SQUEEZE) ld8(dZ + row * g.C + c, d[u]);
      }
#pragma unroll
      for (int u = 0; u < FR_U; ++u) one(fbase + p + u * g.pl, y[u], d[u]);
    }
    for (; p < p1; p += g.pl) {
      const int64_t row = fbase + p;
      float y[8], d[8];
      ld8(Y + row * g.C + c, y);
      if constexpr (OP != FR_SQUEEZE) ld8(dZ + row * g.C + c, d);
      one(row, y, d);
    }
  }
#pragma unroll
  for (int q = 0; q < Q; ++q)
#pragma unroll
    for (int j = 0; j < 8; ++j) sh[q][tid][j] = acc[q][j];
  __syncthreads();
  if (act && li == 0) {
    for (int r = 1; r < g.pl; ++r) {
      const int idx = (l + r) * g.vpg + vec;
#pragma unroll
      for (int q = 0; q < Q; ++q)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[q][j] += sh[q][idx][j];
    }
    const int64_t n = (int64_t)g.frames * g.C;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      float* o = part + ((int64_t)q * g.hsplit + h) * n + (int64_t)f * g.C + c;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = acc[q][j];
    }
  }
}

template <typename T, int OP>
static int launch_frame_reduce(hipStream_t s, const T* dZ, const T* Y, const FrCoef& cf, int frames, int HW, int C,
                               float* part, int64_t part_cap, int* hsplit_out, T* s_out = nullptr,
                               const BnFwdFin* fin = nullptr) {
  constexpr int Q = OP == FR_SEBN ? 5 : 1;
  if (frames <= 0 || HW <= 0) { set_error("frame reduce: empty input", __FILE__, __LINE__); return -1; }
  if ((int64_t)Q * frames * C > part_cap) { set_error("frame reduce: partial buffer too small", __FILE__, __LINE__); return -1; }
  FrGeom g{frames, HW, C, 1, 0, 0, 1};
  int groups;
  bn_vpg_groups(C, g.vpg, groups);
  const int npl = 256 / g.vpg;
  g.fpb = std::max(1, std::min(npl, npl * 8 / HW));  // frames per workgroup: >= ~8 pixels per lane
  g.pl = npl / g.fpb;
  const int fgroups = cdiv(frames, g.fpb);
  while ((int64_t)fgroups * groups * g.hsplit < 1024 && HW / (g.hsplit * 2) >= g.pl * 8 &&
         (int64_t)Q * (g.hsplit * 2) * frames * C <= part_cap)
    g.hsplit *= 2;
  // the input BN's finalize: inside the launch where its stat rows are few (squeeze; channel slices of
  // <= 128), else its own launch first (cf.scale / cf.shift are that launch's outputs)
  const bool embed = OP == FR_SQUEEZE && fin && fin->rows > 0 && fin->rows <= kBnFinRowsMax && g.vpg * 8 <= 128;
  if (fin && fin->rows > 0 && !embed) DFD_TRY(launch_bn_finalize_fin(s, *fin, C));
  if constexpr (OP == FR_SQUEEZE) {
    if (embed) {
      hipLaunchKernelGGL((frame_reduce_kernel<T, OP, true>), dim3(fgroups * g.hsplit, groups), dim3(256), 0, s, dZ, Y,
                         cf, g, part, s_out, *fin);
      DFD_HIP_CHECK(hipGetLastError());
      *hsplit_out = g.hsplit;
      return 0;
    }
  }
    hipLaunchKernelGGL((frame_reduce_kernel<T, OP>), dim3(fgroups * g.hsplit, groups), dim3(256), 0, s, dZ, Y, cf, g,
                       part, s_out, BnFwdFin{});
  DFD_HIP_CHECK(hipGetLastError());
  *hsplit_out = g.hsplit;
  return 0;
}

// sum hsplit partials: out[f][c] = scale * sum_h part[h][f][c]
__global__ void sum_parts_kernel(const float* __restrict__ part, int hsplit, int64_t n, float scale,
                                 float* __restrict__ out) {
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    float a = 0.f;
    int h = 0;
    for (; h + 4 <= hsplit; h += 4) {  // 4 loads in flight, added in order
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = part[(h + u) * n + i];
#pragma unroll
      for (int u = 0; u < 4; ++u) a += v[u];
    }
    for (; h < hsplit; ++h) a += part[h * n + i];
    out[i] = a * scale;
  }
}

// the squeeze's per-frame partial sums part[h][f][c] (h < *hsplit); the excitation (se_chain_kernel)
// adds the partials and scales by 1/HW while loading them
template <typename T>
int launch_se_squeeze(hipStream_t s, const T* Y, const Pro& pro, int frames, int HW, int C, float* part,
                      int64_t part_cap, int* hsplit, T* s_out, const BnFwdFin* fin) {
  const FrCoef cf{pro.scale, pro.shift, nullptr, nullptr};
  return launch_frame_reduce<T, FR_SQUEEZE>(s, nullptr, Y, cf, frames, HW, C, part, part_cap, hsplit, s_out, fin);
}

// ------------------------------------------------------------------ SE + BN backward, one pass
// Backward of  out = silu(z) * gate[f][c] (feeding conv_pwl),  z = y*scale + shift (BN, batch
// stats), sq = mean_hw silu(z) (SE squeeze).  With ge = dL/dout and bc[f][c] = dL/dsq / HW the
// BN's input gradient is g = (ge*gate + bc) * silu'(z); since gate and bc are constant per
// (frame, channel), every reduction the backward needs decomposes into per-frame sums that one
// pass over (ge, y) produces before bc is known (frame_reduce_kernel<FR_SEBN>):
//   D  = sum ge*silu(z)      (-> dgate, the SE branch)
//   P1 = sum ge*silu'(z)     P2 = sum silu'(z)     P3 = sum ge*silu'(z)*xhat     P4 = sum silu'(z)*xhat
// so that  sum g = sum_f gate*P1 + bc*P2  and  sum g*xhat = sum_f gate*P3 + bc*P4.  This replaces
// the separate SE-backward reduction and BN-backward reduction (two full passes over ge and y).
template <typename T>
int launch_se_bn_bwd_reduce(hipStream_t s, const T* dZ, const T* Y, const float* scale, const float* shift,
                            const float* mean, const float* invstd, int frames, int HW, int C, float* part,
                            int64_t part_cap, int* hsplit_out) {
  const FrCoef cf{scale, shift, mean, invstd};
  return launch_frame_reduce<T, FR_SEBN>(s, dZ, Y, cf, frames, HW, C, part, part_cap, hsplit_out);
}

// BN backward finalize from the per-frame sums of frame_reduce_kernel<FR_SEBN> once bc is known:
// dbeta = sum g, dgamma = sum g*xhat, coefficients k1..k3 of dy = k1*g + k2*y + k3 (fp64).
// The sums P1..P4 are the partials part[1..4][h][f][c] of that kernel, added over h in order: chunk 0
// of each q holds the sum (hsplit == 1, or added by sum_parts4_kernel) -- plain loads, all issued up front.
// Block = 64 channels x 16 frame slices (the slices' frames unrolled by 4, all loads issued
// up front); slices added in order.
constexpr int FF_SL = 16;
// part[q][h][i] (q = 1..4) -> part[q][0][i] = sum over h in order (in place: element (q, i) is read
// and written by one thread only); the finalize then reads chunk 0 of each q
__global__ void sum_parts4_kernel(float* __restrict__ part, int hsplit, int64_t n) {
  for (int64_t i = blockIdx.x * 256 + threadIdx.x; i < 4 * n; i += (int64_t)gridDim.x * 256) {
    const int64_t q = i / n + 1, k = i - (q - 1) * n;
    float a = 0.f;
    for (int h = 0; h < hsplit; ++h) a += part[(q * hsplit + h) * n + k];
    part[q * hsplit * n + k] = a;
  }
}

__global__ __launch_bounds__(1024) void bn_bwd_finalize_frames_kernel(
    const float* __restrict__ part, int hsplit, const float* __restrict__ gate, const float* __restrict__ bc, int frames,
    int C, int64_t count, const float* __restrict__ gamma, const float* __restrict__ mean,
    const float* __restrict__ invstd, int training, float* dgamma, float* dbeta, int accumulate, float* coef) {
  __shared__ double red[2][FF_SL][64];
  const int tid = threadIdx.x, cl = tid & 63, sl = tid >> 6;
  const int c = blockIdx.x * 64 + cl;
  const int64_t n = (int64_t)frames * C;
  auto P = [&](int q, int64_t i) { return part[(int64_t)(q + 1) * hsplit * n + i]; };  // q = 0..3 -> P1..P4
  // per-channel operands loaded before the reduction (see bn_finalize_kernel)
  float p_g = 0.f, p_is = 0.f, p_mu = 0.f, p_db = 0.f, p_dg = 0.f;
  if (sl == 0 && c < C) {
    p_g = gamma[c];
    p_is = invstd[c];
    p_mu = mean[c];
    if (accumulate) { p_db = dbeta[c]; p_dg = dgamma[c]; }
  }
  double s = 0.0, q = 0.0;
  if (c < C) {
    const int per = (frames + FF_SL - 1) / FF_SL;
    const int f0 = sl * per, f1 = min(frames, f0 + per);
    int f = f0;
    for (; f + 4 <= f1; f += 4) {
      float gt[4], b[4], p1[4], p2[4], p3[4], p4[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t i = (int64_t)(f + u) * C + c;
        gt[u] = gate[i]; b[u] = bc[i];
        p1[u] = P(0, i); p2[u] = P(1, i);
        p3[u] = P(2, i); p4[u] = P(3, i);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        s += (double)gt[u] * (double)p1[u] + (double)b[u] * (double)p2[u];
        q += (double)gt[u] * (double)p3[u] + (double)b[u] * (double)p4[u];
      }
    }
    for (; f < f1; ++f) {
      const int64_t i = (int64_t)f * C + c;
      s += (double)gate[i] * (double)P(0, i) + (double)bc[i] * (double)P(1, i);
      q += (double)gate[i] * (double)P(2, i) + (double)bc[i] * (double)P(3, i);
    }
  }
  red[0][sl][cl] = s;
  red[1][sl][cl] = q;
  __syncthreads();
  if (sl == 0 && c < C) {
    s = 0.0;
    q = 0.0;
    for (int k = 0; k < FF_SL; ++k) { s += red[0][k][cl]; q += red[1][k][cl]; }
    const BnBwdCoef o = bn_bwd_epilogue(s, q, p_g, p_is, p_mu, count, training, 0);
    if (accumulate) { dbeta[c] = p_db + o.db; dgamma[c] = p_dg + o.dg; }
    else { dbeta[c] = o.db; dgamma[c] = o.dg; }
    coef[c] = o.k1;
    coef[C + c] = o.k2;
    coef[2 * C + c] = o.k3;
  }
}

int launch_bn_bwd_finalize_frames(hipStream_t s, float* part, int hsplit, const float* gate, const float* bc,
                                  int frames, int C, int64_t count, const float* gamma, const float* mean,
                                  const float* invstd, bool training, float* dgamma, float* dbeta, bool accumulate,
                                  float* coef) {
  if (hsplit > 1) {
    // the finalize has only C/64 workgroups: add the pixel-chunk partials of q = 1..4 in a parallel
    // pass first (in place into chunk 0, h ascending)
    const int64_t n = (int64_t)frames * C;
    hipLaunchKernelGGL(sum_parts4_kernel, dim3(ew_grid(4 * n)), dim3(256), 0, s, part, hsplit, n);
    DFD_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(bn_bwd_finalize_frames_kernel, dim3(cdiv(C, 64)), dim3(1024), 0, s, part, hsplit, gate, bc,
                     frames, C, count, gamma, mean, invstd, training ? 1 : 0, dgamma, dbeta, accumulate ? 1 : 0, coef);
  DFD_HIP_CHECK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ conv_pw backward through its BN
// The BN after conv_pw (no activation) has the input gradient ge1 = k1*g + k2*y1 + k3 (per output
// channel k of the conv; bn_bwd_finalize), and y1 = x . W^T is itself a linear function of the
// block input x.  By linearity the conv's gradients need g and x only -- never y1, and no
// materialised ge1 (three full passes over the 6x-expanded tensor saved):
//   dX = g . (diag(k1) W) + x . (W^T diag(k2) W) + W^T k3
//   dW = diag(k1) (g^T x) + diag(k2) W (x^T x) + k3 (1^T x)
// bn_fold_pw: W1t[c][k] = W[k][c] k1[k] (dgrad operand), Q[c][c'] = sum_k W[k][c] k2[k] W[k][c'],
// bv[c] = sum_k k3[k] W[k][c]  (W: fp32 master weights [mid][cin]; sums in fp64, k ascending).
// One workgroup per input channel c (plus one more block per 256 W1t elements): row c of Q and
// bv[c] as k-sliced dot products (4 slices of k per output, fp64, slices added in order).
template <typename T>
__global__ __launch_bounds__(256) void bn_fold_pw_kernel(const float* __restrict__ W, const float* __restrict__ coef,
                                                         int mid, int cin, T* __restrict__ w1t, T* __restrict__ q,
                                                         float* __restrict__ bv) {
  __shared__ double red[4][64];
  if ((int)blockIdx.x >= cin) {  // W1t[c][k] = W[k][c] k1[k]
    const int64_t i = (int64_t)(blockIdx.x - cin) * 256 + threadIdx.x;
    if (i < (int64_t)cin * mid) {
      const int c = (int)(i / mid), k = (int)(i - (int64_t)c * mid);
      w1t[i] = Tr<T>::from_f(W[(int64_t)k * cin + c] * coef[k]);
    }
    return;
  }
  const int c = blockIdx.x, tid = threadIdx.x, cl = tid & 63, sl = tid >> 6;
  const int per = (mid + 3) / 4, k0 = sl * per, k1 = min(mid, k0 + per);
  for (int c2b = 0; c2b <= cin; c2b += 64) {  // column cin = bv
    const int c2 = c2b + cl;
    double a = 0.0;
    if (c2 < cin) {
      for (int k = k0; k < k1; ++k) a += (double)(W[(int64_t)k * cin + c] * coef[mid + k]) * W[(int64_t)k * cin + c2];
    } else if (c2 == cin) {
      for (int k = k0; k < k1; ++k) a += (double)coef[2 * mid + k] * W[(int64_t)k * cin + c];
    }
    red[sl][cl] = a;
    __syncthreads();
    if (sl == 0 && c2 <= cin) {
      const double v = ((red[0][cl] + red[1][cl]) + red[2][cl]) + red[3][cl];
      if (c2 < cin) q[(int64_t)c * cin + c2] = Tr<T>::from_f((float)v);
      else bv[c] = (float)v;
    }
    __syncthreads();
  }
}

template <typename T>
int launch_bn_fold_pw(hipStream_t s, const float* W, const float* coef, int mid, int cin, T* w1t, T* q, float* bv) {
  const int blocks = cin + (int)cdiv64((int64_t)cin * mid, 256);
  hipLaunchKernelGGL((bn_fold_pw_kernel<T>), dim3((unsigned)blocks), dim3(256), 0, s, W, coef, mid, cin, w1t, q, bv);
  DFD_HIP_CHECK(hipGetLastError());
  return 0;
}

// dW[k][c] (+)= k1[k] Tg[k][c] + k2[k] sum_c' W[k][c'] G[c'][c] + k3[k] cs[c]: one workgroup per k,
// W row in LDS, thread c sums c' in order (fp64)
__global__ __launch_bounds__(256) void pw_wgrad_bn_combine_kernel(const float* __restrict__ Tg,
                                                                  const float* __restrict__ G,
                                                                  const float* __restrict__ cs,
                                                                  const float* __restrict__ W,
                                                                  const float* __restrict__ coef, int mid, int cin,
                                                                  float* dW, int accumulate) {
  __shared__ float wr[256];
  const int k = blockIdx.x;
  for (int i = threadIdx.x; i < cin; i += 256) wr[i] = W[(int64_t)k * cin + i];
  __syncthreads();
  for (int c = threadIdx.x; c < cin; c += 256) {
    double t = 0.0;
    for (int c2 = 0; c2 < cin; ++c2) t += (double)wr[c2] * G[(int64_t)c2 * cin + c];
    const int64_t i = (int64_t)k * cin + c;
    const double a = (double)coef[k] * Tg[i] + (double)coef[mid + k] * t + (double)coef[2 * mid + k] * cs[c];
    dW[i] = accumulate ? dW[i] + (float)a : (float)a;
  }
}

int launch_pw_wgrad_bn_combine(hipStream_t s, const float* Tg, const float* G, const float* cs, const float* W,
                               const float* coef, int mid, int cin, float* dW, bool accumulate) {
  if (cin > 256) { set_error("pw bn combine: cin > 256", __FILE__, __LINE__); return -1; }
  hipLaunchKernelGGL(pw_wgrad_bn_combine_kernel, dim3((unsigned)mid), dim3(256), 0, s, Tg, G, cs, W, coef, mid, cin,
                     dW, accumulate ? 1 : 0);
  DFD_HIP_CHECK(hipGetLastError());
  return 0;
}

// column sums of X [M][C]: part rows [gx][C] (vpg threads per row, rows strided, fixed-order
// tree over the block's row lanes), then the slab reducer
template <typename T>
__global__ __launch_bounds__(256) void col_sums_kernel(const T* __restrict__ X, int64_t M, int C, int vpg,
                                                       float* __restrict__ part) {
  __shared__ float sh[256][8];
  const int tid = threadIdx.x, vec = tid % vpg, rl = tid / vpg, nrl = 256 / vpg;
  const int c = (blockIdx.y * vpg + vec) * 8;
  float a[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) a[j] = 0.f;
  if (rl < nrl && c < C) {
    for (int64_t r = (int64_t)blockIdx.x * nrl + rl; r < M; r += (int64_t)gridDim.x * nrl) {
      float x[8];
      ld8(X + r * C + c, x);
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] += x[j];
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) sh[tid][j] = a[j];
  __syncthreads();
  if (tid < vpg && c < C) {
    for (int r = 1; r < nrl; ++r)
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] += sh[r * vpg + tid][j];
#pragma unroll
    for (int j = 0; j < 8; ++j) part[(int64_t)blockIdx.x * C + c + j] = a[j];
  }
}

template <typename T>
int launch_col_sums(hipStream_t s, const T* X, int64_t M, int C, float* part, int64_t part_cap, float* out) {
  int vpg, groups;
  bn_vpg_groups(C, vpg, groups);
  const int nrl = 256 / vpg;
  int64_t gx = std::max<int64_t>(1, std::min<int64_t>(cdiv64(M, nrl * 8), std::max(1, 1024 / groups)));
  gx = std::max<int64_t>(1, std::min<int64_t>(gx, part_cap / C));
  hipLaunchKernelGGL((col_sums_kernel<T>), dim3((unsigned)gx, groups), dim3(256), 0, s, X, M, C, vpg, part);
  DFD_HIP_CHECK(hipGetLastError());
  return launch_reduce_slabs(s, part, (int)gx, C, out, false);
}

template <typename T>
int launch_gap(hipStream_t s, const T* Y, const Pro& pro, int frames, int HW, int C, float* feat, const BnFwdFin* fin) {
  // HW is tiny (7x7 at 224^2): one partial per frame (the partial buffer is feat itself, so
  // hsplit = 1), then the means in place
  const FrCoef cf{pro.scale, pro.shift, nullptr, nullptr};
  int hs = 1;
  if (launch_frame_reduce<T, FR_SQUEEZE>(s, nullptr, Y, cf, frames, HW, C, feat, (int64_t)frames * C, &hs, nullptr,
                                         fin))
    return -1;
  const int64_t n = (int64_t)frames * C;
  hipLaunchKernelGGL(sum_parts_kernel, dim3(ew_grid(n)), dim3(256), 0, s, feat, 1, n, 1.0f / (float)HW, feat);
  DFD_HIP_CHECK(hipGetLastError());
  return 0;
}

#define DFD_FRAME_INST(T)                                                                                            \
  template int launch_se_squeeze<T>(hipStream_t, const T*, const Pro&, int, int, int, float*, int64_t, int*, T*,   \
                                    const BnFwdFin*);                                                               \
  template int launch_gap<T>(hipStream_t, const T*, const Pro&, int, int, int, float*, const BnFwdFin*);          \
  template int launch_se_bn_bwd_reduce<T>(hipStream_t, const T*, const T*, const float*, const float*, const float*, \
                                          const float*, int, int, int, float*, int64_t, int*);                 \
  template int launch_bn_fold_pw<T>(hipStream_t, const float*, const float*, int, int, T*, T*, float*);             \
  template int launch_col_sums<T>(hipStream_t, const T*, int64_t, int, float*, int64_t, float*);
DFD_FRAME_INST(float)
DFD_FRAME_INST(bf16)
DFD_FRAME_INST(f16)
#undef DFD_FRAME_INST

}  // namespace dfd
