// Train-time face-crop augmentation and the eval resize on the device: the
// transform chain of VideoFacesDataset(augment=True) (src/dataset.py:131-142) as a deterministic
// function of (frame, per-frame parameter row).  The host draws; the kernel never does.
//
//   1. crop box (i, j, h, w) + bilinear resize to (out_h, out_w): Pillow's two-pass fixed-point
//      resample (Resample.c: precompute_coeffs / normalize_coeffs_8bpc, horizontal pass first, uint8
//      intermediate), fused per output pixel: out = clip8(2^21 + sum_y ky * clip8(2^21 + sum_x kx * p)).
//      The flip is the store address of this stage.
//   2. colour jitter in the row's permutation order: ImageEnhance blends in fp32 (brightness, contrast
//      against the rounded mean of L, saturation against L) and the hue shift through Pillow's HSV.
//   3. grayscale (L on the three channels)
//   4. downscale / upscale: two more resizes of stage 1's kind through a per-frame scratch image
//   5. 3x3 Gaussian blur, reflect padding, fp32, round half to even; written straight to `out`.
//
// One workgroup per frame.  The working image (out_h x out_w x 3 uint8) and the resize coefficient
// tables live in LDS when they fit the CU's 160 KiB (a 224 x 224 frame does: 150,528 + 12,544 B), so a
// frame is read once from HBM and written once; otherwise both live in the per-frame scratch.  The
// downscaled image of stage 4 is always scratch (it is written and read back by the same CU).
// All arithmetic is integer or IEEE + - * / in fp32 / fp64; the file is built with -ffp-contract=off
// so the numpy restatement (tests/augment_helpers.py) matches bit for bit.
#include "../../include/dfd_hip.h"
#include "kernels.h"

namespace dfd {

namespace {

constexpr int AUG_NT = 1024;
constexpr int AUG_LDS_MAX = 160 * 1024;
constexpr int AUG_LDS_STATIC = 256;  // the reduction slots below

struct AugArgs {
  const uint8_t* src;
  const int32_t* pi;  // [n][DFD_AUG_PI] (device copy, head of the scratch)
  const float* pf;    // [n][DFD_AUG_PF]
  uint8_t* out;
  uint8_t* frame_scratch;  // n x frame_scratch_bytes
  int64_t frame_scratch_bytes;
  int src_h, src_w, out_h, out_w;
  int tab_ints;     // capacity of the coefficient tables of one resize
  int small_bytes;  // capacity of stage 4's downscaled image
};

__host__ __device__ inline int aug_align16(int64_t v) { return (int)((v + 15) & ~(int64_t)15); }
// ints one dimension's coefficient table can need: out x (2 + ksize), ksize = 2 ceil(max(in / out, 1)) + 1
__host__ __device__ inline int aug_tab_dim(int in, int out) { return 5 * out + 2 * (in > out ? in : out); }

// coefficient rows of one pass, Pillow's precompute_coeffs + normalize_coeffs_8bpc for the bilinear
// filter (support 1) with in0 = 0: row o = {first input index, taps, k[ksize]}
__device__ void aug_coeffs(int* tab, int in, int out, int ksize) {
  const double scale = (double)in / (double)out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * fs;
  const double ss = 1.0 / fs;
  for (int o = threadIdx.x; o < out; o += AUG_NT) {
    int* row = tab + (int64_t)o * (2 + ksize);
    const double center = ((double)o + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    const int n = xmax - xmin;
    double ww = 0.0;
    for (int x = 0; x < n; ++x) {
      double v = ((double)(x + xmin) - center + 0.5) * ss;
      if (v < 0.0) v = -v;
      ww += v < 1.0 ? 1.0 - v : 0.0;
    }
    for (int x = 0; x < n; ++x) {
      double v = ((double)(x + xmin) - center + 0.5) * ss;
      if (v < 0.0) v = -v;
      double w = v < 1.0 ? 1.0 - v : 0.0;
      if (ww != 0.0) w = w / ww;
      row[2 + x] = (int)(0.5 + w * 4194304.0);
    }
    row[0] = xmin;
    row[1] = n;
  }
}

__device__ __forceinline__ uint32_t aug_clip8(int32_t v) {
  v >>= 22;
  return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// in: (ih, iw) pixels with in_row bytes per row -> dst: (oh, ow) packed; `flip` mirrors the store.
// Ends with the workgroup in step: dst is complete and visible.
__device__ void aug_resize(const uint8_t* in, int64_t in_row, int ih, int iw, uint8_t* dst, int oh, int ow,
                           bool flip, int* tab) {
  if (ih == oh && iw == ow) {  // every coefficient row is {o, .., 1 << 22}: a copy
    for (int p = threadIdx.x; p < oh * ow; p += AUG_NT) {
      const int y = p / ow, x = p - y * ow;
      const uint8_t* s = in + y * in_row + 3 * (int64_t)x;
      uint8_t* d = dst + 3 * ((int64_t)y * ow + (flip ? ow - 1 - x : x));
      d[0] = s[0]; d[1] = s[1]; d[2] = s[2];
    }
    __syncthreads();
    return;
  }
  const double sx = (double)iw / (double)ow, sy = (double)ih / (double)oh;
  const int kx = (int)ceil(sx < 1.0 ? 1.0 : sx) * 2 + 1, ky = (int)ceil(sy < 1.0 ? 1.0 : sy) * 2 + 1;
  int* tx = tab;
  int* ty = tab + (int64_t)ow * (2 + kx);
  aug_coeffs(tx, iw, ow, kx);
  aug_coeffs(ty, ih, oh, ky);
  __syncthreads();
  for (int p = threadIdx.x; p < oh * ow; p += AUG_NT) {
    const int y = p / ow, x = p - y * ow;
    const int* rx = tx + (int64_t)x * (2 + kx);
    const int* ry = ty + (int64_t)y * (2 + ky);
    const int x0 = rx[0], nx = rx[1], y0 = ry[0], ny = ry[1];
    int32_t a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
    for (int b = 0; b < ny; ++b) {
      const uint8_t* s = in + (int64_t)(y0 + b) * in_row + 3 * (int64_t)x0;
      int32_t h0 = 1 << 21, h1 = 1 << 21, h2 = 1 << 21;
      for (int a = 0; a < nx; ++a) {
        const int32_t k = rx[2 + a];
        h0 += (int32_t)s[3 * a] * k;
        h1 += (int32_t)s[3 * a + 1] * k;
        h2 += (int32_t)s[3 * a + 2] * k;
      }
      const int32_t k = ry[2 + b];
      a0 += (int32_t)aug_clip8(h0) * k;
      a1 += (int32_t)aug_clip8(h1) * k;
      a2 += (int32_t)aug_clip8(h2) * k;
    }
    uint8_t* d = dst + 3 * ((int64_t)y * ow + (flip ? ow - 1 - x : x));
    d[0] = (uint8_t)aug_clip8(a0); d[1] = (uint8_t)aug_clip8(a1); d[2] = (uint8_t)aug_clip8(a2);
  }
  __syncthreads();
}

// Pillow's RGB -> L (Convert.c L24)
__device__ __forceinline__ uint32_t aug_luma(uint32_t r, uint32_t g, uint32_t b) {
  return (19595u * r + 38470u * g + 7471u * b + 0x8000u) >> 16;
}

// Image.blend(degenerate, image, f) on one byte (Blend.c)
__device__ __forceinline__ uint8_t aug_blend(uint32_t d, uint32_t x, float f, bool inside) {
  const float t = (float)(int)d + f * (float)((int)x - (int)d);
  if (inside) return (uint8_t)(int)t;
  return t <= 0.f ? (uint8_t)0 : (t >= 255.f ? (uint8_t)255 : (uint8_t)(int)t);
}

// C round() of a non-negative double
__device__ __forceinline__ int aug_round(double v) {
  const double r = floor(v);
  return (int)r + (v - r >= 0.5 ? 1 : 0);
}
__device__ __forceinline__ int aug_clampi(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// convert('HSV'), H += shift (uint8 wrap), convert('RGB'): Pillow's rgb2hsv_row / hsv2rgb (Convert.c)
__device__ void aug_hue(uint8_t* px, uint32_t shift) {
  const int r = px[0], g = px[1], b = px[2];
  const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
  uint32_t uh = 0, us = 0;
  const uint32_t uv = (uint32_t)maxc;
  if (minc != maxc) {
    const float cr = (float)(maxc - minc);
    const float s = cr / (float)maxc;
    const float rc = (float)(maxc - r) / cr, gc = (float)(maxc - g) / cr, bc = (float)(maxc - b) / cr;
    float h;
    if (r == maxc) h = bc - gc;
    else if (g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
    else h = (float)(4.0 + (double)gc - (double)rc);
    double t = (double)h / 6.0 + 1.0;
    t = t - floor(t);
    h = (float)t;
    uh = (uint32_t)aug_clampi((int)((double)h * 255.0));
    us = (uint32_t)aug_clampi((int)((double)s * 255.0));
  }
  uh = (uh + shift) & 0xffu;
  if (us == 0) {
    px[0] = px[1] = px[2] = (uint8_t)uv;
    return;
  }
  const double h6 = (double)(float)uh * 6.0 / 255.0;
  const int i = (int)floor(h6);
  const double f = (double)(float)(h6 - (double)(float)i);
  const double fs = (double)(float)((double)(float)us / 255.0);
  const double v = (double)(float)uv;
  const int p = aug_clampi(aug_round(v * (1.0 - fs)));
  const int q = aug_clampi(aug_round(v * (1.0 - fs * f)));
  const int t = aug_clampi(aug_round(v * (1.0 - fs * (1.0 - f))));
  const int vi = (int)uv;
  int R, G, B;
  switch (i % 6) {
    case 0: R = vi; G = t; B = p; break;
    case 1: R = q; G = vi; B = p; break;
    case 2: R = p; G = vi; B = t; break;
    case 3: R = p; G = q; B = vi; break;
    case 4: R = t; G = p; B = vi; break;
    default: R = vi; G = p; B = q; break;
  }
  px[0] = (uint8_t)R; px[1] = (uint8_t)G; px[2] = (uint8_t)B;
}

template <bool LDS>
__global__ __launch_bounds__(AUG_NT) void augment_frames_kernel(AugArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t aug_smem[];
  __shared__ unsigned long long red[AUG_NT / 64];
  __shared__ unsigned long long red_total;
  const int n = blockIdx.x, tid = threadIdx.x;
  const int32_t* pi = a.pi + (int64_t)n * DFD_AUG_PI;
  const float* pf = a.pf + (int64_t)n * DFD_AUG_PF;
  const int oh = a.out_h, ow = a.out_w, npix = oh * ow;
  const int cur_bytes = aug_align16((int64_t)npix * 3);
  uint8_t* fs = a.frame_scratch + (int64_t)n * a.frame_scratch_bytes;
  uint8_t* small = fs;
  uint8_t* cur;
  int* tab;
  if constexpr (LDS) {
    cur = aug_smem;
    tab = reinterpret_cast<int*>(aug_smem + cur_bytes);
  } else {
    tab = reinterpret_cast<int*>(fs + a.small_bytes);
    cur = fs + a.small_bytes + (int64_t)a.tab_ints * 4;
  }
  const int flags = pi[0];
  const int bi = pi[1], bj = pi[2], bh = pi[3], bw = pi[4];

  // 1 + 2: crop, resize, flip
  const int64_t src_row = (int64_t)a.src_w * 3;
  const uint8_t* box = a.src + (int64_t)n * a.src_h * src_row + bi * src_row + 3 * (int64_t)bj;
  aug_resize(box, src_row, bh, bw, cur, oh, ow, (flags & DFD_AUG_FLIP) != 0, tab);

  // 3: colour jitter.  A lane keeps to its own pixels, so only the contrast mean needs the workgroup.
  if (flags & DFD_AUG_JITTER) {
    for (int o = 0; o < 4; ++o) {
      const int op = pi[5 + o];
      if (op == 3) {
        const uint32_t shift = (uint32_t)pi[9] & 0xffu;
        for (int p = tid; p < npix; p += AUG_NT) aug_hue(cur + 3 * (int64_t)p, shift);
        continue;
      }
      const float f = pf[op];
      const bool inside = f >= 0.f && f <= 1.f;
      uint32_t mean = 0;
      if (op == 1) {
        unsigned long long sum = 0;
        for (int p = tid; p < npix; p += AUG_NT) {
          const uint8_t* px = cur + 3 * (int64_t)p;
          sum += aug_luma(px[0], px[1], px[2]);
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) sum += __shfl_xor(sum, s, 64);
        if ((tid & 63) == 0) red[tid >> 6] = sum;
        __syncthreads();
        if (tid == 0) {
          unsigned long long t = 0;
          for (int w = 0; w < AUG_NT / 64; ++w) t += red[w];
          red_total = t;
        }
        __syncthreads();
        mean = (uint32_t)(int)((double)red_total / (double)npix + 0.5);
      }
      for (int p = tid; p < npix; p += AUG_NT) {
        uint8_t* px = cur + 3 * (int64_t)p;
        const uint32_t r = px[0], g = px[1], b = px[2];
        const uint32_t d = op == 0 ? 0u : (op == 1 ? mean : aug_luma(r, g, b));
        px[0] = aug_blend(d, r, f, inside);
        px[1] = aug_blend(d, g, f, inside);
        px[2] = aug_blend(d, b, f, inside);
      }
    }
  }

  // 4: grayscale
  if (flags & DFD_AUG_GRAY) {
    for (int p = tid; p < npix; p += AUG_NT) {
      uint8_t* px = cur + 3 * (int64_t)p;
      px[0] = px[1] = px[2] = (uint8_t)aug_luma(px[0], px[1], px[2]);
    }
  }
  __syncthreads();

  // 5: downscale / upscale
  if (flags & DFD_AUG_DOWNUP) {
    const int h2 = pi[10], w2 = pi[11];
    aug_resize(cur, (int64_t)ow * 3, oh, ow, small, h2, w2, false, tab);
    aug_resize(small, (int64_t)w2 * 3, h2, w2, cur, oh, ow, false, tab);
  }

  // 6: blur, or the plain copy out
  uint8_t* out = a.out + (int64_t)n * npix * 3;
  if (flags & DFD_AUG_BLUR) {
    const float k0 = pf[3], k1 = pf[4], k2 = pf[5];
    const float kk[3] = {k0, k1, k2};
    for (int p = tid; p < npix; p += AUG_NT) {
      const int y = p / ow, x = p - y * ow;
      float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f;
#pragma unroll
      for (int dy = 0; dy < 3; ++dy) {
        int yy = y + dy - 1;
        yy = yy < 0 ? 1 : (yy >= oh ? oh - 2 : yy);
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          int xx = x + dx - 1;
          xx = xx < 0 ? 1 : (xx >= ow ? ow - 2 : xx);
          const float w = kk[dy] * kk[dx];
          const uint8_t* px = cur + 3 * ((int64_t)yy * ow + xx);
          acc0 = acc0 + w * (float)px[0];
          acc1 = acc1 + w * (float)px[1];
          acc2 = acc2 + w * (float)px[2];
        }
      }
      uint8_t* d = out + 3 * (int64_t)p;
      d[0] = (uint8_t)fminf(fmaxf(rintf(acc0), 0.f), 255.f);
      d[1] = (uint8_t)fminf(fmaxf(rintf(acc1), 0.f), 255.f);
      d[2] = (uint8_t)fminf(fmaxf(rintf(acc2), 0.f), 255.f);
    }
  } else {
    const int64_t nb = (int64_t)npix * 3;
    if ((nb & 3) == 0 && ((uintptr_t)out & 3) == 0) {
      const uint32_t* c4 = reinterpret_cast<const uint32_t*>(cur);
      uint32_t* o4 = reinterpret_cast<uint32_t*>(out);
      for (int64_t v = tid; v < nb / 4; v += AUG_NT) o4[v] = c4[v];
    } else {
      for (int64_t v = tid; v < nb; v += AUG_NT) out[v] = cur[v];
    }
  }
}

struct AugLayout {
  int tab_ints, small_bytes, cur_bytes;
  int64_t frame_bytes;  // scratch of one frame
  int64_t param_bytes;  // device copy of the two tables (head of the scratch)
  bool lds;
};

AugLayout aug_layout(int n, int src_h, int src_w, int out_h, int out_w) {
  AugLayout l{};
  const int mh = std::max(out_h, 8), mw = std::max(out_w, 8);
  // the three resizes: box -> out, out -> (h2, w2) <= (mh, mw), (h2, w2) -> out
  const int in_h = std::max(src_h, mh), in_w = std::max(src_w, mw);
  l.tab_ints = (aug_tab_dim(in_h, mh) + aug_tab_dim(in_w, mw) + 3) & ~3;
  l.small_bytes = aug_align16((int64_t)mh * mw * 3);
  l.cur_bytes = aug_align16((int64_t)out_h * out_w * 3);
  l.lds = (int64_t)l.cur_bytes + (int64_t)l.tab_ints * 4 + AUG_LDS_STATIC <= AUG_LDS_MAX;
  l.frame_bytes = l.small_bytes + (l.lds ? 0 : (int64_t)l.tab_ints * 4 + l.cur_bytes);
  l.param_bytes = aug_align16((int64_t)n * (DFD_AUG_PI + DFD_AUG_PF) * 4);
  return l;
}

}  // namespace

int64_t augment_scratch_bytes(int n, int src_h, int src_w, int out_h, int out_w) {
  const AugLayout l = aug_layout(n, src_h, src_w, out_h, out_w);
  return l.param_bytes + (int64_t)n * l.frame_bytes;
}

int augment_path(int src_h, int src_w, int out_h, int out_w) {
  return aug_layout(1, src_h, src_w, out_h, out_w).lds ? 1 : 0;
}

int launch_augment_frames(hipStream_t s, const uint8_t* src, int n, int src_h, int src_w, const int32_t* params_i,
                          const float* params_f, int out_h, int out_w, uint8_t* out, void* scratch,
                          int64_t scratch_bytes) {
  const AugLayout l = aug_layout(n, src_h, src_w, out_h, out_w);
  if (scratch_bytes < l.param_bytes + (int64_t)n * l.frame_bytes) {
    set_error("augment_frames: scratch too small (dfd_augment_scratch_bytes)", __FILE__, __LINE__);
    return -1;
  }
  uint8_t* sc = static_cast<uint8_t*>(scratch);
  const int64_t ib = (int64_t)n * DFD_AUG_PI * 4, fb = (int64_t)n * DFD_AUG_PF * 4;
  DFD_HIP_CHECK(hipMemcpyAsync(sc, params_i, ib, hipMemcpyHostToDevice, s));
  DFD_HIP_CHECK(hipMemcpyAsync(sc + ib, params_f, fb, hipMemcpyHostToDevice, s));
  AugArgs a{};
  a.src = src;
  a.pi = reinterpret_cast<const int32_t*>(sc);
  a.pf = reinterpret_cast<const float*>(sc + ib);
  a.out = out;
  a.frame_scratch = sc + l.param_bytes;
  a.frame_scratch_bytes = l.frame_bytes;
  a.src_h = src_h; a.src_w = src_w; a.out_h = out_h; a.out_w = out_w;
  a.tab_ints = l.tab_ints;
  a.small_bytes = l.small_bytes;
  if (l.lds) {
    const int dyn = l.cur_bytes + l.tab_ints * 4;
    // more than 64 KiB of dynamic LDS is opt-in, per device
    DFD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(augment_frames_kernel<true>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, AUG_LDS_MAX - AUG_LDS_STATIC));
    hipLaunchKernelGGL(augment_frames_kernel<true>, dim3(n), dim3(AUG_NT), dyn, s, a);
  } else {
    hipLaunchKernelGGL(augment_frames_kernel<false>, dim3(n), dim3(AUG_NT), 0, s, a);
  }
  DFD_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace dfd
