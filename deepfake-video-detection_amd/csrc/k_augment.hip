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
//  4b. (dfd_augment_frames_jpeg only) JPEG recompression at the frame's quality: libjpeg-turbo's baseline 4:2:0
//      round trip in 32-bit integers, one lane per 8 x 8 block, in the dead regions of stage 4 (aug_jpeg below)
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

// ---- JPEG recompression at quality q (stage 4b), libjpeg-turbo's baseline 4:2:0 round trip (jccolor, jcsample,
// jfdctint, the quantiser, jidctint, jdsample's fancy upsampler, jdcolor).  Entropy coding is lossless, so the
// round trip is these integer stages; 32-bit integers throughout, no floating point.
constexpr int aug_fix(double x) { return (int)(x * 65536.0 + 0.5); }  // compile time only

// Annex K in natural order: luminance, then chrominance
__device__ const uint8_t aug_jpeg_base[128] = {
    16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
    14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99,
    17, 18, 24, 47, 99,  99,  99,  99,  18, 21, 26, 66, 99,  99,  99,  99,  24, 26, 56, 99, 99,  99,  99,  99,
    47, 66, 99, 99, 99,  99,  99,  99,  99, 99, 99, 99, 99,  99,  99,  99,  99, 99, 99, 99, 99,  99,  99,  99,
    99, 99, 99, 99, 99,  99,  99,  99,  99, 99, 99, 99, 99,  99,  99,  99};

// jfdctint.c / jidctint.c, CONST_BITS 13, PASS1_BITS 2
constexpr int JF_0_298 = 2446, JF_0_390 = 3196, JF_0_541 = 4433, JF_0_765 = 6270, JF_0_899 = 7373, JF_1_175 = 9633,
              JF_1_501 = 12299, JF_1_847 = 15137, JF_1_961 = 16069, JF_2_053 = 16819, JF_2_562 = 20995,
              JF_3_072 = 25172;

__device__ __forceinline__ int aug_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// the odd half both DCTs share
__device__ __forceinline__ void aug_dct_odd(int& t0, int& t1, int& t2, int& t3) {
  int z1 = t0 + t3, z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
  const int z5 = (z3 + z4) * JF_1_175;
  t0 *= JF_0_298; t1 *= JF_2_053; t2 *= JF_3_072; t3 *= JF_1_501;
  z1 *= -JF_0_899; z2 *= -JF_2_562;
  z3 = z3 * -JF_1_961 + z5;
  z4 = z4 * -JF_0_390 + z5;
  t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
}

// one 8-point forward pass over v[0], v[S], .., v[7 S]
template <int S, bool FIRST>
__device__ __forceinline__ void aug_fdct8(int* v) {
  constexpr int n = FIRST ? 11 : 15;
  const int t0 = v[0] + v[7 * S], t1 = v[S] + v[6 * S], t2 = v[2 * S] + v[5 * S], t3 = v[3 * S] + v[4 * S];
  int t4 = v[3 * S] - v[4 * S], t5 = v[2 * S] - v[5 * S], t6 = v[S] - v[6 * S], t7 = v[0] - v[7 * S];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  v[0] = FIRST ? (t10 + t11) * 4 : aug_descale(t10 + t11, 2);
  v[4 * S] = FIRST ? (t10 - t11) * 4 : aug_descale(t10 - t11, 2);
  const int z1 = (t12 + t13) * JF_0_541;
  v[2 * S] = aug_descale(z1 + t13 * JF_0_765, n);
  v[6 * S] = aug_descale(z1 - t12 * JF_1_847, n);
  aug_dct_odd(t4, t5, t6, t7);
  v[7 * S] = aug_descale(t4, n);
  v[5 * S] = aug_descale(t5, n);
  v[3 * S] = aug_descale(t6, n);
  v[S] = aug_descale(t7, n);
}

template <int S, bool FIRST>
__device__ __forceinline__ void aug_idct8(int* v) {
  constexpr int n = FIRST ? 11 : 18;
  const int z1 = (v[2 * S] + v[6 * S]) * JF_0_541;
  const int e2 = z1 - v[6 * S] * JF_1_847, e3 = z1 + v[2 * S] * JF_0_765;
  const int e0 = (v[0] + v[4 * S]) * (1 << 13), e1 = (v[0] - v[4 * S]) * (1 << 13);
  const int t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
  int t0 = v[7 * S], t1 = v[5 * S], t2 = v[3 * S], t3 = v[S];
  aug_dct_odd(t0, t1, t2, t3);
  v[0] = aug_descale(t10 + t3, n);
  v[7 * S] = aug_descale(t10 - t3, n);
  v[S] = aug_descale(t11 + t2, n);
  v[6 * S] = aug_descale(t11 - t2, n);
  v[2 * S] = aug_descale(t12 + t1, n);
  v[5 * S] = aug_descale(t12 - t1, n);
  v[3 * S] = aug_descale(t13 + t0, n);
  v[4 * S] = aug_descale(t13 - t0, n);
}

// one 8 x 8 block of samples b[8 row + col] through forward DCT (rows, then columns; scaled by 8), quantiser
// table t (round half away from zero), dequantiser, inverse DCT (columns, then rows) and the range-limit table
__device__ __forceinline__ void aug_jpeg_block(int (&b)[64], const uint8_t* t) {
#pragma unroll
  for (int k = 0; k < 64; ++k) b[k] -= 128;
#pragma unroll
  for (int r = 0; r < 8; ++r) aug_fdct8<1, true>(b + 8 * r);
#pragma unroll
  for (int c = 0; c < 8; ++c) aug_fdct8<8, false>(b + c);
#pragma unroll
  for (int k = 0; k < 64; ++k) {
    const int q = t[k], c = b[k];
    const uint32_t d = (uint32_t)q << 3;
    const int m = (int)(((uint32_t)(c < 0 ? -c : c) + (d >> 1)) / d);
    b[k] = (c < 0 ? -m : m) * q;
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) aug_idct8<8, true>(b + c);
#pragma unroll
  for (int r = 0; r < 8; ++r) aug_idct8<1, false>(b + 8 * r);
#pragma unroll
  for (int k = 0; k < 64; ++k) {
    const int x = b[k] & 1023;  // range_limit[(x) & RANGE_MASK], offset by CENTERJSAMPLE
    b[k] = x < 128 ? x + 128 : (x < 512 ? 255 : (x < 896 ? 0 : x - 896));
  }
}

// cur: the (oh, ow) RGB working image, recompressed in place.  tab8 (128 bytes) and planes (2 ceil(oh / 2)
// ceil(ow / 2) bytes) are the dead coefficient-table and downscale regions.  Enters with the workgroup in step
// and leaves it so.  A block task touches what no other task reads -- a Y task byte 0 of its own 64 pixels, a
// chroma task bytes 1 / 2 of its MCU (read) and its own samples of `planes` (written) -- so the tasks need no
// barrier among themselves.
__device__ void aug_jpeg(uint8_t* cur, int oh, int ow, int quality, uint8_t* tab8, uint8_t* planes) {
  const int tid = threadIdx.x, npix = oh * ow;
  const int h2 = (oh + 1) >> 1, w2 = (ow + 1) >> 1;
  if (tid < 128) {  // jpeg_set_quality, baseline
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int v = ((int)aug_jpeg_base[tid] * s + 50) / 100;
    tab8[tid] = (uint8_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
  }
  for (int p = tid; p < npix; p += AUG_NT) {  // jccolor
    uint8_t* px = cur + 3 * (int64_t)p;
    const int r = px[0], g = px[1], b = px[2];
    px[0] = (uint8_t)((aug_fix(.299) * r + aug_fix(.587) * g + aug_fix(.114) * b + 32768) >> 16);
    px[1] = (uint8_t)((-aug_fix(.16874) * r - aug_fix(.33126) * g + aug_fix(.5) * b + (128 << 16) + 32767) >> 16);
    px[2] = (uint8_t)((aug_fix(.5) * r - aug_fix(.41869) * g - aug_fix(.08131) * b + (128 << 16) + 32767) >> 16);
  }
  __syncthreads();

  const int ybx = (ow + 7) >> 3, nyb = ((oh + 7) >> 3) * ybx;
  const int mbx = (ow + 15) >> 4, nmcu = ((oh + 15) >> 4) * mbx;
  for (int task = tid; task < nyb + 2 * nmcu; task += AUG_NT) {
    int b[64];
    const bool is_y = task < nyb;
    int y0, x0, comp = 0;
    if (is_y) {  // edge-replicated to a multiple of 8
      y0 = (task / ybx) << 3;
      x0 = (task - (task / ybx) * ybx) << 3;
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const uint8_t* row = cur + 3 * (int64_t)min(y0 + r, oh - 1) * ow;
#pragma unroll
        for (int c = 0; c < 8; ++c) b[8 * r + c] = row[3 * min(x0 + c, ow - 1)];
      }
    } else {
      // h2v2 downsampling of the MCU's 16 x 16 samples: columns replicated at full resolution (to a multiple of
      // 16, before the averaging), rows replicated to an even height, and below the last downsampled row that row
      const int t = task - nyb, m = t >> 1;
      comp = 1 + (t & 1);
      y0 = (m / mbx) << 3;  // in downsampled coordinates
      x0 = (m - (m / mbx) * mbx) << 3;
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int cy = min(y0 + r, h2 - 1);
        const uint8_t* r0 = cur + 3 * (int64_t)(2 * cy) * ow + comp;
        const uint8_t* r1 = cur + 3 * (int64_t)min(2 * cy + 1, oh - 1) * ow + comp;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const int xa = 3 * min(2 * (x0 + c), ow - 1), xb = 3 * min(2 * (x0 + c) + 1, ow - 1);
          b[8 * r + c] = ((int)r0[xa] + (int)r0[xb] + (int)r1[xa] + (int)r1[xb] + 1 + (c & 1)) >> 2;
        }
      }
    }
    aug_jpeg_block(b, tab8 + (is_y ? 0 : 64));
    if (is_y) {
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        uint8_t* row = cur + 3 * (int64_t)(y0 + r) * ow;
#pragma unroll
        for (int c = 0; c < 8; ++c)
          if (y0 + r < oh && x0 + c < ow) row[3 * (x0 + c)] = (uint8_t)b[8 * r + c];
      }
    } else {  // the real ceil(oh / 2) x ceil(ow / 2) samples only: padding never enters the upsampler
      uint8_t* plane = planes + (comp - 1) * h2 * w2;
#pragma unroll
      for (int r = 0; r < 8; ++r) {
#pragma unroll
        for (int c = 0; c < 8; ++c)
          if (y0 + r < h2 && x0 + c < w2) plane[(y0 + r) * w2 + x0 + c] = (uint8_t)b[8 * r + c];
      }
    }
  }
  __syncthreads();

  // jdsample (h2v2 fancy upsampling: 3/4 near + 1/4 far each way; plain replication when the downsampled width
  // is at most 2, as jinit_upsampler chooses) and jdcolor, per pixel
  for (int p = tid; p < npix; p += AUG_NT) {
    const int y = p / ow, x = p - y * ow, i = y >> 1, j = x >> 1;
    int cc[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const uint8_t* plane = planes + c * h2 * w2;
      int v;
      if (w2 <= 2) {
        v = plane[i * w2 + j];
      } else {
        const int fi = (y & 1) ? min(i + 1, h2 - 1) : max(i - 1, 0);
        const int jo = (x & 1) ? min(j + 1, w2 - 1) : max(j - 1, 0);
        const uint8_t* near = plane + i * w2;
        const uint8_t* far = plane + fi * w2;
        const int cs = 3 * (int)near[j] + (int)far[j], co = 3 * (int)near[jo] + (int)far[jo];
        v = (3 * cs + co + ((x & 1) ? 7 : 8)) >> 4;
      }
      cc[c] = v - 128;
    }
    uint8_t* px = cur + 3 * (int64_t)p;
    const int yy = px[0];
    px[0] = (uint8_t)aug_clampi(yy + ((aug_fix(1.402) * cc[1] + 32768) >> 16));
    px[1] = (uint8_t)aug_clampi(yy + ((-aug_fix(.34414) * cc[0] + 32768 - aug_fix(.71414) * cc[1]) >> 16));
    px[2] = (uint8_t)aug_clampi(yy + ((aug_fix(1.772) * cc[0] + 32768) >> 16));
  }
  __syncthreads();
}

// JPEG: the instantiation with the recompression stage; its per-frame quality (0: stage off) follows the two
// parameter tables in the head of the scratch.  <LDS, false> is the kernel without the stage, unchanged.
template <bool LDS, bool JPEG>
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

  // 5b: JPEG recompression; `tab` and `small` are dead from here on
  if constexpr (JPEG) {
    const int quality = reinterpret_cast<const int32_t*>(a.pf + (int64_t)gridDim.x * DFD_AUG_PF)[n];
    if (quality > 0) aug_jpeg(cur, oh, ow, quality, reinterpret_cast<uint8_t*>(tab), small);
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

AugLayout aug_layout(int n, int src_h, int src_w, int out_h, int out_w, bool jpeg = false) {
  AugLayout l{};
  const int mh = std::max(out_h, 8), mw = std::max(out_w, 8);
  // the three resizes: box -> out, out -> (h2, w2) <= (mh, mw), (h2, w2) -> out
  const int in_h = std::max(src_h, mh), in_w = std::max(src_w, mw);
  l.tab_ints = (aug_tab_dim(in_h, mh) + aug_tab_dim(in_w, mw) + 3) & ~3;
  l.small_bytes = aug_align16((int64_t)mh * mw * 3);
  l.cur_bytes = aug_align16((int64_t)out_h * out_w * 3);
  l.lds = (int64_t)l.cur_bytes + (int64_t)l.tab_ints * 4 + AUG_LDS_STATIC <= AUG_LDS_MAX;
  l.frame_bytes = l.small_bytes + (l.lds ? 0 : (int64_t)l.tab_ints * 4 + l.cur_bytes);
  l.param_bytes = aug_align16((int64_t)n * (DFD_AUG_PI + DFD_AUG_PF + (jpeg ? 1 : 0)) * 4);  // + the qualities
  return l;
}

}  // namespace

int64_t augment_scratch_bytes(int n, int src_h, int src_w, int out_h, int out_w, bool jpeg) {
  const AugLayout l = aug_layout(n, src_h, src_w, out_h, out_w, jpeg);
  return l.param_bytes + (int64_t)n * l.frame_bytes;
}

int augment_path(int src_h, int src_w, int out_h, int out_w) {
  return aug_layout(1, src_h, src_w, out_h, out_w).lds ? 1 : 0;
}

int launch_augment_frames(hipStream_t s, const uint8_t* src, int n, int src_h, int src_w, const int32_t* params_i,
                          const float* params_f, const int32_t* quality, int out_h, int out_w, uint8_t* out,
                          void* scratch, int64_t scratch_bytes) {
  const AugLayout l = aug_layout(n, src_h, src_w, out_h, out_w, quality != nullptr);
  if (scratch_bytes < l.param_bytes + (int64_t)n * l.frame_bytes) {
    set_error(quality ? "augment_frames: scratch too small (dfd_augment_jpeg_scratch_bytes)"
                      : "augment_frames: scratch too small (dfd_augment_scratch_bytes)", __FILE__, __LINE__);
    return -1;
  }
  uint8_t* sc = static_cast<uint8_t*>(scratch);
  const int64_t ib = (int64_t)n * DFD_AUG_PI * 4, fb = (int64_t)n * DFD_AUG_PF * 4;
  DFD_HIP_CHECK(hipMemcpyAsync(sc, params_i, ib, hipMemcpyHostToDevice, s));
  DFD_HIP_CHECK(hipMemcpyAsync(sc + ib, params_f, fb, hipMemcpyHostToDevice, s));
  if (quality) DFD_HIP_CHECK(hipMemcpyAsync(sc + ib + fb, quality, (int64_t)n * 4, hipMemcpyHostToDevice, s));
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
  auto* lds_kernel = quality ? augment_frames_kernel<true, true> : augment_frames_kernel<true, false>;
  auto* scratch_kernel = quality ? augment_frames_kernel<false, true> : augment_frames_kernel<false, false>;
  if (l.lds) {
    const int dyn = l.cur_bytes + l.tab_ints * 4;
    // more than 64 KiB of dynamic LDS is opt-in, per device
    DFD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(lds_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, AUG_LDS_MAX - AUG_LDS_STATIC));
    hipLaunchKernelGGL(lds_kernel, dim3(n), dim3(AUG_NT), dyn, s, a);
  } else {
    hipLaunchKernelGGL(scratch_kernel, dim3(n), dim3(AUG_NT), 0, s, a);
  }
  DFD_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace dfd
