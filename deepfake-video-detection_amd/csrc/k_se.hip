// Squeeze-excite excitation for the EfficientNet-B0 hot path on gfx950: the SE module's two biased
// 1x1 convs, silu, sigmoid, forward and backward (the squeeze and the one-pass backward sums it reads
// are k_frame.hip's), with the BN backward finalize of the block's second BN folded into the backward.
#include "kernels.h"

#include "tail.h"

namespace dfd {

// ------------------------------------------------------------------ SE excitation (per frame)
// timm SqueezeExcite conv_reduce / act / conv_expand / sigmoid on the per-frame channel means,
// forward and input-gradient backward, as ONE launch each: two chained small GEMMs per tile of
// 16 frames on fp32 MFMA (v_mfma_f32_16x16x4_f32, exact products, fixed summation order):
//   T[f][j]   = epi1( sum_c A[f][c] B1(c, j) )      j < rd  (the 16 waves split c; LDS sum in order)
//   out[f][c] = epi2( sum_j T[f][j] B2(j, c) )      c in this workgroup's channel slice
// forward  A = sq: B1(c,j) = Wr[j][c], T1 = rpre = . + br (saved), T = silu(rpre);
//          B2(j,c) = We[c][j], out = gate = sigmoid(. + be)
// backward A = de = dgate g (1-g): B1(c,j) = We[c][j], T = dz = . * silu'(rpre) (saved);
//          B2(j,c) = Wr[j][c], out = bc = inv_hw * .   (the squeeze path's input gradient)
// The channel slices (gridDim.y) recompute the small first product instead of a second launch.
constexpr int SE_RDMAX = 48, SE_TS = SE_RDMAX + 4, SE_CSL = 256, SE_W = 16;  // SE_W waves per workgroup
#ifndef DFD_SE_B2PF
#define DFD_SE_B2PF 1
#endif
typedef float se_f32x4 __attribute__((ext_vector_type(4)));

// A is read from the squeeze / SE-backward partials A[h][f][c] (h < hsplit, added in order):
// forward A = a_scale * sum (the squeeze mean), backward A = sum * g (1 - g) with g = a_gate[f][c]
// (de = dgate * sigmoid'); the workgroups of channel slice 0 store A to a_out (sq / de), which the
// backward's weight gradients read.
// FIN (backward only): the BN2 backward finalize of bn_bwd_finalize_frames_kernel folded into the
// same launch -- every workgroup adds its 16 frames' terms gate*P1 + bc*P2 / gate*P3 + bc*P4 (fp64)
// for its channel slice into a partial row, and the last-arriving workgroup of the slice (tail.h)
// sums the frame tiles' rows in order and writes dbeta, dgamma and the coefficients k1..k3.
struct SeFin {
  const float* part;  // frame_reduce<FR_SEBN> partials part[5][hsplit][frames][C] (q = 1..4 read)
  int hsplit;
  double* rows;       // [frame tiles][2][C] scratch
  unsigned* ctr;      // one zeroed counter per channel slice
  int64_t count;      // BN rows (frames x HW)
  const float *gamma, *mean, *invstd;
  int training, accumulate;
  float *dgamma, *dbeta, *coef;
};

// SPLIT (SeSplit.on): the first product is split over the channel slices too -- the workgroup of
// slice s sums only k in its own slice (one 16-deep k step per wave instead of C / 256), writes its
// partial T to scratch, the slices of a frame tile meet at a counter barrier (the grid is launched
// slice-fastest and only when every workgroup is co-resident, so the spin cannot starve a sibling)
// and each adds the slices' partials in slice order.  Used where C > 256 (several slices), whose
// first product was a chain of C / 256 dependent load round trips per wave.
struct SeSplit {
  float* tp;      // [frame tiles][slices][16][SE_TS] partial first products
  unsigned* bar;  // 2 zeroed counters (arrive, depart) per frame tile
  int on;
  SyncAbort ab;   // a timed-out slice barrier is reported here (the plan raises on its next call)
};

// grid: x = channel slice (fastest), y = 16-frame tile
template <bool FWD, bool FIN = false>
__global__ __launch_bounds__(64 * SE_W) void se_chain_kernel(const float* __restrict__ A, int hsplit, float a_scale,
                                                       const float* __restrict__ a_gate, float* __restrict__ a_out,
                                                       int frames, int C, int rd,
                                                       const float* __restrict__ W1, const float* __restrict__ b1,
                                                       const float* __restrict__ rpre_in,
                                                       const float* __restrict__ W2, const float* __restrict__ b2,
                                                       float scale2, float* __restrict__ t1_out,
                                                       float* __restrict__ out, SeFin fin, SeSplit sp) {
  __shared__ float red[SE_W][3][4][64];
  __shared__ float Ts[16][SE_TS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int slc = blockIdx.x, nsl = gridDim.x, ftile = blockIdx.y, nft = gridDim.y;
  const int f0 = ftile * 16;
  const int nt1 = (rd + 15) / 16;
  const int cbeg = slc * SE_CSL, cend = min(C, cbeg + SE_CSL);
  // FIN: this lane's second-product outputs are column cbeg + 16 wave + li, frames f0 + 4 lk + r; their
  // gate and frame sums P1..P4 (added over the pixel chunks) are loaded up front, off the chain
  float fgt[4], fp[4][4];
  if constexpr (FIN) {
    const int n = cbeg + 16 * wave + li;
    const int64_t nfc = (int64_t)frames * C;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int f = f0 + 4 * lk + r;
      const bool ok = f < frames && n < C;
      const int64_t i = ok ? (int64_t)f * C + n : 0;
      fgt[r] = ok ? a_gate[i] : 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) fp[r][q] = ok ? fin.part[(int64_t)(q + 1) * fin.hsplit * nfc + i] : 0.f;
    }
    for (int h = 1; h < fin.hsplit; ++h)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = f0 + 4 * lk + r;
        const bool ok = f < frames && n < C;
        const int64_t i = ok ? (int64_t)f * C + n : 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) fp[r][q] += ok ? fin.part[((int64_t)(q + 1) * fin.hsplit + h) * nfc + i] : 0.f;
      }
  }
  // the second product's B2 column of this wave's first (usually only) 16-channel block, loaded up front:
  // independent of T, so its round trip overlaps the first product and the slice barrier instead of
  // following them (DFD_SE_B2PF, A/B build switch)
  float bw0[SE_RDMAX / 4];
  if constexpr (DFD_SE_B2PF) {
    const int n = cbeg + 16 * wave + li;
#pragma unroll
    for (int i = 0; i < SE_RDMAX / 4; ++i) {
      const int k = 4 * i + lk;
      const bool ok = n < cend && k < rd;
      bw0[i] = ok ? (FWD ? W2[(int64_t)n * rd + k] : W2[(int64_t)k * C + n]) : 0.f;
    }
  }
  // ---- T = A[16 frames][C] . B1[C][rd] ----
  se_f32x4 acc1[3];
#pragma unroll
  for (int t = 0; t < 3; ++t) acc1[t] = se_f32x4{0.f, 0.f, 0.f, 0.f};
  const bool fok = f0 + li < frames;
  // k range of the first product: this slice's channels (split) or all of them
  const int kbeg = sp.on ? cbeg : 0, kend = sp.on ? cend : C;
  const bool store_a = sp.on || slc == 0;  // every A element stored once (sq / de for the weight gradients)
  // 16 k per iteration; lane group lk takes k = k0 + 4 lk + u in MFMA step u (the same
  // permutation on both operands), so the row-major operands load as 16-B vectors (C % 8 == 0)
  for (int k0 = kbeg + 16 * wave; k0 < kend; k0 += 16 * SE_W) {
    const int kq = k0 + 4 * lk;
    const bool kok = kq < kend;
    float av[4], bv[4][3];
    if (fok && kok) {
      const int64_t ai = (int64_t)(f0 + li) * C + kq, hn = (int64_t)frames * C;
      float4 a4 = *reinterpret_cast<const float4*>(A + ai);
      if (hsplit > 1)
      for (int h = 1; h < hsplit; ++h) {
        const float4 v = *reinterpret_cast<const float4*>(A + h * hn + ai);
        a4.x += v.x; a4.y += v.y; a4.z += v.z; a4.w += v.w;
      }
      if constexpr (FWD) {
        a4.x *= a_scale; a4.y *= a_scale; a4.z *= a_scale; a4.w *= a_scale;
      } else {
        const float4 g = *reinterpret_cast<const float4*>(a_gate + ai);
        a4.x = a4.x * g.x * (1.f - g.x); a4.y = a4.y * g.y * (1.f - g.y);
        a4.z = a4.z * g.z * (1.f - g.z); a4.w = a4.w * g.w * (1.f - g.w);
      }
      if (store_a) *reinterpret_cast<float4*>(a_out + ai) = a4;
      av[0] = a4.x; av[1] = a4.y; av[2] = a4.z; av[3] = a4.w;
    } else {
      av[0] = av[1] = av[2] = av[3] = 0.f;
    }
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int n = 16 * t + li;
      const bool ok = t < nt1 && n < rd && kok;
      if constexpr (FWD) {
        const float4 b4 = ok ? *reinterpret_cast<const float4*>(W1 + (int64_t)n * C + kq) : make_float4(0.f, 0.f, 0.f, 0.f);
        bv[0][t] = b4.x; bv[1][t] = b4.y; bv[2][t] = b4.z; bv[3][t] = b4.w;
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) bv[u][t] = ok ? W1[(int64_t)(kq + u) * rd + n] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int t = 0; t < 3; ++t)
        if (t < nt1) acc1[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u][t], acc1[t], 0, 0, 0);
  }
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][t][r][lane] = acc1[t][r];
  __syncthreads();
  // element (fl, j): MFMA D layout lane = 16 * (fl / 4) + j % 16, register fl % 4, tile j / 16;
  // 16 x SE_TS < 64 SE_W: one element per thread
  static_assert(16 * SE_TS <= 64 * SE_W, "one first-product element per thread");
  const int fl = tid / SE_TS, j = tid - fl * SE_TS;
  const bool el = tid < 16 * SE_TS && j < rd;
  float v = 0.f;
  if (el) {
    const int t = j >> 4, ln = 16 * (fl >> 2) + (j & 15), r = fl & 3;
#pragma unroll
    for (int w = 0; w < SE_W; ++w) v += red[w][t][r][ln];
  }
  if (sp.on) {  // the slices' partials of this frame tile, added in slice order
    float* tp = sp.tp + (int64_t)ftile * nsl * 16 * SE_TS;
    if (el) tp[slc * 16 * SE_TS + tid] = v;
    // the slice barrier (tail.h); false when it timed out (the workgroup leaves)
    if (!group_sync(sp.bar + 2 * ftile, sp.bar + 2 * ftile + 1, (unsigned)nsl, sp.ab)) return;
    if (el) {  // up to 8 slices' loads in flight, added in slice order
      float pv[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) pv[q] = q < nsl ? tp[q * 16 * SE_TS + tid] : 0.f;
      v = pv[0];
#pragma unroll
      for (int q = 1; q < 8; ++q)
        if (q < nsl) v += pv[q];
      for (int q = 8; q < nsl; ++q) v += tp[q * 16 * SE_TS + tid];
    }
  }
  if (tid < 16 * SE_TS) {
    float tv = 0.f;
    const int f = f0 + fl;
    if (el && f < frames) {
      if constexpr (FWD) {
        v += b1[j];
        if (slc == 0) t1_out[(int64_t)f * rd + j] = v;
        tv = siluf_(v);
      } else {
        v *= dsiluf_(rpre_in[(int64_t)f * rd + j]);
        if (slc == 0) t1_out[(int64_t)f * rd + j] = v;
        tv = v;
      }
    }
    Ts[fl][j] = tv;  // zero for j >= rd and for frames past the end
  }
  __syncthreads();
  // ---- out = T[16][rd] . B2[rd][C slice] ----
  for (int n0 = cbeg + 16 * wave; n0 < cend; n0 += 16 * SE_W) {
    const int n = n0 + li;
    const bool nok = n < cend;
    // all of B2's column for this lane first (<= 12 independent loads in flight), then the MFMA
    // chain in the same k order (one serialized load per MFMA step was the kernel's latency chain)
    float bw[SE_RDMAX / 4];
    const bool pre = DFD_SE_B2PF && n0 == cbeg + 16 * wave;
#pragma unroll
    for (int i = 0; i < SE_RDMAX / 4; ++i) {
      const int k = 4 * i + lk;
      const bool ok = nok && k < rd;
      bw[i] = pre ? bw0[i] : ok ? (FWD ? W2[(int64_t)n * rd + k] : W2[(int64_t)k * C + n]) : 0.f;
    }
    se_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < SE_RDMAX / 4; ++i)
      if (4 * i < rd) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(Ts[li][4 * i + lk], bw[i], acc, 0, 0, 0);
    double fs = 0.0, fq = 0.0;  // FIN: this lane's frames' BN2-backward terms
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int f = f0 + 4 * lk + r;
      if (f < frames && nok) {
        const float o = FWD ? sigmoidf_(acc[r] + b2[n]) : acc[r] * scale2;
        out[(int64_t)f * C + n] = o;
        if constexpr (FIN) {
          fs += (double)fgt[r] * (double)fp[r][0] + (double)o * (double)fp[r][1];
          fq += (double)fgt[r] * (double)fp[r][2] + (double)o * (double)fp[r][3];
        }
      }
    }
    if constexpr (FIN) {
      // the 4 frame groups of a column (lanes li, li+16, li+32, li+48) in a fixed order
      fs += __shfl_xor(fs, 16, 64);
      fq += __shfl_xor(fq, 16, 64);
      fs += __shfl_xor(fs, 32, 64);
      fq += __shfl_xor(fq, 32, 64);
      if (lk == 0 && nok) {
        tail_store(fin.rows + ((int64_t)ftile * 2 + 0) * C + n, fs);
        tail_store(fin.rows + ((int64_t)ftile * 2 + 1) * C + n, fq);
      }
    }
  }
  if constexpr (FIN) {
    if (!tail_arrive(fin.ctr + slc, nft)) return;
    // last workgroup of this channel slice: frame tiles in order, then bn_bwd_finalize_frames' arithmetic
    const int c = cbeg + tid;
    if (c < cend) {
      const float p_g = fin.gamma[c], p_is = fin.invstd[c], p_mu = fin.mean[c];
      const float p_db = fin.accumulate ? fin.dbeta[c] : 0.f, p_dg = fin.accumulate ? fin.dgamma[c] : 0.f;
      double s = 0.0, q = 0.0;
      int t = 0;
      for (; t + 8 <= nft; t += 8) {  // 16 loads in flight, added in tile order
        double vs[8], vq[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          vs[u] = tail_load(fin.rows + ((int64_t)(t + u) * 2 + 0) * C + c);
          vq[u] = tail_load(fin.rows + ((int64_t)(t + u) * 2 + 1) * C + c);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) { s += vs[u]; q += vq[u]; }
      }
      for (; t < nft; ++t) {
        s += tail_load(fin.rows + ((int64_t)t * 2 + 0) * C + c);
        q += tail_load(fin.rows + ((int64_t)t * 2 + 1) * C + c);
      }
      const BnBwdCoef o = bn_bwd_epilogue(s, q, p_g, p_is, p_mu, fin.count, fin.training, 0);
      fin.dbeta[c] = fin.accumulate ? p_db + o.db : o.db;
      fin.dgamma[c] = fin.accumulate ? p_dg + o.dg : o.dg;
      fin.coef[c] = o.k1;
      fin.coef[C + c] = o.k2;
      fin.coef[2 * C + c] = o.k3;
    }
  }
}

// CUs of the current device (co-residency bound of the split excitation's barrier)
static int se_device_cus() {
  static int cus[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
  if (!cus[dev]) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    cus[dev] = n;
  }
  return cus[dev];
}

// the split form where it applies: several slices, one 1024-thread workgroup per CU fits the whole grid
static SeSplit se_split(const SeScratch* sc, int frames, int C) {
  SeSplit sp{};
  if (!sc || !sc->bar || !sc->tp) return sp;
  const int64_t nsl = cdiv(C, SE_CSL), nft = cdiv(frames, 16);
  // >= 4 slices (C > 768): the slice barrier costs ~3-4 us, which the split repays only where the
  // unsplit first product walks >= 4 dependent k steps per wave (trace r05 C: 7x7 stage -2 us per
  // launch, 14x14 stage +0.5..2 us)
  if (nsl < 4 || nsl * nft > se_device_cus() || 2 * nft > sc->bar_slots || nft * nsl * 16 * SE_TS > sc->tp_cap)
    return sp;
  sp.tp = sc->tp;
  sp.bar = sc->bar;
  sp.on = 1;
  static const unsigned long long budget = sync_budget_ticks(2.0);
  sp.ab = SyncAbort{sc->abort_dev, sc->abort_host, budget};
  return sp;
}

int launch_se_fc_fwd(hipStream_t s, const float* part, int hsplit, float inv_hw, float* sq, const float* wr,
                     const float* br, const float* we, const float* be, int frames, int C, int rd, float* rpre,
                     float* gate, const SeScratch* sc) {
  if (rd < 1 || rd > SE_RDMAX) { set_error("se: reduce width out of range", __FILE__, __LINE__); return -1; }
  const dim3 grid((unsigned)cdiv(C, SE_CSL), (unsigned)cdiv(frames, 16));
  hipLaunchKernelGGL(se_chain_kernel<true>, grid, dim3(64 * SE_W), 0, s, part, hsplit, inv_hw, nullptr, sq, frames, C,
                     rd, wr, br, nullptr, we, be, 1.f, rpre, gate, SeFin{}, se_split(sc, frames, C));
  DFD_HIP_CHECK(hipGetLastError());
  return 0;
}

// SE excitation backward from de = dgate * sigmoid'(.) (launch_se_bn_bwd_reduce):
//   dz[f][j]  = silu'(rpre[f][j]) sum_c de[f][c] we[c][j],  bc[f][c] = inv_hw sum_j dz[f][j] wr[j][c]
//                                                          (se_chain_kernel, one launch)
//   gwe[c][j] = sum_f de[f][c] silu(rpre[f][j]),  gbe = sum_f de      (frames ascending)
//   gwr[j][c] = sum_f dz[f][j] sq[f][c],          gbr = sum_f dz      (one paired MFMA launch)
int launch_se_fc_bwd(hipStream_t s, const float* part, int hsplit, const float* gate, float* de, const float* sq,
                     const float* rpre, const float* wr, const float* we, int frames, int C, int rd, float inv_hw,
                     float* tmp_dz, float* bc_out, float* gwr, float* gbr, float* gwe, float* gbe, bool accumulate,
                     MfmaGemm* defer2, const BnFramesFin* bnf, const SeScratch* sc) {
  if (rd < 1 || rd > SE_RDMAX) { set_error("se: reduce width out of range", __FILE__, __LINE__); return -1; }
  const dim3 grid((unsigned)cdiv(C, SE_CSL), (unsigned)cdiv(frames, 16));
  const SeSplit sp = se_split(sc, frames, C);
  if (bnf) {
    if ((int)grid.x > bnf->ctr_slots || (int64_t)grid.y * 2 * C * 2 > bnf->rows_cap) {
      set_error("se: fused finalize scratch too small", __FILE__, __LINE__);
      return -1;
    }
    const SeFin f{part, hsplit, bnf->rows, bnf->ctr, bnf->count, bnf->gamma, bnf->mean, bnf->invstd,
                  bnf->training ? 1 : 0, bnf->accumulate ? 1 : 0, bnf->dgamma, bnf->dbeta, bnf->coef};
    hipLaunchKernelGGL((se_chain_kernel<false, true>), grid, dim3(64 * SE_W), 0, s, part, hsplit, 1.f, gate, de, frames,
                       C, rd, we, nullptr, rpre, wr, nullptr, inv_hw, tmp_dz, bc_out, f, sp);
  } else {
    hipLaunchKernelGGL((se_chain_kernel<false>), grid, dim3(64 * SE_W), 0, s, part, hsplit, 1.f, gate, de, frames, C,
                       rd, we, nullptr, rpre, wr, nullptr, inv_hw, tmp_dz, bc_out, SeFin{}, sp);
  }
  DFD_HIP_CHECK(hipGetLastError());
  MfmaGemm ge{}, gr{};
  ge.A = de; ge.sam = 1; ge.sak = C; ge.B = rpre; ge.sbk = rd; ge.sbn = 1; ge.b_silu = 1; ge.C = gwe; ge.ldc = rd;
  ge.M = C; ge.N = rd; ge.K = frames; ge.asum = gbe; ge.accumulate = accumulate;
  gr.A = tmp_dz; gr.sam = 1; gr.sak = rd; gr.B = sq; gr.sbk = C; gr.sbn = 1; gr.C = gwr; gr.ldc = C;
  gr.M = rd; gr.N = C; gr.K = frames; gr.asum = gbr; gr.accumulate = accumulate;
  if (defer2) {
    defer2[0] = ge;
    defer2[1] = gr;
    return 0;
  }
  return launch_mfma_small_gemm2(s, ge, gr);
}

}  // namespace dfd
