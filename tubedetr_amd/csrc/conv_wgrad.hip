// Weight-gradient kernels for gfx950 (MI355X) and their host code.
//
//   conv_wgrad:  dW[n][k] += sum_m g[m][n] * gather(src)[m][k]             split over m, fp32 atomics
//
// Layout as in gemm_conv.hip (activations NHWC, one source for bf16 and exact fp32); gemm_dev.h holds the device helpers both files share.
// How a call is laid out on the device - kernel, tile class, splits, XCD, slots, fills - is planned by wgrad_plan.h; the host code at the end
// of this file fills WgradParams from the plan and launches it.
//
// Replaces the autograd weight gradients of the torch Conv2d / Linear calls gemm_conv.hip's header lists.
#include <vector>

#include "gemm_dev.h"
#include "gemm_host.h"
#include "wgrad_plan.h"

namespace td {

// ------------------------------------------------------------------------------------------------
// wgrad: dW[co][kk] += sum_{m in split} g[m][co] * gather(src)[m][kk]
// Both operands are reduction-major in memory ([m][channel]); LDS keeps them that way and the bf16
// fragments are produced by the gfx950 transposing LDS read (ds_read_b64_tr_b16).
// ------------------------------------------------------------------------------------------------
struct WgradParams {
  const char* g;
  const char* src;
  float* dw;
  const float* scale;  // out_mode 1/2: per-output-channel factor folded into the result (FrozenBN scale), may be null
  float* dbias;        // optional: dbias[co] += sum_m g[m][co] (column sums of the gradient), by the k-tile-0 workgroups
  td_conv_desc d;
  int M, K, ldg, mper;
  uint32_t g_bytes, src_bytes;
  int out_mode;  // 0: dw = [Nc][K] (K = R*S*C), fp32 atomics.  1: dw = the parameter's own [Nc][ci_real][R][S], atomics.
                 // 2: as 1 with plain stores (the job has a single split: nobody else touches the tile)
  int ci_real;   // input channels of the parameter (C may be padded)
  int tn, tk, first;  // batched launch: tile grid of this job and its first slot (work-item index) inside its XCD
  int cls;            // wide-tile instance (conv_wgrad_wide_batch_kernel): bit 0 = 256 output channels per tile (else 128),
                      // bit 1 = 256 k columns per tile (else 128), bit 2 = pointwise
  unsigned long long* stamps;  // debug: 40 cycle stamps per workgroup (tools/stamp_wgrad.py)
};

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

// LDS image of one stage: G tile [MK][128 channels] and X tile [MK][128 k] - reduction-major rows exactly as they
// lie in HBM, filled by buffer_load ... lds (lane-linear destination).  The transposing fragment reads
// (ds_read_b64_tr_b16) of a 32-lane group touch 8 different rows at one column: rows are a full bank period apart, so
// the 32-byte (bf16) / 64-byte (fp32) column blocks are XOR-swizzled by swz(row) - on the DMA source address and on
// the read, never on the DMA destination.
template <int ES>
__device__ __forceinline__ int wg_swz(int row) {
  return ES == 2 ? ((row & 3) | (((row >> 3) & 1) << 2)) : (row & 7);
}

// Four 32-KiB stages (128 KiB of the CU's 160 KiB LDS, one workgroup per CU), three in flight behind counted
// s_waitcnt vmcnt - the launch has about one workgroup per CU anyway (fp32 atomics per output tile limit the split
// count), so bytes in flight per CU are what is left to raise.
template <typename T, bool PW>
__device__ __forceinline__ void wgrad_body(const WgradParams& p, const int bx, const int by, const int bz, const int lin) {
  constexpr int ES = sizeof(T);
  constexpr int VEC = 16 / ES;
  constexpr int MK = 128 / ES;             // reduction rows per stage: 64 (bf16) / 32 (fp32)
  constexpr int ROWB = 128 * ES;           // bytes per row: 256 / 512
  constexpr int CPR = ROWB / 16;           // 16-byte chunks per row: 16 / 32
  constexpr int RPI = 64 / CPR;            // rows per wave DMA instruction: 4 / 2
  constexpr int LI = MK / (4 * RPI);       // DMA instructions per wave per operand per stage: 4 / 4
  constexpr int SWS = ES == 2 ? 1 : 2;     // log2(16-byte chunks per swizzle block): 32 B / 64 B blocks
  constexpr int TILEB = MK * ROWB;         // 16 KiB
  constexpr uint32_t OOB = 0xFFFFFFF0u;
  __shared__ __attribute__((aligned(16))) char stage0[2 * TILEB];
  __shared__ __attribute__((aligned(16))) char stage1[2 * TILEB];
  __shared__ __attribute__((aligned(16))) char stage2[2 * TILEB];
  __shared__ __attribute__((aligned(16))) char stage3[2 * TILEB];

  const td_conv_desc& d = p.d;
  const int t = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const unsigned long long t_start = __builtin_readcyclecounter();
  const int co0 = bx * 128, kk0 = by * 128;
  const int mbeg = bz * p.mper;
  const int mend = min(p.M, mbeg + p.mper);
  if (mbeg >= mend) return;
  const int HoWo = d.Ho * d.Wo;
  constexpr bool pointwise = PW;  // 1x1, stride 1, no padding: im2col row == source row
  const __amdgpu_buffer_rsrc_t rs_g = __builtin_amdgcn_make_buffer_rsrc((void*)p.g, 0, p.g_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc((void*)p.src, 0, p.src_bytes, 0x00020000);

  // per-lane DMA bookkeeping: instruction i of this wave fills rows (i*4 + wave)*RPI + lane/CPR, LDS chunk lane%CPR
  int rloc[LI], gcol[LI], xr[LI], xs[LI], xc[LI];
  bool gok[LI], xok[LI];
#pragma unroll
  for (int i = 0; i < LI; ++i) {
    const int row = (i * 4 + wave) * RPI + lane / CPR;
    const int c16 = lane % CPR;
    const int blk = (c16 >> SWS) ^ wg_swz<ES>(row);                    // logical swizzle block stored at this slot
    const int col = ((blk << SWS) | (c16 & ((1 << SWS) - 1))) * VEC;   // logical column (elements) inside the tile
    rloc[i] = row;
    gcol[i] = co0 + col;
    gok[i] = gcol[i] < d.Nc;
    const int kk = kk0 + col;
    xok[i] = kk < p.K;
    xr[i] = 0; xs[i] = 0; xc[i] = kk;
    if (d.R * d.S > 1) {
      int tap = kk / d.C;
      xc[i] = kk - tap * d.C;
      xr[i] = tap / d.S;
      xs[i] = tap - xr[i] * d.S;
    }
  }
  // running (row, frame, ho, wo) of each DMA row of this lane; stages are issued strictly in order, MK rows apart, so the
  // im2col coordinates advance by a constant (dN, dH, dW) with one carry each - no divisions, no divergent branches in
  // the loop (the compiler can then interleave the address arithmetic with the MFMAs of the stage being consumed)
  int mcur[LI], rn[LI], rho[LI], rwo[LI];
  const int dN = MK / HoWo, dH = (MK - dN * HoWo) / d.Wo, dW = MK - dN * HoWo - dH * d.Wo;
#pragma unroll
  for (int i = 0; i < LI; ++i) {
    mcur[i] = mbeg + rloc[i];
    rn[i] = mcur[i] / HoWo;
    const int rem = mcur[i] - rn[i] * HoWo;
    rho[i] = rem / d.Wo;
    rwo[i] = rem - rho[i] * d.Wo;
  }
  auto issue_stage = [&](char* st) {
#pragma unroll
    for (int i = 0; i < LI; ++i) {
      const int m = mcur[i];
      const bool ok = m < mend;
      const uint32_t og = (ok && gok[i]) ? ((uint32_t)m * (uint32_t)p.ldg + (uint32_t)gcol[i]) * ES : OOB;
      uint32_t ox;
      if constexpr (pointwise) {
        ox = (ok && xok[i]) ? ((uint32_t)m * (uint32_t)d.C + (uint32_t)xc[i]) * ES : OOB;
      } else {
        const int hs = rho[i] * d.stride - d.pad + xr[i], ws = rwo[i] * d.stride - d.pad + xs[i];
        const bool in = ok && xok[i] && (unsigned)hs < (unsigned)d.Hs && (unsigned)ws < (unsigned)d.Ws;
        ox = in ? ((uint32_t)((rn[i] * d.Hs + hs) * d.Ws + ws) * (uint32_t)d.C + (uint32_t)xc[i]) * ES : OOB;
        rwo[i] += dW;
        const int c1 = rwo[i] >= d.Wo;
        rwo[i] -= c1 ? d.Wo : 0;
        rho[i] += dH + c1;
        const int c2 = rho[i] >= d.Ho;
        rho[i] -= c2 ? d.Ho : 0;
        rn[i] += dN + c2;
      }
      mcur[i] += MK;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_g, (lds_ptr_t)(st + (i * 4 + wave) * 1024), 16, og, 0, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_x, (lds_ptr_t)(st + TILEB + (i * 4 + wave) * 1024), 16, ox, 0, 0, 0);
    }
  };

  const int wy = wave >> 1, wx = wave & 1;  // wy: co direction, wx: kk direction
  const int lr = lane & 15, lg = lane >> 4;
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // bias gradient = column sums of g: one more MFMA per G fragment against an all-ones operand, only in the
  // workgroups of the first k tile (every column of the product holds the same sums)
  const bool do_bias = p.dbias != nullptr && by == 0;
  f32x4 accb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) accb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto compute_stage = [&](const char* st) {
    const char* sG = st;
    const char* sX = st + TILEB;
    if constexpr (ES == 2) {
      // all fragment reads of the stage are issued before the first MFMA: one wavefront per SIMD has nobody to hide the
      // LDS latency behind, so the second half's reads must fly while the first half multiplies
      constexpr int KS = MK / 32;
      const int jrow = lr >> 2, q = lr & 3;
      const int f = jrow | ((lg & 1) << 2);  // = wg_swz(r0) = wg_swz(r1)
      uint4 gf[KS][4], xf[KS][4];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const int r0 = ks * 32 + 8 * lg + jrow, r1 = r0 + 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int cb = (((wy * 4 + i) ^ f) << 5) + q * 8;
          bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(sG + r0 * ROWB + cb));
          bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(sG + r1 * ROWB + cb));
          uint2 l2 = *(uint2*)&lo, h2 = *(uint2*)&hi;
          gf[ks][i] = make_uint4(l2.x, l2.y, h2.x, h2.y);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int cb = (((wx * 4 + j) ^ f) << 5) + q * 8;
          bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(sX + r0 * ROWB + cb));
          bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(sX + r1 * ROWB + cb));
          uint2 l2 = *(uint2*)&lo, h2 = *(uint2*)&hi;
          xf[ks][j] = make_uint4(l2.x, l2.y, h2.x, h2.y);
        }
      }
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)&gf[ks][i], *(const bf16x8*)&xf[ks][j], acc[i][j], 0, 0, 0);
      if (do_bias) {
        const uint4 ones = make_uint4(0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u);  // 8 x bf16(1.0)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
          for (int i = 0; i < 4; ++i)
            accb[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8*)&gf[ks][i], *(const bf16x8*)&ones, accb[i], 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int s4 = 0; s4 < MK / 4; ++s4) {
        float gf[4], xf[4];
        const int krow = lg + 4 * s4;
        const int f = krow & 7;
#pragma unroll
        for (int i = 0; i < 4; ++i) gf[i] = *(const float*)(sG + krow * ROWB + (((wy * 4 + i) ^ f) << 6) + lr * 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) xf[j] = *(const float*)(sX + krow * ROWB + (((wx * 4 + j) ^ f) << 6) + lr * 4);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(gf[i], xf[j], acc[i][j], 0, 0, 0);
        if (do_bias) {
#pragma unroll
          for (int i = 0; i < 4; ++i) accb[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(gf[i], 1.0f, accb[i], 0, 0, 0);
        }
      }
    }
  };

  const int nit = (mend - mbeg + MK - 1) / MK;
  unsigned long long* stp = p.stamps ? p.stamps + (size_t)lin * 40 : nullptr;
#define TD_WSTAMP(i) do { if (stp && t == 0) stp[i] = __builtin_readcyclecounter(); } while (0)
  if (stp && t == 0) stp[0] = t_start;
  TD_WSTAMP(1);
  // every step issues exactly one stage (rows past mend are all-OOB = zero fill, no traffic), so "the stage I am about
  // to read has landed" is always "at most two stages = 4*LI DMA instructions of this wave still outstanding"
#define TD_WG_STEP(cur, nxt, j)                                                        \
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * LI) : "memory");                      \
  __builtin_amdgcn_s_barrier();                                                       \
  issue_stage(nxt);                                                                   \
  if ((j) >= 0) { compute_stage(cur); if ((j) < 32) TD_WSTAMP(4 + (j)); }
  // software-pipeline warm-up folded into the loop (steps -3..-1 only issue): every stage buffer has exactly one
  // static DMA site, which keeps the compiler's own LDS-DMA wait counts exact
  for (int it = -3; it < nit; it += 4) {
    TD_WG_STEP(stage1, stage0, it)
    if (it + 1 >= nit) break;
    TD_WG_STEP(stage2, stage1, it + 1)
    if (it + 2 >= nit) break;
    TD_WG_STEP(stage3, stage2, it + 2)
    if (it + 3 >= nit) break;
    TD_WG_STEP(stage0, stage3, it + 3)
  }
#undef TD_WG_STEP
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // trailing zero-fill DMAs must not outlive the workgroup's LDS
  // D[i=co][j=kk]: lane holds co = base + 4*lg + r, kk = base + lr
  TD_WSTAMP(2);
  if (do_bias && wx == 0 && lr == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int coo = co0 + wy * 64 + i * 16 + 4 * lg + rr;
        if (coo >= d.Nc) continue;
        if (p.out_mode == 2) p.dbias[coo] = accb[i][rr];  // single split: this workgroup owns the column sums of its channels
        else atomicAdd(p.dbias + coo, accb[i][rr]);
      }
  }
  if (p.out_mode == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int kko = kk0 + wx * 64 + j * 16 + lr;
        if (kko >= p.K) continue;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          int coo = co0 + wy * 64 + i * 16 + 4 * lg + rr;
          if (coo < d.Nc) atomicAdd(p.dw + (size_t)coo * p.K + kko, acc[i][j][rr]);
        }
      }
  } else {
    // straight into the parameter's [Nc][ci_real][R][S] layout with the FrozenBN scale folded (what wgrad_finalize did)
    const int RS = d.R * d.S;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int kko = kk0 + wx * 64 + j * 16 + lr;
      if (kko >= p.K) continue;
      const int tap = kko / d.C, ci = kko - tap * d.C;
      if (ci >= p.ci_real) continue;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int coo = co0 + wy * 64 + i * 16 + 4 * lg + rr;
          if (coo >= d.Nc) continue;
          const float v = acc[i][j][rr] * (p.scale ? p.scale[coo] : 1.f);
          float* dst = p.dw + ((size_t)coo * p.ci_real + ci) * RS + tap;
          if (p.out_mode == 2) *dst = v;
          else atomicAdd(dst, v);
        }
    }
  }
  TD_WSTAMP(3);
#undef TD_WSTAMP
}

template <typename T, bool PW>
__global__ __launch_bounds__(256, 1) void conv_wgrad_kernel(WgradParams p) {
  wgrad_body<T, PW>(p, blockIdx.x, blockIdx.y, blockIdx.z, blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z));
}

// Batched form: one launch covers the weight gradients of many layers.  With every trainable conv of the trunk in one
// launch there are thousands of tiles, so a job needs no (or few) splits: no atomics, no accumulator memset, no separate
// finalize pass - and no per-layer tail where 256 CUs wait on the slowest workgroup.
// Workgroup w runs on XCD w % 8 (round-robin dispatch): each job is owned by ONE XCD (host-side longest-first
// balancing), so the 32 CUs that share an L2 stream the same gradient / activation rows at about the same time and every
// operand row is fetched into that L2 once instead of once per tile.  Within its XCD a workgroup finds its job by
// binary search over the job's first slot.
struct WgradXcdIndex {
  int start[9];  // job table range of XCD x: [start[x], start[x+1])
  int slots[8];  // work items of XCD x
};

template <typename T, bool PW>
__global__ __launch_bounds__(256, 1) void conv_wgrad_batch_kernel(const WgradParams* __restrict__ jobs, WgradXcdIndex xi) {
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  if (slot >= xi.slots[xcd]) return;
  int lo = xi.start[xcd], hi = xi.start[xcd + 1] - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].first <= slot) lo = mid;
    else hi = mid - 1;
  }
  const WgradParams p = jobs[lo];
  int local = slot - p.first;
  const int bx = local % p.tn;
  local /= p.tn;
  const int by = local % p.tk;
  wgrad_body<T, PW>(p, bx, by, local / p.tk, blockIdx.x);
}

// ------------------------------------------------------------------------------------------------
// Wide-tile weight gradients (bf16, batched launches, large M): the 128 x 128 instance above moves 32 KiB HBM/L2 -> LDS per
// 128 MFMAs with ONE wavefront per SIMD - 0.17 of the MFMA peak measured over the trunk's 93 jobs.  Here a workgroup of
// SIXTEEN wavefronts (four per SIMD: the LDS latency of one is covered by the MFMAs of the others, no fragment double
// buffering, 128 registers each) owns a 256 (output channels) x 256 (k) tile of dW - or 128 x 256 / 256 x 128 for the
// 128-wide layers - and walks its slice of the reduction in stages of 64 rows: 64 KiB per 512 MFMAs, the gradient rows of a
// 256-channel layer read once per k tile.  LDS image: each 128-column sub-tile exactly as in the instance above
// (reduction-major rows as they lie in HBM, swizzled 32-byte blocks, ds_read_b64_tr_b16 fragment reads); one DMA
// instruction per wavefront, sub-tile and stage.  The barrier that publishes stage s + 1 sits between the fragment reads and
// the MFMAs of the last k-step of stage s, so its skew is covered by 16 MFMAs per wavefront.  Output straight into the
// parameter's [Nc][ci][R][S] layout with the FrozenBN scale folded (plain stores for unsplit jobs, fp32 atomics otherwise).
// Nc and C are multiples of 128 (host-checked): a sub-tile is inside the matrix or outside as a whole and lies within ONE
// filter tap - validity, tap and channel base are wave-uniform scalars, the lane only adds its column.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <int GS, int XS, bool PW>
__device__ __forceinline__ void wgrad_wide_body(const WgradParams& p, const int bx, const int by, const int bz, char* st0, char* st1) {
  constexpr int ES = 2, MK = 64, ROWB = 256, SUB = MK * ROWB;  // one 128-column sub-tile = 16 KiB
  constexpr int RPW = 1;  // DMA instructions (4 rows each) per wavefront, sub-tile and stage.  (The one-trip loops over it stay as loops: written out as
                          // scalars, the same arithmetic comes out of the compiler in another instruction order, and this kernel's schedule is measured.)
  constexpr int WVK = XS * 2, WVC = 16 / WVK;  // wavefronts along k / along the output channels
  constexpr int WCO = GS * 128 / WVC;          // output channels per wavefront: 64 or 32
  constexpr int FI = WCO / 16, FJ = 4;
  constexpr uint32_t OOB = 0xFFFFFFF0u;
  const td_conv_desc& d = p.d;
  const int t = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const int co0 = bx * (GS * 128), kk0 = by * (XS * 128);
  const int mbeg = bz * p.mper;
  const int mend = min(p.M, mbeg + p.mper);
  if (mbeg >= mend) return;
  const int HoWo = d.Ho * d.Wo;
  const __amdgpu_buffer_rsrc_t rs_g = __builtin_amdgcn_make_buffer_rsrc((void*)p.g, 0, p.g_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc((void*)p.src, 0, p.src_bytes, 0x00020000);

  // DMA bookkeeping: this wavefront's instruction fills rows wave * 4 + lane/16 of every sub-tile, LDS chunk lane%16
  const int drow = wave * 4 + (lane >> 4);
  const int c16 = lane & 15;
  const int col = ((((c16 >> 1) ^ wg_swz<ES>(drow)) << 1) | (c16 & 1)) * 8;  // logical column of this lane's chunk
  int mcur = mbeg + drow;
  int rn[RPW], rho[RPW], rwo[RPW];
#pragma unroll
  for (int h = 0; h < RPW; ++h) {
    const int m_ = mcur + 4 * h;
    rn[h] = m_ / HoWo;
    rho[h] = (m_ - rn[h] * HoWo) / d.Wo;
    rwo[h] = m_ - rn[h] * HoWo - rho[h] * d.Wo;
  }
  bool g_in[GS], x_in[XS];
  int g_c0[GS], x_c0[XS], x_r[XS], x_s[XS];
#pragma unroll
  for (int s_ = 0; s_ < GS; ++s_) {
    g_c0[s_] = co0 + s_ * 128;
    g_in[s_] = g_c0[s_] < d.Nc;
  }
#pragma unroll
  for (int s_ = 0; s_ < XS; ++s_) {
    const int kk = kk0 + s_ * 128;
    x_in[s_] = kk < p.K;
    x_r[s_] = 0; x_s[s_] = 0; x_c0[s_] = kk;
    if (!PW && d.R * d.S > 1) {
      const int tap = kk / d.C;
      x_c0[s_] = kk - tap * d.C;
      x_r[s_] = tap / d.S;
      x_s[s_] = tap - x_r[s_] * d.S;
    }
  }
  const int dN = MK / HoWo, dH = (MK - dN * HoWo) / d.Wo, dW = MK - dN * HoWo - dH * d.Wo;
  auto issue_stage = [&](char* st) {
#pragma unroll
    for (int h = 0; h < RPW; ++h) {
      const int m = mcur + 4 * h;
      const bool ok = m < mend;
      const uint32_t grow = ((uint32_t)m * (uint32_t)p.ldg + (uint32_t)col) * ES;
#pragma unroll
      for (int s_ = 0; s_ < GS; ++s_) {
        const uint32_t og = (ok && g_in[s_]) ? grow + (uint32_t)g_c0[s_] * ES : OOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_g, (lds_ptr_t)(st + s_ * SUB + (wave * RPW + h) * 1024), 16, og, 0, 0, 0);
      }
#pragma unroll
      for (int s_ = 0; s_ < XS; ++s_) {
        uint32_t ox;
        if constexpr (PW) {
          ox = (ok && x_in[s_]) ? ((uint32_t)m * (uint32_t)d.C + (uint32_t)(x_c0[s_] + col)) * ES : OOB;
        } else {
          const int hs = rho[h] * d.stride - d.pad + x_r[s_], ws = rwo[h] * d.stride - d.pad + x_s[s_];
          const bool in = ok && x_in[s_] && (unsigned)hs < (unsigned)d.Hs && (unsigned)ws < (unsigned)d.Ws;
          ox = in ? ((uint32_t)((rn[h] * d.Hs + hs) * d.Ws + ws) * (uint32_t)d.C + (uint32_t)(x_c0[s_] + col)) * ES : OOB;
        }
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_x, (lds_ptr_t)(st + (GS + s_) * SUB + (wave * RPW + h) * 1024), 16, ox, 0, 0, 0);
      }
      if constexpr (!PW) {
        rwo[h] += dW;
        const int c1 = rwo[h] >= d.Wo;
        rwo[h] -= c1 ? d.Wo : 0;
        rho[h] += dH + c1;
        const int c2 = rho[h] >= d.Ho;
        rho[h] -= c2 ? d.Ho : 0;
        rn[h] += dN + c2;
      }
    }
    mcur += MK;
  };

  const int wyc = wave / WVK, wxk = wave - wyc * WVK;
  const int lr = lane & 15, lg = lane >> 4;
  const int jrow = lr >> 2, q = lr & 3;
  int f = jrow | ((lg & 1) << 2);  // = wg_swz(r0) = wg_swz(r1)
  f32x4 acc[FI][FJ];
#pragma unroll
  for (int i = 0; i < FI; ++i)
#pragma unroll
    for (int j = 0; j < FJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  u32x4 gf[FI], xf[FJ];
  auto frag = [&](const char* sub, int ks, int blk16) -> u32x4 {
    const int r0 = ks * 32 + 8 * lg + jrow;
    const int cb = ((blk16 ^ f) << 5) + q * 8;
    bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(sub + r0 * ROWB + cb));
    bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(sub + (r0 + 4) * ROWB + cb));
    const uint2 l2 = *(uint2*)&lo, h2 = *(uint2*)&hi;
    return u32x4{l2.x, l2.y, h2.x, h2.y};
  };
  auto load_frags = [&](const char* st, int ks) {
    const int xoff = wxk * 64, goff = wyc * WCO;  // both inside one sub-tile (WCO <= 64)
    // the swizzle operand is laundered per call: the 2 x (FI + FJ) fragment addresses are then recomputed where they are
    // used (an xor and a shift-add in the shadow of the MFMAs) instead of living in 16 registers across the loop
    asm volatile("" : "+v"(f));
#pragma unroll
    for (int i = 0; i < FI; ++i) gf[i] = frag(st + ((goff + i * 16) / 128) * SUB, ks, ((goff + i * 16) % 128) / 16);
#pragma unroll
    for (int j = 0; j < FJ; ++j) xf[j] = frag(st + (GS + xoff / 128) * SUB, ks, (xoff % 128) / 16 + j);
  };
  // The accumulator operand is TIED (inline asm "+v"): with the builtin the register allocator renames the accumulators
  // through the two-stage loop body (destination != source C on most MFMAs), which doubles their footprint and spills.
  // Hazards the compiler cannot see inside the asm: an accumulator is touched again 15 MFMAs (>= 240 cycles) later, and the
  // epilogue below waits explicitly before its first VALU read.
  auto mfmas = [&]() {
#pragma unroll
    for (int i = 0; i < FI; ++i)
#pragma unroll
      for (int j = 0; j < FJ; ++j)
        asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc[i][j]) : "v"(gf[i]), "v"(xf[j]));
  };
  // Round 6: the refill of a stage buffer is issued the moment the buffer is free - behind the barrier that follows its last fragment
  // read, i.e. in the middle of the stage that consumed it, for the stage AFTER the next one - and waited for one whole stage later.
  // (Rounds 4 - 5 issued it at the head of the next stage and waited for it in that stage's middle: half a stage, ~0.5 us, of lead for a
  // load that takes longer than that under load.)
  auto stage_body = [&](char* cur, char* nxt) {
    (void)nxt;
    load_frags(cur, 0);
    __builtin_amdgcn_sched_barrier(0);  // (the scheduler would hoist the second k-step's reads: 2 x 32 fragment registers)
    mfmas();
    __builtin_amdgcn_sched_barrier(0);
    load_frags(cur, 1);
    __builtin_amdgcn_s_waitcnt(0x0070);  // vmcnt(0) lgkmcnt(0): own DMA of the next stage (issued a stage ago) landed, own reads of `cur` returned
    __builtin_amdgcn_s_barrier();
    issue_stage(cur);  // every wavefront has read its last fragment of `cur`: refill it with the rows of the stage after next (past the slice: all-OOB, no traffic)
    mfmas();
    __builtin_amdgcn_sched_barrier(0);
  };

  // ONE loop over stage pairs and nothing else: an odd stage count is rounded up (rows past the slice are zero-filled
  // without traffic).  A separate tail would bring register spills of the accumulators, and a spill store right behind an
  // inline-asm MFMA lacks the MFMA -> VMEM wait states the compiler adds for MFMAs it knows about.
  const int npair = ((mend - mbeg + MK - 1) / MK + 1) / 2;
  issue_stage(st0);
  issue_stage(st1);
  __syncthreads();
#pragma unroll 1
  for (int it = 0; it < npair; ++it) {
    stage_body(st0, st1);
    stage_body(st1, st0);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the two trailing (all-OOB) refills must not outlive the workgroup's LDS
  // last MFMA results -> first read: 2 x 16 idle cycles, and every accumulator passes through an asm "modification" placed
  // behind them, so no compiler-generated use (VALU read, spill store) of an accumulator can be scheduled before the wait
  asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
#pragma unroll
  for (int i = 0; i < FI; ++i)
#pragma unroll
    for (int j = 0; j < FJ; ++j) asm volatile("" : "+v"(acc[i][j]));
  // D[i = co][j = kk]: lane holds co = base + 4*lg + rr, kk = base + lr
  const int RS = d.R * d.S;
#pragma unroll
  for (int j = 0; j < FJ; ++j) {
    const int kko = kk0 + wxk * 64 + j * 16 + lr;
    if (kko >= p.K) continue;
    int tap = 0, ci = kko;
    if (!PW && RS > 1) {
      tap = kko / d.C;
      ci = kko - tap * d.C;
    }
    if (ci >= p.ci_real) continue;
#pragma unroll
    for (int i = 0; i < FI; ++i)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int coo = co0 + wyc * WCO + i * 16 + 4 * lg + rr;
        if (coo >= d.Nc) continue;
        const float v = acc[i][j][rr] * (p.scale ? p.scale[coo] : 1.f);
        float* dst = p.dw + ((size_t)coo * p.ci_real + ci) * RS + tap;
        if (p.out_mode == 2) *dst = v;
        else atomicAdd(dst, v);
      }
  }
}

__global__ __launch_bounds__(1024, 1) void conv_wgrad_wide_batch_kernel(const WgradParams* __restrict__ jobs, WgradXcdIndex xi) {
  __shared__ __attribute__((aligned(16))) char wst0[65536];
  __shared__ __attribute__((aligned(16))) char wst1[65536];
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  if (slot >= xi.slots[xcd]) return;
  int lo = xi.start[xcd], hi = xi.start[xcd + 1] - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].first <= slot) lo = mid;
    else hi = mid - 1;
  }
  const WgradParams p = jobs[lo];
  int local = slot - p.first;
  const int bx = local % p.tn;
  local /= p.tn;
  const int by = local % p.tk, bz = local / p.tk;
  switch (p.cls) {
    case 3: wgrad_wide_body<2, 2, false>(p, bx, by, bz, wst0, wst1); break;
    case 7: wgrad_wide_body<2, 2, true>(p, bx, by, bz, wst0, wst1); break;
    case 2: wgrad_wide_body<1, 2, false>(p, bx, by, bz, wst0, wst1); break;
    case 6: wgrad_wide_body<1, 2, true>(p, bx, by, bz, wst0, wst1); break;
    case 1: wgrad_wide_body<2, 1, false>(p, bx, by, bz, wst0, wst1); break;
    default: wgrad_wide_body<2, 1, true>(p, bx, by, bz, wst0, wst1); break;
  }
}


}  // namespace td

using namespace td;

// ---- host side: wgrad_plan.h decides, this launches ----

// everything of WgradParams the plan and the job determine (batched launches add dw / dbias / scale / ci_real)
static WgradParams wgrad_params(const WgradJobPlan& q, const void* g, const void* src, const td_conv_desc* d, int ldg) {
  WgradParams p;
  memset(&p, 0, sizeof(p));
  p.g = (const char*)g;
  p.src = (const char*)src;
  p.d = *d;
  p.M = q.M;
  p.K = q.K;
  p.ldg = ldg;
  p.mper = q.mper;
  p.g_bytes = q.g_bytes;
  p.src_bytes = q.src_bytes;
  p.out_mode = q.out_mode;
  p.ci_real = d->C;
  p.tn = q.tn;
  p.tk = q.tk;
  p.first = q.first;
  p.cls = q.cls;
  p.stamps = stamp_buffer();
  return p;
}

extern "C" int td_conv_wgrad(const void* g, const void* src, float* dw, const td_conv_desc* d, int ldg, int dtype,
                             int splits, td_stream_t stream) {
  return td_conv_wgrad_bias(g, src, dw, nullptr, d, ldg, dtype, splits, stream);
}

extern "C" int td_conv_wgrad_bias(const void* g, const void* src, float* dw, float* dbias, const td_conv_desc* d, int ldg,
                                  int dtype, int splits, td_stream_t stream) {
  TD_REQUIRE(g && src && dw && d, "td_conv_wgrad: null pointer");
  WgradJobPlan q;
  int rc = plan_wgrad_single(d, ldg, dtype, splits, deterministic(), gemm_knobs(), q);
  if (rc) return rc;
  WgradParams p = wgrad_params(q, g, src, d, ldg);
  p.dw = dw;
  p.dbias = dbias;
  dim3 grid(q.tn, q.tk, q.splits);
  hipStream_t st = (hipStream_t)stream;
  const bool prof = prof_on();
  if (prof) prof_begin(TD_PROF_WGRAD_SINGLE, dtype, 2.0 * p.M * d->Nc * p.K, st, p.M, d->Nc, p.K, d->R, d->stride, q.splits);
  if (prof) prof_set_bytes(((double)p.M * ldg + (double)d->N * d->Hs * d->Ws * d->C) * (dtype == TD_BF16 ? 2.0 : 4.0) + (double)d->Nc * p.K * 4.0);
  const bool pw = q.kernel == TD_WGRAD_KERNEL_POINTWISE;
#define TD_WG_LAUNCH(TT)                                                    \
  do {                                                                      \
    if (pw) conv_wgrad_kernel<TT, true><<<grid, 256, 0, st>>>(p);           \
    else conv_wgrad_kernel<TT, false><<<grid, 256, 0, st>>>(p);             \
  } while (0)
  if (dtype == TD_BF16) TD_WG_LAUNCH(u16);
  else TD_WG_LAUNCH(float);
#undef TD_WG_LAUNCH
  if (prof) prof_end(st);
  return check_launch("td_conv_wgrad");
}

// ---- batched weight gradients ----
// The job table of a launch lives in caller-provided memory: the library writes it into `table_host` (page-locked),
// enqueues ONE hipMemcpyAsync into `table_dev` on the caller's stream and launches; no allocation, no synchronisation.
static size_t wg_table_half(int n_jobs) { return (((size_t)n_jobs * sizeof(WgradParams)) + 255) & ~(size_t)255; }
extern "C" size_t td_conv_wgrad_batch_table_bytes(int n_jobs) { return n_jobs > 0 ? 6 * wg_table_half(n_jobs) : 0; }  // (general / pointwise / wide-tile tables) x (overwriting / accumulating jobs)

extern "C" int td_conv_wgrad_batch_plan(const td_wgrad_job* jobs, int n_jobs, int dtype, int n_cu, int deterministic_mode, td_wgrad_plan_job* plan_jobs,
                                        td_wgrad_plan_launch* launches, int* n_launches) {
  TD_REQUIRE(jobs && n_jobs >= 1, "td_conv_wgrad_batch: no jobs");
  TD_REQUIRE(plan_jobs && launches && n_launches, "td_conv_wgrad_batch_plan: null pointer");
  TD_REQUIRE(n_cu >= 1, "td_conv_wgrad_batch_plan: n_cu=%d", n_cu);
  std::vector<WgradJobPlan> plan(n_jobs);
  int rc = plan_wgrad_batch(jobs, n_jobs, dtype, n_cu, deterministic_mode != 0, gemm_knobs(), plan.data(), launches, n_launches);
  if (rc) return rc;
  for (int i = 0; i < n_jobs; ++i) plan_jobs[i] = plan[i];
  return TD_OK;
}

extern "C" int td_conv_wgrad_batch(const td_wgrad_job* jobs, int n_jobs, int dtype, void* table_host, void* table_dev,
                                   size_t table_bytes, td_stream_t stream) {
  TD_REQUIRE(jobs && n_jobs >= 1, "td_conv_wgrad_batch: no jobs");
  TD_REQUIRE(table_host && table_dev && table_bytes >= td_conv_wgrad_batch_table_bytes(n_jobs),
             "td_conv_wgrad_batch: job-table workspace missing or smaller than td_conv_wgrad_batch_table_bytes(%d)", n_jobs);
  std::vector<WgradJobPlan> plan(n_jobs);
  td_wgrad_plan_launch launches[6];
  int n_launches = 0;
  int rc = plan_wgrad_batch(jobs, n_jobs, dtype, cu_count(), deterministic(), gemm_knobs(), plan.data(), launches, &n_launches);
  if (rc) return rc;
  // launch (phase, kernel) owns sixth 3 * phase + kernel of the caller's table
  hipStream_t st = (hipStream_t)stream;
  const size_t half = wg_table_half(n_jobs);
  auto table = [&](void* base, const td_wgrad_plan_launch& L) { return (WgradParams*)((char*)base + (3 * L.phase + L.kernel) * half); };
  for (int i = 0; i < n_jobs; ++i) {
    const td_wgrad_job& j = jobs[i];
    const WgradJobPlan& q = plan[i];
    WgradParams& p = table(table_host, launches[q.launch])[q.pos];
    p = wgrad_params(q, j.g, j.src, &j.d, j.ldg);
    p.dw = j.dW;
    p.dbias = j.dbias;
    p.scale = j.scale;
    p.ci_real = j.ci_real;
    if ((q.fill_dw && hipMemsetAsync(j.dW, 0, (size_t)j.d.Nc * j.ci_real * j.d.R * j.d.S * sizeof(float), st) != hipSuccess) ||
        (q.fill_dbias && hipMemsetAsync(j.dbias, 0, (size_t)j.d.Nc * sizeof(float), st) != hipSuccess)) {
      set_error("td_conv_wgrad_batch: memset failed");
      return TD_ERR_LAUNCH;
    }
  }
  const bool prof = prof_on();
  for (int l = 0; l < n_launches; ++l) {
    const td_wgrad_plan_launch& L = launches[l];
    if (prof && (l == 0 || launches[l - 1].phase != L.phase)) {  // one profiler row per phase: the sums over its launches
      double flops = 0, abytes = 0;
      int members = 0;
      for (int m = l; m < n_launches && launches[m].phase == L.phase; ++m) flops += launches[m].flops, abytes += launches[m].bytes, members += launches[m].n_jobs;
      prof_begin(TD_PROF_WGRAD, dtype, flops, st, 0, 0, 0, 0, 0, members);
      prof_set_bytes(abytes);
    }
    // the async copy reads table_host when the stream gets there (or, inside a captured graph, at every replay): the caller keeps both
    // buffers untouched until then
    const WgradParams* dev = table(table_dev, L);
    if (hipMemcpyAsync((void*)dev, table(table_host, L), L.n_jobs * sizeof(WgradParams), hipMemcpyHostToDevice, st) != hipSuccess) {
      set_error("td_conv_wgrad_batch: job table upload failed");
      return TD_ERR_LAUNCH;
    }
    WgradXcdIndex xi;
    memcpy(xi.start, L.start, sizeof(xi.start));
    memcpy(xi.slots, L.slots, sizeof(xi.slots));
    const bool pw = L.kernel == TD_WGRAD_KERNEL_POINTWISE;
#define TD_WGB_LAUNCH(TT)                                                                        \
  do {                                                                                           \
    if (pw) conv_wgrad_batch_kernel<TT, true><<<L.grid, L.block, 0, st>>>(dev, xi);              \
    else conv_wgrad_batch_kernel<TT, false><<<L.grid, L.block, 0, st>>>(dev, xi);                \
  } while (0)
    if (L.kernel == TD_WGRAD_KERNEL_WIDE) conv_wgrad_wide_batch_kernel<<<L.grid, L.block, 0, st>>>(dev, xi);
    else if (dtype == TD_BF16) TD_WGB_LAUNCH(u16);
    else TD_WGB_LAUNCH(float);
#undef TD_WGB_LAUNCH
    rc = check_launch("td_conv_wgrad_batch");
    if (rc) return rc;
    if (prof && (l + 1 == n_launches || launches[l + 1].phase != L.phase)) prof_end(st);
  }
  return TD_OK;
}
