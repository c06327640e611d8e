// Implicit-GEMM convolution / linear kernels for gfx950 (MI355X).
//
//   conv_gemm :  out[m][n] = epi( sum_k gather(src)[m][k] * W[n][k] )      forward (mode 0) and dgrad (mode 1)
//
// (The weight gradients, dW[n][k] += sum_m g[m][n] * gather(src)[m][k], are conv_wgrad.hip; gemm_dev.h holds the device helpers both share.)
//
// Layout: activations NHWC (rows = (n,ho,wo), channels contiguous), weights [Cout][R*S*Cin] with K
// contiguous, so both MFMA operands are read from LDS as 16-byte K-contiguous fragments.  One source,
// two element types: TD_BF16 -> v_mfma_f32_16x16x32_bf16, TD_F32 -> v_mfma_f32_16x16x4_f32 (exact fp32,
// the parity mode).  Tiles are described in BYTES along K (128 B per row per stage) so the load path is
// identical for both types.  MFMA roles are swapped (A = weights, B = activations) so every lane ends up
// with 4 consecutive output channels of one output row -> 8/16-byte NHWC stores.
//
// Replaces the torch Conv2d/Linear (+FrozenBatchNorm2d/ReLU/residual) calls of the reference hot path:
// models/backbone.py:60-70,97-98 (torchvision resnet101 body), models/tubedetr.py:80,131,134 (input_proj),
// models/transformer.py:124-125,387,441-445,613-617,643,661-667,748,764-773 and models/tubedetr.py:37-42.
#include <stdlib.h>

#include "gemm_dev.h"
#include "gemm_host.h"

#ifndef TD_BIG_XCD_CONTIG
#define TD_BIG_XCD_CONTIG 1  // conv_gemm_big8_kernel: an XCD walks a contiguous range of row tiles (0: row tile = 8 * seq + XCD; A/B builds)
#endif
namespace td {

struct GemmParams {
  const char* src;
  const char* w;
  char* out;
  td_conv_desc d;
  int M, K;
  uint32_t src_bytes, w_bytes;
  unsigned long long* dbg;  // optional per-workgroup cycle stamps (tools/stamp_conv.py)
  const float* bias;
  const char* residual;
  const char* mask_src;
  int relu, sigmoid;
  float alpha;
  uint32_t drop_thresh;
  float drop_scale;
  uint32_t seed;
  const uint32_t* seed_dev;
  // td_linear_ex (GX instances): the activation operand is [ A1[a1_map[m]] (K1 columns) | A2[a2_map[m]] (K - K1 columns) ]
  const char* src2;
  uint32_t src2_bytes;
  int K1, lda1, lda2, ldr;
  int w_shared;  // 1: wmat is [N][K1] and multiplies BOTH sources (= (A1 + A2) W^T without a [W | W] copy)
  const int* a1_map;
  const int* a2_map;
  const int* out_map;
  const int* res_map;
  int tap_inner;  // 256-row tile kernel, spatial layers: walk the K axis channel-chunk-major (all taps of one 64-channel chunk, then the next chunk)
  int w_ld;       // row stride of wmat in elements when it is not K (a launch that uses a subset of the columns of a larger matrix); 0 = K
  int wtap[4];    // tap-uniform instances with use_wtap: tap t of this launch reads weight columns wtap[t] * C .. (the tap's block in the larger matrix)
  int use_wtap;
};

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + __expf(-x)); }

// Main loop: operands go HBM -> LDS directly (buffer_load_dwordx4 ... lds, 1 KiB = 8 rows x 128 B per wave
// instruction, no VGPR staging).  The LDS image is row-major with the 16-byte chunk index XOR-swizzled by
// (row & 7): the DMA destination is lane-linear, so the swizzle is applied to the per-lane SOURCE address and
// again on the fragment read.  Out-of-image taps, rows >= M, channels >= Nc and the K tail are given an
// out-of-range buffer offset, which the hardware returns as zeros - no divergent control flow in the loop.
//
// NST = 2: two stages, one tile in flight (compute-bound shapes).  NST = 3: three stages and COUNTED waits - at each
// step only the oldest tile is waited for (s_waitcnt vmcnt(#DMA per tile) + raw s_barrier), the next one stays in
// flight across the barrier, and the residual / mask operands of the epilogue are requested before the K loop - for
// the short-K, HBM-bound 1x1 layers whose per-workgroup latency chain would otherwise be 5-6 exposed round trips.
// PW = pointwise (1x1, stride 1, no padding, dense output rows): the gather degenerates to row m at offset m*K, so all
// the (n,ho,wo)/(r,s,c) index arithmetic is compiled out.
// TU = tap-uniform tiles: a spatial conv whose channel count is a multiple of the K tile (C % BK == 0; every 3x3 of the
// trunk) - all 8 chunks of a tile row then belong to ONE filter tap, so the tap, its validity and its pixel offset are
// wave-uniform scalars that advance once per tile, and a DMA address is (row base + tap offset) * C + channel: a shift, an
// and, a multiply-add and a select per instruction instead of ~20 VALU operations of per-lane (r, s, c) decomposition and
// bounds tests.  Which taps fall inside the image is a per-row bit mask computed once per workgroup.  Forward geometry with
// any stride, or input-gradient geometry with stride 1.
// GX = gather-extended pointwise operand (td_linear_ex): the K axis is the concatenation of TWO row-major sources - columns
// < K1 from A1, the rest from A2 (K1 a multiple of the K tile: a tile never straddles the seam, the choice is wave-uniform) -
// each read through an optional row index (a1_map / a2_map), the result row and the residual row through out_map / res_map.
// That is how "x + pos" enters the Q/K projections without being formed ([x | pos] [W | W]^T = (x + pos) W^T,
// models/transformer.py:637-640, 735-737) and how the temporal replication (:393-427) is an index inside its consumers.
template <typename T, int BM, int BN, int NST, bool PW, bool TU = false, bool GX = false>
// (three 24-KiB stages of a 64 x 128 tile = 72 KiB: two workgroups per CU, so that is what the NST == 3 instances declare)
__global__ __launch_bounds__(256, (BM * BN >= 128 * 128 || NST == 3) ? 2 : 3) void conv_gemm_kernel(GemmParams p) {
  static_assert(!(PW && TU), "pointwise layers have no taps");
  static_assert(!GX || (PW && NST == 2), "the gather-extended operand is a pointwise, two-stage instance");
  constexpr int ES = sizeof(T);
  constexpr int VEC = 16 / ES;   // elements per 16-byte chunk
  constexpr int BK = 128 / ES;   // K elements per tile (128 bytes per row)
  constexpr int AI = BM / 32, BI = BN / 32;   // 8-row groups per wave
  constexpr int WM = BM / 2, WN = BN / 2;
  constexpr int TM = WM / 16, TN = WN / 16;
  constexpr uint32_t OOB = 0xFFFFFFF0u;
  // two distinct LDS objects (one per pipeline stage): LDS lowering then tags their accesses with disjoint alias
  // scopes, so fragment reads of one stage do not wait (vmcnt) for the DMA that is filling the other stage.
  __shared__ __attribute__((aligned(16))) char smem0[(BM + BN) * 128];
  __shared__ __attribute__((aligned(16))) char smem1[(BM + BN) * 128];
  __shared__ __attribute__((aligned(16))) char smem2[NST == 3 ? (BM + BN) * 128 : 16];

  const td_conv_desc& d = p.d;
  const int t = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  // 1-D grid; consecutive workgroup ids go round-robin over the 8 XCDs (one L2 each), so M tiles are dealt to XCDs
  // and every XCD walks all N tiles of its M tile back to back: the activation tile is re-read from that XCD's L2.
  const int NT = (d.Nc + BN - 1) / BN;
  const int xcd = blockIdx.x & 7, seq = blockIdx.x >> 3;
  const int mt = (seq / NT) * 8 + xcd, nt = seq - (seq / NT) * NT;
  const int m0 = mt * BM, n0 = nt * BN;
  if (m0 >= p.M) return;
  const int lrow = lane >> 3;                 // row inside an 8-row group
  const int chunk = (lane & 7) ^ lrow;        // source chunk that lands in LDS slot (lane & 7) of that row
  const int HoWo = d.Ho * d.Wo;

  const __amdgpu_buffer_rsrc_t rs_src = __builtin_amdgcn_make_buffer_rsrc((void*)p.src, 0, p.src_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, p.w_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_src2 = __builtin_amdgcn_make_buffer_rsrc((void*)(GX ? p.src2 : p.src), 0, GX ? p.src2_bytes : p.src_bytes, 0x00020000);

  // per-lane row bookkeeping (fixed for the whole K loop)
  int a_img[AI], a_hb[AI], a_wb[AI];
  bool a_ok[AI];
  uint32_t a_off[AI];
  uint32_t a_off2[GX ? AI : 1];  // GX: byte offset of this lane's row in the second source
  int a_base[AI];        // TU: pixel index of tap (0, 0) of this row (may be negative: only used for taps inside the image)
  uint32_t a_mask[AI];   // TU: bit (r*S + s) set = tap (r, s) of this row lies inside the image
  const int RS = d.R * d.S;
#pragma unroll
  for (int i = 0; i < AI; ++i) {
    int m = m0 + (i * 4 + wave) * 8 + lrow;
    a_ok[i] = m < p.M;
    if constexpr (GX) {
      const int mm = a_ok[i] ? m : 0;
      const int r1 = p.a1_map ? p.a1_map[mm] : mm;
      const int r2 = p.a2_map ? p.a2_map[mm] : mm;
      a_off[i] = a_ok[i] ? (uint32_t)r1 * (uint32_t)p.lda1 * ES : OOB;
      a_off2[i] = (a_ok[i] && p.src2) ? (uint32_t)r2 * (uint32_t)p.lda2 * ES : OOB;
    } else if constexpr (PW) {
      a_off[i] = a_ok[i] ? (uint32_t)m * (uint32_t)p.K * ES : OOB;
    } else {
      int mm = a_ok[i] ? m : 0;
      int n = mm / HoWo;
      int rem = mm - n * HoWo;
      int ho = rem / d.Wo, wo = rem - ho * d.Wo;
      a_img[i] = n * d.Hs * d.Ws;
      if (d.mode == 0) {
        a_hb[i] = ho * d.stride - d.pad;
        a_wb[i] = d.aniso ? wo * d.stride_w - d.pad_w : wo * d.stride - d.pad;  // (aniso: forward geometry of the generic path only)
      } else {
        a_hb[i] = ho + d.pad;
        a_wb[i] = wo + d.pad;
      }
      if constexpr (TU) {
        a_base[i] = a_img[i] + a_hb[i] * d.Ws + a_wb[i];
        uint32_t msk = 0;
        for (int r = 0; r < d.R; ++r) {
          const int hs = d.mode == 0 ? a_hb[i] + r : a_hb[i] - r;
          for (int sx = 0; sx < d.S; ++sx) {
            const int ws = d.mode == 0 ? a_wb[i] + sx : a_wb[i] - sx;
            const bool in = (unsigned)hs < (unsigned)d.Hs && (unsigned)ws < (unsigned)d.Ws;
            msk |= (in ? 1u : 0u) << (r * d.S + sx);
          }
        }
        a_mask[i] = a_ok[i] ? msk : 0u;
      }
    }
  }
  uint32_t b_off[BI];
#pragma unroll
  for (int i = 0; i < BI; ++i) {
    int n = n0 + (i * 4 + wave) * 8 + lrow;
    b_off[i] = n < d.Nc ? (uint32_t)n * (uint32_t)(p.w_ld ? p.w_ld : ((GX && p.w_shared) ? p.K1 : p.K)) * ES : OOB;
  }
  // running decomposition of this lane's k index into (r, s, c)
  int kk = chunk * VEC;
  int kr = 0, ks_ = 0, kc = kk;
  if constexpr (!PW && !TU) {
    if (d.R * d.S > 1) {
      int tap = kk / d.C;
      kc = kk - tap * d.C;
      kr = tap / d.S;
      ks_ = tap - kr * d.S;
    }
  }
  // TU: wave-uniform tile position (tap, channel base, pixel offset of the tap); the lane only contributes its chunk
  int t_tap = 0, t_ks = 0, t_kc = 0, t_pix = 0;
  int k_tile0 = 0;  // first column of the tile being issued (wave-uniform; GX picks the source by it)
  const int lane_c = chunk * VEC;

  auto issue_tile = [&](char* stage) {
    char* stA = stage;
    char* stB = stage + BM * 128;
    const bool kvalid = TU ? (t_tap < RS) : (kk < p.K);
#pragma unroll
    for (int i = 0; i < AI; ++i) {
      uint32_t off;
      if constexpr (TU) {
        const bool ok = kvalid && ((a_mask[i] >> (t_tap & 31)) & 1u);
        off = ok ? (uint32_t)((a_base[i] + t_pix) * d.C + t_kc + lane_c) * ES : OOB;
      } else if constexpr (GX) {
        // k_tile0 (wave-uniform) is the tile's first column: below K1 the whole tile comes from A1, else from A2
        if (k_tile0 >= p.K1) {
          off = (kvalid && a_off2[i] != OOB) ? a_off2[i] + (uint32_t)(kk - p.K1) * ES : OOB;
          __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_src2, (lds_ptr_t)(stA + (i * 4 + wave) * 1024), 16, off, 0, 0, 0);
          continue;
        }
        off = (kvalid && a_off[i] != OOB) ? a_off[i] + (uint32_t)kk * ES : OOB;
      } else if constexpr (PW) {
        off = (kvalid && a_ok[i]) ? a_off[i] + (uint32_t)kk * ES : OOB;
      } else {
        int hs, ws;
        bool ok = a_ok[i] && kvalid;
        if (d.mode == 0) {
          hs = a_hb[i] + kr;
          ws = a_wb[i] + ks_;
        } else {
          int th = a_hb[i] - kr, tw = a_wb[i] - ks_;
          ok = ok && th >= 0 && tw >= 0;
          if (d.stride == 1) {
            hs = th; ws = tw;
          } else if (d.stride == 2) {
            ok = ok && (((th | tw) & 1) == 0);
            hs = th >> 1; ws = tw >> 1;
          } else {
            ok = ok && (th % d.stride == 0) && (tw % d.stride == 0);
            hs = th / d.stride; ws = tw / d.stride;
          }
        }
        ok = ok && (unsigned)hs < (unsigned)d.Hs && (unsigned)ws < (unsigned)d.Ws;
        off = ok ? ((uint32_t)(a_img[i] + hs * d.Ws + ws) * (uint32_t)d.C + (uint32_t)kc) * ES : OOB;
      }
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_src, (lds_ptr_t)(stA + (i * 4 + wave) * 1024), 16, off, 0, 0, 0);
    }
    int kw = (GX && p.w_shared && k_tile0 >= p.K1) ? kk - p.K1 : kk;  // shared weight: the second source re-reads the same columns
    if constexpr (TU) {
      if (p.use_wtap) kw = p.wtap[t_tap & 3] * d.C + t_kc + lane_c;  // the tap's column block in the larger matrix (wave-uniform choice)
    }
#pragma unroll
    for (int i = 0; i < BI; ++i) {
      uint32_t off = (kvalid && b_off[i] != OOB) ? b_off[i] + (uint32_t)kw * ES : OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (lds_ptr_t)(stB + (i * 4 + wave) * 1024), 16, off, 0, 0, 0);
    }
    // advance this lane's k by one tile
    kk += BK;
    k_tile0 += BK;
    if constexpr (TU) {
      t_kc += BK;
      if (t_kc >= d.C) {  // next tap (C is a multiple of BK: a tile never straddles two taps)
        t_kc = 0;
        ++t_tap;
        if (++t_ks == d.S) { t_ks = 0; t_pix += d.mode == 0 ? d.Ws - (d.S - 1) : -(d.Ws - (d.S - 1)); }
        else t_pix += d.mode == 0 ? 1 : -1;
      }
    } else if constexpr (!PW) {
      kc += BK;
      if (d.R * d.S > 1) {
        while (kc >= d.C) {
          kc -= d.C;
          if (++ks_ == d.S) { ks_ = 0; ++kr; }
        }
      }
    }
  };

  const int wy = wave >> 1, wx = wave & 1;
  const int lr = lane & 15, lg = lane >> 4;

  f32x4 acc[TN][TM];
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < TM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto compute_tile = [&](const char* stage) {
    const char* stA = stage;
    const char* stB = stage + BM * 128;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int cidx = ks * 4 + lg;
      uint4 af[TM], wf[TN];
#pragma unroll
      for (int j = 0; j < TM; ++j) {
        int row = wy * WM + j * 16 + lr;
        af[j] = *(const uint4*)(stA + row * 128 + ((cidx ^ (row & 7)) << 4));
      }
#pragma unroll
      for (int i = 0; i < TN; ++i) {
        int row = wx * WN + i * 16 + lr;
        wf[i] = *(const uint4*)(stB + row * 128 + ((cidx ^ (row & 7)) << 4));
      }
#pragma unroll
      for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) Mfma<T>::run(wf[i], af[j], acc[i][j]);
    }
  };

  // ---- epilogue operands (defined before the K loop so NST == 3 can request them early) ----
  // The accumulators (4 consecutive channels of 16 different rows per lane) are transposed through LDS - each wave
  // owns a [WM][WN] fp32 region of the idle stage buffers, 16-byte chunks XOR-swizzled by the row - so that every
  // lane then owns 16 bytes of ONE output row (8 bf16 / 4 fp32 channels): residual / mask loads and the output
  // stores are dwordx4 over whole contiguous row segments (stores are issue-bound per instruction, not per byte).
  constexpr int CPRW = WN / 4;          // 16-byte fp32 chunks per staged row
  constexpr int EPL = 16 / ES;          // output elements per lane per row: 8 (bf16) / 4 (fp32)
  constexpr int LPR = WN / EPL;         // lanes per output row segment
  constexpr int RPI = 64 / LPR;         // rows handled per wave instruction
  constexpr int NIT = WM / RPI;
  static_assert(2 * WM * WN * 4 <= (BM + BN) * 128, "staging region does not fit the stage buffer");
  const int cc = lane % LPR, rsub = lane / LPR;
  const int n = n0 + wx * WN + cc * EPL;
  const bool vec_ok = ((d.ldc % EPL) == 0) && (!GX || (p.ldr % EPL) == 0) && (n + EPL - 1 < d.Nc);
  size_t offs[NIT];
  size_t roffs[GX ? NIT : 1];  // GX: element offset of the residual row (its own row map and row stride)
  bool live[NIT];
  uint4 res[NIT], msk[NIT];
  // every residual / mask operand of this lane is requested in one go - 2*NIT independent 16-byte loads in flight
  // instead of a load->store chain (the output may alias the residual, so the compiler cannot hoist them itself)
  auto fetch_epilogue_operands = [&]() {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int m = m0 + wy * WM + it * RPI + rsub;
      live[it] = (m < p.M) && (n < d.Nc);
      size_t orow = live[it] ? m : 0;
      if (!PW && d.out_sp > 1) {
        int ni = (int)orow / HoWo;
        int rem = (int)orow - ni * HoWo;
        int ho = rem / d.Wo, wo = rem - ho * d.Wo;
        orow = ((size_t)ni * d.out_H + (size_t)ho * d.out_sp) * d.out_W + (size_t)wo * d.out_sp;
      }
      if constexpr (GX) {
        const size_t mm = orow;
        if (p.out_map) orow = (size_t)p.out_map[mm];
        roffs[it] = (p.res_map ? (size_t)p.res_map[mm] : orow) * (size_t)p.ldr + n;
      }
      offs[it] = orow * d.ldc + n;
      if (vec_ok && live[it]) {
        if (p.residual) res[it] = ld16(p.residual + (GX ? roffs[it] : offs[it]) * ES);
        if (p.mask_src) msk[it] = ld16(p.mask_src + offs[it] * ES);
      }
    }
  };

  const int nk = (p.K + BK - 1) / BK;
#define TD_STAMP(i) do { if (p.dbg && t == 0) p.dbg[(size_t)blockIdx.x * 8 + (i)] = __builtin_readcyclecounter(); } while (0)
  TD_STAMP(0);
  if constexpr (NST == 2) {
    issue_tile(smem0);
    for (int kt = 0; kt < nk; kt += 2) {
      __syncthreads();  // tile kt has landed in stage 0 (vmcnt(0) + barrier); all waves are done reading stage 1
      if (kt == 0) TD_STAMP(1);
      if (kt + 1 < nk) issue_tile(smem1);
      compute_tile(smem0);
      if (kt + 1 >= nk) break;
      __syncthreads();
      if (kt + 2 < nk) issue_tile(smem0);
      compute_tile(smem1);
    }
    TD_STAMP(2);
    fetch_epilogue_operands();
  } else {
    // three stages, two tiles in flight.  Every step issues exactly one tile (k tiles past the end are all-OOB = zero
    // fill, no traffic) so "tile j has landed" is always "at most AI+BI DMA instructions of this wave outstanding"; the
    // pipeline warm-up is folded into the loop (steps -2, -1 only issue) so that each stage buffer has a single static
    // DMA site and the compiler's own LDS-DMA wait counts stay exact.
#define TD_CG_STEP(cur, nxt, j)                                                     \
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(AI + BI) : "memory");                    \
  __builtin_amdgcn_s_barrier();                                                     \
  issue_tile(nxt);                                                                  \
  if ((j) >= 0) compute_tile(cur);
    for (int it = -2; it < nk; it += 3) {
      TD_CG_STEP(smem1, smem0, it)
      if (it + 1 >= nk) break;
      TD_CG_STEP(smem2, smem1, it + 1)
      if (it + 2 >= nk) break;
      TD_CG_STEP(smem0, smem2, it + 2)
    }
#undef TD_CG_STEP
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // trailing zero-fill DMAs must not land in the epilogue staging area
    TD_STAMP(2);
    fetch_epilogue_operands();
  }

  // (2) transpose the accumulators through LDS.  Raw barrier: the operand loads above stay in flight (a
  //     __syncthreads() would drain vmcnt); the fragment reads of the K loop are complete once their MFMAs issued.
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  TD_STAMP(3);
  float* stg = (float*)((wave < 2 ? smem0 : smem1) + (wave & 1) * (WM * WN * 4));
  const float alpha = p.alpha;
#pragma unroll
  for (int j = 0; j < TM; ++j) {
    const int row = j * 16 + lr;
#pragma unroll
    for (int i = 0; i < TN; ++i) {
      const int c = (i * 4 + lg) ^ (row & (CPRW - 1));
      f32x4 a = acc[i][j];
      *(float4*)(stg + row * WN + c * 4) = make_float4(a[0] * alpha, a[1] * alpha, a[2] * alpha, a[3] * alpha);
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  float bias[EPL];
#pragma unroll
  for (int r = 0; r < EPL; ++r) bias[r] = (p.bias && n + r < d.Nc) ? p.bias[n + r] : 0.f;
  TD_STAMP(4);
  const uint32_t eff_seed = effective_seed(p.seed, p.drop_thresh ? p.seed_dev : nullptr);
  // (3) row-contiguous epilogue + 16-byte stores
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    if (!live[it]) continue;
    const int row = it * RPI + rsub;
    const int sw = row & (CPRW - 1);
    float v[EPL];
#pragma unroll
    for (int q = 0; q < EPL / 4; ++q) {
      float4 f = *(const float4*)(stg + row * WN + (((cc * (EPL / 4) + q) ^ sw) * 4));
      v[4 * q + 0] = f.x + bias[4 * q + 0]; v[4 * q + 1] = f.y + bias[4 * q + 1];
      v[4 * q + 2] = f.z + bias[4 * q + 2]; v[4 * q + 3] = f.w + bias[4 * q + 3];
    }
    const size_t off = offs[it];
    if (vec_ok) {
      if (p.residual) {
        float r8[EPL];
        unpack16<T>(res[it], r8);
#pragma unroll
        for (int r = 0; r < EPL; ++r) v[r] += r8[r];
      }
      if (p.relu) {
#pragma unroll
        for (int r = 0; r < EPL; ++r) v[r] = fmaxf(v[r], 0.f);
      }
      if (p.sigmoid) {
#pragma unroll
        for (int r = 0; r < EPL; ++r) v[r] = sigmoidf_(v[r]);
      }
      if (p.mask_src) {
        float m8[EPL];
        unpack16<T>(msk[it], m8);
#pragma unroll
        for (int r = 0; r < EPL; ++r) v[r] = m8[r] > 0.f ? v[r] : 0.f;
      }
      if (p.drop_thresh) {
#pragma unroll
        for (int r = 0; r < EPL; ++r) v[r] = dropout_keep(eff_seed, (uint32_t)(off + r), p.drop_thresh) ? v[r] * p.drop_scale : 0.f;
      }
      st16(p.out + off * ES, pack16<T>(v));
    } else {
      const int cnt = min(EPL, d.Nc - n);
      for (int r = 0; r < cnt; ++r) {
        float x = v[r];
        if (p.residual) x += Elem<T>::load(p.residual, (GX ? roffs[it] : off) + r);
        if (p.relu) x = fmaxf(x, 0.f);
        if (p.sigmoid) x = sigmoidf_(x);
        if (p.mask_src) x = Elem<T>::load(p.mask_src, off + r) > 0.f ? x : 0.f;
        if (p.drop_thresh) x = dropout_keep(eff_seed, (uint32_t)(off + r), p.drop_thresh) ? x * p.drop_scale : 0.f;
        Elem<T>::store(p.out, off + r, x);
      }
    }
  }
  TD_STAMP(5);
#undef TD_STAMP
}

// ------------------------------------------------------------------------------------------------
// 256-row tiles for the MFMA-bound layers (bf16; every 3x3 of layer2..4, the 1x1 layers with K >= 512), forward and input
// gradient.  Why a second instance next to conv_gemm_kernel: a 128 x 128 x 64 tile moves 32 KiB HBM/L2 -> LDS per 512 MFMA cycles of
// the CU, i.e. it needs the full 64 B/clk/CU of the vector-memory path to keep the matrix pipes busy, and measured it sits at a
// third of both.  Here one workgroup of EIGHT wavefronts (two per SIMD, the only workgroup of its CU: 2 x 64 KiB stages) owns a
// 256 x 256 (conv_gemm_big8_kernel) or 256 x 128 (conv_gemm_big8n_kernel) tile: the same DMA instruction count per wavefront and
// tile feeds twice the MFMAs (32 B/clk/CU at peak), the activation rows of a 256-channel layer are read exactly once, and each
// wavefront's 128 x 64 sub-tile needs 12 KiB of LDS fragment reads per 32 MFMAs instead of 16.  Accumulators: 128 VGPRs per lane.
// (Measured and dropped: FOUR wavefronts with 128 x 128 sub-tiles and 256 AGPR-pinned accumulators each - 192 instead of 256 KiB of
// LDS traffic per K tile - ran the layer3 3x3 forward in 602 us against 493 us: one wavefront per SIMD cannot cover its own LDS
// and barrier latencies.)  TU / pointwise addressing exactly as in conv_gemm_kernel.
//
// The main loop is PHASED (round 4).  Its round-3 predecessor kept the eight wavefronts in lock step: once per K tile every
// wavefront issued its 8 DMA pieces and their address arithmetic back to back, then drained its own DMA (vmcnt(0)) in front of the
// tile's one barrier - both SIMD-resident wavefronts away from the matrix pipe at the same moment (2840 cycles per K tile measured
// against 2 x 64 MFMAs x 17 = 2176; removed in round 5, the phased kernels were bit-identical to it).  Here
//   * the wavefronts form two groups (0-3 / 4-7: one wavefront of each group per SIMD) that run the same instruction stream ONE
//     BARRIER APART: a K tile is four phases of { load section | barrier | 16 MFMAs | barrier }, so while one group multiplies the
//     other one reads its fragments and issues DMA - matrix beside memory on every SIMD, never matrix beside matrix;
//   * DMA pieces are spread over the phases, two per wavefront and phase, and run 4-6 phases (about two K tiles) ahead of their
//     first use; a load section ends with a COUNTED s_waitcnt vmcnt(7..10) that retires exactly the pieces the next phase reads
//     and leaves everything younger in flight across the barriers - vmcnt(0) does not occur in the loop;
//   * what is in flight lands in LDS regions whose last reader finished at least two barrier intervals earlier: the weight
//     fragments of a tile are read once (phase 0) into 32 registers, so the weight half of a stage is free for tile kt + 2 from
//     phase 2 of tile kt on; the activation rows are consumed a quarter per phase (the wavefront's M fragments 2q, 2q + 1), and
//     tile kt + 1's quarters go into the other stage during phases 0 and 1;
//   * s_setprio(1) around each MFMA cluster (the groups are in different roles at any time, so the arbiter has something to prefer).
// Fragment reads are inline asm: the compiler's wait-count pass would put a vmcnt in front of any LDS read that may alias an
// LDS-DMA in flight (here: always), i.e. re-serialise the loop; with asm reads it sees no LDS read in the loop and the
// ordering is the counted waits + barriers written out below.  Ordering rules used (MI355X_MICROARCH.md, "Two waves per SIMD" 7):
// RAW - the issuing wavefront's vmcnt, then a barrier, then the read (one phase later for either group); WAR - a region is
// re-staged no earlier than two barrier intervals after its last read was issued (the reads are retired by the lgkmcnt(0) right
// behind the next barrier).  Tiles past the end of K are issued with out-of-range offsets (zero fill, no traffic) so that the
// counts are the same in every iteration.  (TD_ABL, this kernel's timing ablations, is defined in gemm_dev.h next to lds_read16, which reads it.)
#ifndef TD_BIG8_AUX_W
#define TD_BIG8_AUX_W 0  // cache-policy bits of the weight / activation LDS-DMA loads of conv_gemm_big8_kernel (A/B builds: 2 = nt)
#endif
#ifndef TD_BIG8_AUX_X
#define TD_BIG8_AUX_X 0
#endif
template <bool TU, bool RES>  // RES: a residual operand in the epilogue (rare on this instance - the K = 512 expansions of layer4 -: its own instantiation keeps the loads out of everybody else's epilogue)
__global__ __launch_bounds__(512, 1) void conv_gemm_big8_kernel(GemmParams p) {
  using T = u16;
  constexpr int ES = 2, BM = 256, BN = 256, BK = 64, NW = 8, VEC = 8;
  constexpr int WM = 128, WN = 64, TM = 8, TN = 4;
  constexpr int STAGE = (BM + BN) * 128, WREG = BM * 128;  // one stage: activation rows, then weight rows (128 B per row)
  constexpr uint32_t OOB = 0xFFFFFFF0u;
  constexpr int MAXT = 160;  // K tiles + 4 look-ahead / round-up entries (host: K <= 64 * (MAXT - 4))
  constexpr int STG = 16 * WN * ES;  // output transposition staging per wavefront: 16 rows x 64 channels of bf16 (2 KiB)
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
  __shared__ __attribute__((aligned(16))) uint4 ktab[MAXT];  // per K tile: {activation byte offset of the tile's tap / columns, tap, weight byte offset, in-range mask}
  __shared__ __attribute__((aligned(16))) char stg_all[NW * STG];  // (its own 16 KiB: the stage buffers take the NEXT tile's first pieces while this one is stored)

  const td_conv_desc& d = p.d;
  const int t = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const int NT = d.Nc / BN;
  const int lrow = lane >> 3;
  const int chunk = (lane & 7) ^ lrow;
  const int HoWo = d.Ho * d.Wo;
  const __amdgpu_buffer_rsrc_t rs_src = __builtin_amdgcn_make_buffer_rsrc((void*)p.src, 0, p.src_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, p.w_bytes, 0x00020000);
  const uint32_t out_bytes = (uint32_t)p.M * (uint32_t)d.ldc * ES;  // (host: M * ldc < 2^31)
  const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc((void*)p.out, 0, out_bytes, 0x00020000);
  const int wy = wave >> 2, wx = wave & 3;  // wy is also the wavefront's group
  const int RS = d.R * d.S;
  const int lane_c = chunk * VEC;
  // The K walk is a TABLE in LDS, built once per workgroup: entry t = where tile t's 64 columns come from.  (As a running
  // (tap, channel, pixel) state advanced in the loop it was ~35 dependent scalar instructions per advance, two advances per tile:
  // 2697 -> 2239 cycles per K tile with the advance compiled out, tools/build_variant.sh abl1 - the scalar unit issues into the
  // same in-order stream as the wavefront's MFMAs.)  Tile order: tap-inner = all R*S taps of one 64-channel chunk back to back
  // (the workgroup's window stays L2-resident), else tap-major; pointwise: columns t*64.  Entries past K are marked invalid.
  const int nk = p.K / BK;
  const bool tap_inner = TU && p.tap_inner;
  if (t < nk + 4) {  // (the loop runs an even number of tiles and looks two ahead)
    uint32_t xo, tap = 0, wo;
    if constexpr (TU) {
      const int cpt = d.C / BK;
      const int chunkc = tap_inner ? t / RS : t % cpt;
      tap = tap_inner ? t - chunkc * RS : t / cpt;
      const int r = (int)tap / d.S, sx = (int)tap - r * d.S;
      const int pix = d.mode == 0 ? r * d.Ws + sx : -(r * d.Ws + sx);
      xo = (uint32_t)(pix * d.C + chunkc * BK) * ES;
      wo = (uint32_t)((int)tap * d.C + chunkc * BK) * ES;
    } else {
      xo = wo = (uint32_t)t * BK * ES;
    }
    ktab[t] = make_uint4(xo, t < nk ? tap : 0u, wo, t < nk ? 0xFFFFFFFFu : 0u);
  }
  // PERSISTENT, with the next tile's first pieces in flight under this tile's epilogue (round 5).  The workgroup walks output tiles
  // vb = blockIdx.x, + gridDim.x, ... (the host launches one workgroup per CU when there are more tiles than CUs; gridDim.x is a
  // multiple of 8, so a workgroup stays on its XCD's share of the rows).  What the 100 MHz wall clock said about the one-tile-per-
  // workgroup form (tools/stamp_occupancy.py, tools/stamp_big.py; layer3 3x3, 800 frames, 62 us per tile and CU): K loop 50 us; per-
  // lane row decoding with integer divisions and a test per tap ~4 us; landing time of the first pieces 2.2 us; epilogue 4.9 us
  // (fp32 transposition in 16-row chunks through the stage buffers, two lgkmcnt(0) round trips per chunk) - 19 % of a tile with
  // the matrix pipe idle.  Now: rows decoded with reciprocal multiplications; the accumulators leave through a wavefront-private
  // 2-KiB bf16 staging region (bias / ReLU / rounding applied in the MFMA layout, 8-byte writes, 16-byte reads, both bank-conflict
  // free under the chunk ^ row swizzle; DS operations of a wavefront execute in order, so no wait separates a chunk's reads from
  // the next chunk's writes), and the twelve pieces of the NEXT tile's prologue are issued BEFORE the epilogue starts.
#if TD_ABL & 16  // (with 2: no LDS-DMA, but the stage buffers hold pseudo-random bf16 values around 1.0 - the matrix pipes then toggle as on real data)
  for (int i = t; i < 2 * STAGE / 4; i += 512) ((uint32_t*)smem)[i] = 0x3F803F80u ^ (mix32((uint32_t)i * 0x9E3779B1u + blockIdx.x) & 0x007F007Fu);
#endif
  const int nvb = 8 * ((cdiv(p.M, BM) + 7) / 8) * NT;
  const float rcp_howo = 1.f / (float)HoWo, rcp_wo = 1.f / (float)d.Wo;
  auto divmod = [](int a, int dv, float rcp, int& q, int& r) {
    q = (int)((float)a * rcp);
    r = a - q * dv;
    const int up = r >= dv, dn = r < 0;
    q += up - dn;
    r += (dn - up) * dv;
  };
  // tile (rows m0.., columns n0..) of virtual block vb; the blocks past the last row tile (grid rounded up to 8) can only be a
  // workgroup's LAST ones
#if TD_BIG_XCD_CONTIG
  // XCD x (= vb & 7: workgroups go to XCDs round-robin, the grid is a multiple of 8) walks a CONTIGUOUS range of row tiles: neighbouring
  // row tiles of a 3x3 layer share their halo rows (2 x (W + 1) of 256 rows at W = 22: 18 %), and with row tile = 8 * seq + x every
  // one of them was fetched into two L2s (traffic 1.19x of the algorithmic bytes); now the 32 tiles an XCD has in flight are neighbours.
  const int mtx = (cdiv(p.M, BM) + 7) / 8;
  auto tile_m0 = [&](int vb) { const int seq = vb >> 3; return ((vb & 7) * mtx + seq / NT) * BM; };
  auto tile_n0 = [&](int vb) { const int seq = vb >> 3; return (seq - (seq / NT) * NT) * BN; };
  auto tile_ok = [&](int vb) { return vb < nvb && (vb >> 3) / NT < mtx && tile_m0(vb) < p.M; };
#else
  auto tile_m0 = [&](int vb) { const int seq = vb >> 3; return ((seq / NT) * 8 + (vb & 7)) * BM; };
  auto tile_n0 = [&](int vb) { const int seq = vb >> 3; return (seq - (seq / NT) * NT) * BN; };
  auto tile_ok = [&](int vb) { return vb < nvb && tile_m0(vb) < p.M; };
#endif

  // DMA piece q (0..3) of this wavefront on the activation side: tile rows xrow(q) .. + 8 = the part of QUARTER q (the rows the
  // readers consume in phase q: M fragments 2q, 2q + 1 of both row groups) that this wavefront stages
  uint32_t a_off[4];   // byte offset of the row (pointwise) / of tap (0, 0) of the row (TU; modulo 2^32)
  uint32_t a_mask[4];  // bit (tap) set = the tap lies inside the image (pointwise: bit 0 = row below M)
  uint32_t b_off[4];
  const bool small_filter = d.R <= 3 && d.S <= 3;
  const int sgn = d.mode == 0 ? 1 : -1;  // forward: tap (r, s) reads pixel (hb + r, wb + s); input gradient: (hb - r, wb - s)
  auto tile_addr = [&](int m0, int n0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int m = m0 + (wave >> 2) * WM + q * 32 + (wave & 3) * 8 + lrow;
      const bool ok = m < p.M;
      if constexpr (!TU) {
        a_off[q] = (uint32_t)m * (uint32_t)p.K * ES + (uint32_t)lane_c * ES;
        a_mask[q] = ok ? 1u : 0u;  // (the table's tap is 0 for pointwise tiles)
      } else {
        // (reciprocal multiplication + one correction step: exact for rows below 2^24, the host's condition for this instance)
        const int mm = ok ? m : 0;
        int n, rem, ho, wo;
        divmod(mm, HoWo, rcp_howo, n, rem);
        divmod(rem, d.Wo, rcp_wo, ho, wo);
        const int hb = d.mode == 0 ? ho * d.stride - d.pad : ho + d.pad;
        const int wb = d.mode == 0 ? wo * d.stride - d.pad : wo + d.pad;
        a_off[q] = (uint32_t)(n * d.Hs * d.Ws + hb * d.Ws + wb) * (uint32_t)d.C * ES + (uint32_t)lane_c * ES;
        uint32_t cols = 0, msk = 0;
        if (small_filter) {  // (uniform) at most 3 x 3 taps: no loop, no branch per tap
#pragma unroll
          for (int sx = 0; sx < 3; ++sx) cols |= (sx < d.S && (unsigned)(wb + sgn * sx) < (unsigned)d.Ws ? 1u : 0u) << sx;
#pragma unroll
          for (int r = 0; r < 3; ++r) msk |= (r < d.R && (unsigned)(hb + sgn * r) < (unsigned)d.Hs ? cols : 0u) << (r * d.S);
        } else {
          for (int sx = 0; sx < d.S; ++sx) cols |= ((unsigned)(wb + sgn * sx) < (unsigned)d.Ws ? 1u : 0u) << sx;
          for (int r = 0; r < d.R; ++r) msk |= ((unsigned)(hb + sgn * r) < (unsigned)d.Hs ? cols : 0u) << (r * d.S);
        }
        a_mask[q] = ok ? msk : 0u;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) b_off[i] = ((uint32_t)(n0 + (i * NW + wave) * 8 + lrow) * (uint32_t)p.K + (uint32_t)lane_c) * ES;  // Nc % BN == 0: always inside
  };
  // one activation piece (quarter q) / one weight piece (i) of the tile described by table entry e into `stage`; branch-free: an
  // out-of-image tap, a row past M or a tile past K becomes the out-of-range offset through an all-ones / all-zeros mask
  auto issue_x = [&](char* stage, int q, const u32x4_t& e) {
    uint32_t ok = (0u - ((a_mask[q] >> (e.y & 31)) & 1u)) & e.w;
#if TD_ABL & 32  // (timing only) activation rows fetched for tap 0 of every channel chunk only, the other taps' pieces are out-of-range (zero fill, no L2 traffic): what staging a chunk's rows ONCE for all nine taps could save at most
    ok &= e.y == 0 ? 0xFFFFFFFFu : 0u;
#endif
    uint32_t off = a_off[q] + e.x;  // a_off (TU) = byte offset of tap (0, 0) of the row (mod 2^32: may be "negative")
    off = (off & ok) | (OOB & ~ok);
#if TD_ABL & 2
    asm volatile("" ::"v"(off));
    return;
#endif
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_src, (lds_ptr_t)(stage + ((wave >> 2) * WM + q * 32 + (wave & 3) * 8) * 128), 16, off, 0, 0, TD_BIG8_AUX_X);
  };
  auto issue_w = [&](char* stage, int i, const u32x4_t& e) {
    const uint32_t off = ((b_off[i] + e.z) & e.w) | (OOB & ~e.w);
#if TD_ABL & 2
    asm volatile("" ::"v"(off));
    return;
#endif
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (lds_ptr_t)(stage + WREG + (i * NW + wave) * 1024), 16, off, 0, 0, TD_BIG8_AUX_W);
  };

  const int lr = lane & 15, lg = lane >> 4;
  f32x4 acc[TN][TM];

  // fragment read addresses (LDS byte offsets; the 16-byte chunk index is XOR-swizzled by row & 7 = lr & 7, the k-step flips bit 6)
  const uint32_t lds0 = (uint32_t)(uintptr_t)(lds_ptr_t)smem;
  const uint32_t xa0 = lds0 + (uint32_t)((wy * WM + lr) * 128 + ((lg ^ (lr & 7)) << 4));
  const uint32_t wa0 = lds0 + (uint32_t)(WREG + (wx * WN + lr) * 128 + ((lg ^ (lr & 7)) << 4));
  const uint32_t xa[2][2] = {{xa0, xa0 ^ 64u}, {xa0 + STAGE, (xa0 ^ 64u) + STAGE}};  // [stage][k-step]: the offset field of a DS instruction holds 16 bits
  const uint32_t wa[2][2] = {{wa0, wa0 ^ 64u}, {wa0 + STAGE, (wa0 ^ 64u) + STAGE}};
  u32x4_t wreg[2][TN], xreg[2][2];  // [k-step][N fragment], [M fragment of the phase][k-step]

  // table entries: tile kt in stage 0 -> ea = entry kt + 1 (its activations are staged in phases 0, 1), eb = entry kt + 2 (its weights in
  // phases 2, 3; eb is read in phase 0 of the same tile and returns with that phase's fragments); tile kt + 1 in stage 1 swaps the roles
  const uint32_t tab0 = (uint32_t)(uintptr_t)(lds_ptr_t)ktab;
  uint32_t taddr = tab0 + 2 * 16;  // entry the next tile reads
  u32x4_t ea, eb;
  // one phase of the tile in stage S
  auto phase = [&](auto S_, auto P_) {
    constexpr int S = decltype(S_)::value, P = decltype(P_)::value;
    u32x4_t& ex = S == 0 ? ea : eb;  // entry kt + 1
    u32x4_t& ew = S == 0 ? eb : ea;  // entry kt + 2
    char* const cur = smem + S * STAGE;
    char* const oth = smem + (1 - S) * STAGE;
    // ---- load section ----
    if constexpr (P == 0) {
      wreg[0][0] = lds_read16<0 * 2048>(wa[S][0]); wreg[0][1] = lds_read16<1 * 2048>(wa[S][0]);
      wreg[0][2] = lds_read16<2 * 2048>(wa[S][0]); wreg[0][3] = lds_read16<3 * 2048>(wa[S][0]);
    }
    xreg[0][0] = lds_read16<(2 * P + 0) * 2048>(xa[S][0]);
    xreg[1][0] = lds_read16<(2 * P + 1) * 2048>(xa[S][0]);
    if constexpr (P == 0) {
      wreg[1][0] = lds_read16<0 * 2048>(wa[S][1]); wreg[1][1] = lds_read16<1 * 2048>(wa[S][1]);
      wreg[1][2] = lds_read16<2 * 2048>(wa[S][1]); wreg[1][3] = lds_read16<3 * 2048>(wa[S][1]);
    }
    xreg[0][1] = lds_read16<(2 * P + 0) * 2048>(xa[S][1]);
    xreg[1][1] = lds_read16<(2 * P + 1) * 2048>(xa[S][1]);
    if constexpr (P == 0) { ew = lds_read16<0>(taddr); taddr += 16; issue_x(oth, 0, ex); issue_x(oth, 1, ex); wait_vmcnt<8>(); }
    if constexpr (P == 1) { issue_x(oth, 2, ex); issue_x(oth, 3, ex); wait_vmcnt<9>(); }
    if constexpr (P == 2) { issue_w(cur, 0, ew); issue_w(cur, 1, ew); wait_vmcnt<10>(); }
    if constexpr (P == 3) { issue_w(cur, 2, ew); issue_w(cur, 3, ew); wait_vmcnt<7>(); }
    __builtin_amdgcn_s_barrier();
    // ---- MFMA section ----
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#if !(TD_ABL & 8)
    __builtin_amdgcn_s_setprio(1);
#endif
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < TN; ++i)
          asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc[i][2 * P + j]) : "v"(wreg[ks][i]), "v"(xreg[j][ks]));  // accumulate in place
#if !(TD_ABL & 8)
    __builtin_amdgcn_s_setprio(0);
#endif
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
  };
  // prologue of a tile = the issue order of the steady state: weights of tile 0, activations of tile 0, weights of tile 1 (twelve pieces)
  auto prologue_issue = [&]() {
    u32x4_t e0 = lds_read16<0>(tab0);
    ea = lds_read16<16>(tab0);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(e0), "+v"(ea) : : "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < 4; ++i) issue_w(smem, i, e0);
#pragma unroll
    for (int q = 0; q < 4; ++q) issue_x(smem, q, e0);
#pragma unroll
    for (int i = 0; i < 4; ++i) issue_w(smem + STAGE, i, ea);
  };

  // ---- epilogue addressing.  Write side: the MFMA layout - lane (lr, lg) holds channels i * 16 + lg * 4 .. + 4 of row lr of fragment
  // (i, j): 8 bytes of bf16 at 16-byte chunk 2 i + (lg >> 1), half lg & 1.  Read side: 8 lanes x 16 bytes per 128-byte row, 8 rows per
  // pass.  Chunk index XOR (row & 7) on both sides: the 8-byte writes of a wavefront spread over all 64 banks twice (rows r / r + 8),
  // each 16-lane group of the 16-byte reads over the sixteen 16-byte slots of a 256-byte bank row. ----
  const uint32_t stg0 = (uint32_t)(uintptr_t)(lds_ptr_t)stg_all + (uint32_t)wave * STG;
  uint32_t swa[TN];
#pragma unroll
  for (int i = 0; i < TN; ++i) swa[i] = stg0 + (uint32_t)(lr * 128 + (((2 * i + (lg >> 1)) ^ (lr & 7)) << 4) + (lg & 1) * 8);
  const int cc = lane & 7, rsub = lane >> 3;
  const uint32_t sra = stg0 + (uint32_t)(rsub * 128 + ((cc ^ rsub) << 4));  // pass h: + h * 1024 (row h * 8 + rsub: the same row & 7)
  const float alpha = p.alpha;

#define TD_STAMP(i) do { if (p.dbg && t == 0) p.dbg[(size_t)vb * 8 + (i)] = __builtin_readcyclecounter(); } while (0)
  int vb = blockIdx.x;
  if (!tile_ok(vb)) return;  // (uniform)
  tile_addr(tile_m0(vb), tile_n0(vb));
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();  // the K table is complete
  prologue_issue();
#pragma unroll 1
  for (;;) {
    const int m0 = tile_m0(vb), n0 = tile_n0(vb);
    TD_STAMP(0);
    if (p.dbg && t == 0) p.dbg[(size_t)vb * 8 + 6] = wall_clock64();  // (100 MHz, the same base on every CU: workgroup timeline, tools/stamp_occupancy.py)
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
      for (int j = 0; j < TM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    taddr = tab0 + 2 * 16;
    f32x4 bs[TN];  // bias of this lane's channels in the MFMA layout: requested now, used after the K loop
#pragma unroll
    for (int i = 0; i < TN; ++i) bs[i] = p.bias ? *(const f32x4*)(p.bias + n0 + wx * WN + i * 16 + lg * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    // weights of K tile 0 and activation quarter 0 have landed (with stores of the previous tile's epilogue still in the queue the count
    // is only stricter: loads retire in order among themselves, whatever else is outstanding)
    wait_vmcnt<7>();
    __builtin_amdgcn_s_barrier();
    if (wy == 1) __builtin_amdgcn_s_barrier();  // the second group runs one barrier behind the first from here on
    TD_STAMP(1);
    // ONE loop over tile pairs and nothing else (an odd tile count is rounded up: the extra tile is zero fill without traffic) - an
    // exit in the middle of the body makes the register allocator rename the accumulators across the two halves and spill them
    const int npair = (nk + 1) / 2;
#pragma unroll 1
    for (int it = 0; it < npair; ++it) {
      phase(ic<0>{}, ic<0>{}); phase(ic<0>{}, ic<1>{}); phase(ic<0>{}, ic<2>{}); phase(ic<0>{}, ic<3>{});
      phase(ic<1>{}, ic<0>{}); phase(ic<1>{}, ic<1>{}); phase(ic<1>{}, ic<2>{}); phase(ic<1>{}, ic<3>{});
    }
    if (wy == 0) __builtin_amdgcn_s_barrier();  // pairs with the second group's last barrier: every wavefront has read its last fragments
    TD_STAMP(2);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // the trailing zero-fill DMAs have landed: the stage buffers are free
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");           // the asm MFMAs' results are read below: the hazard the compiler would pad for
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
      for (int j = 0; j < TM; ++j) asm volatile("" : "+v"(acc[i][j]));
    // (the bias registers are defined HERE, before the next tile's LDS-DMA pieces are issued: a register load still outstanding beside
    //  them would be waited for with vmcnt(0) by the compiler, i.e. together with them)
#pragma unroll
    for (int i = 0; i < TN; ++i) asm volatile("" : "+v"(bs[i]));
    const int vb_next = vb + (int)gridDim.x;
    const bool more = tile_ok(vb_next);
    if (more) {  // (uniform) the next tile's rows, and its first twelve pieces into the stage buffers every wavefront has left
      tile_addr(tile_m0(vb_next), tile_n0(vb_next));
      prologue_issue();
    }
    TD_STAMP(3);
    // ---- epilogue: 16 rows (one M fragment) at a time ----
    uint4 mk[2][2];
    auto seg_off = [&](int j, int h) -> uint32_t {  // byte offset of this lane's 16-byte output segment of row h * 8 + rsub of fragment row j
      const int m = m0 + wy * WM + j * 16 + h * 8 + rsub;
      return m < p.M ? ((uint32_t)m * (uint32_t)d.ldc + (uint32_t)(n0 + wx * WN + cc * 8)) * ES : OOB;
    };
    auto fetch_mask = [&](int j, int b) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const uint32_t off = seg_off(j, h);
        mk[b][h] = off != OOB ? ld16(p.mask_src + off) : make_uint4(0, 0, 0, 0);
      }
    };
    // fragment row j: bias / residual / ReLU / rounding in the MFMA layout, then four 8-byte writes into the staging rows
    auto put = [&](int j) {
#pragma unroll
      for (int i = 0; i < TN; ++i) {
        const f32x4 a = acc[i][j];
        float v[4] = {a[0] * alpha + bs[i][0], a[1] * alpha + bs[i][1], a[2] * alpha + bs[i][2], a[3] * alpha + bs[i][3]};
        if constexpr (RES) {  // 8 bytes per lane in the MFMA layout
          const int m = m0 + wy * WM + j * 16 + lr;
          if (m < p.M) {
            const uint2 rr = *(const uint2*)(p.residual + ((size_t)m * d.ldc + n0 + wx * WN + i * 16 + lg * 4) * ES);
            v[0] += __uint_as_float(rr.x << 16); v[1] += __uint_as_float(rr.x & 0xffff0000u);
            v[2] += __uint_as_float(rr.y << 16); v[3] += __uint_as_float(rr.y & 0xffff0000u);
          }
        }
        if (p.relu) {
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.f);
        }
        const uint32_t lo = pack_bf16x2(v[0], v[1]), hi = pack_bf16x2(v[2], v[3]);
        asm volatile("ds_write_b64 %0, %1" ::"v"(swa[i]), "v"(u32x2_t{lo, hi}) : "memory");
      }
    };
    // Pipelined over the fragment rows with ONE staging buffer: DS operations of a wavefront execute in order, so the writes of row
    // j + 1 may be issued right behind the reads of row j (which then return the old bytes), and lgkmcnt(4) - the four younger writes
    // may still be outstanding - says that those reads have returned.  The arithmetic of row j + 1 covers the LDS round trip of row j.
    if (p.mask_src) fetch_mask(0, 0);
    put(0);
    u32x4_t o0, o1;
    asm volatile("ds_read_b128 %0, %1" : "=v"(o0) : "v"(sra) : "memory");
    asm volatile("ds_read_b128 %0, %1 offset:1024" : "=v"(o1) : "v"(sra) : "memory");
#pragma unroll
    for (int j = 0; j < TM; ++j) {
      const int b = j & 1;
      if (j + 1 < TM) {
        if (p.mask_src) fetch_mask(j + 1, b ^ 1);
        put(j + 1);
        asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(o0), "+v"(o1) : : "memory");
      } else {
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(o0), "+v"(o1) : : "memory");
      }
      u32x4_t s0 = o0, s1 = o1;
      if (j + 1 < TM) {
        asm volatile("ds_read_b128 %0, %1" : "=v"(o0) : "v"(sra) : "memory");
        asm volatile("ds_read_b128 %0, %1 offset:1024" : "=v"(o1) : "v"(sra) : "memory");
      }
      if (p.mask_src) {  // ReLU mask of the producing layer (input gradients): a select on the rounded values
        float x8[8], m8[8];
        unpack16<T>(make_uint4(s0.x, s0.y, s0.z, s0.w), x8);
        unpack16<T>(mk[b][0], m8);
#pragma unroll
        for (int r = 0; r < 8; ++r) x8[r] = m8[r] > 0.f ? x8[r] : 0.f;
        const uint4 q0 = pack16<T>(x8);
        s0 = u32x4_t{q0.x, q0.y, q0.z, q0.w};
        unpack16<T>(make_uint4(s1.x, s1.y, s1.z, s1.w), x8);
        unpack16<T>(mk[b][1], m8);
#pragma unroll
        for (int r = 0; r < 8; ++r) x8[r] = m8[r] > 0.f ? x8[r] : 0.f;
        const uint4 q1 = pack16<T>(x8);
        s1 = u32x4_t{q1.x, q1.y, q1.z, q1.w};
      }
      __builtin_amdgcn_raw_buffer_store_b128(s0, rs_out, (int)seg_off(j, 0), 0, 0);  // rows past M: out-of-range offset, dropped
      __builtin_amdgcn_raw_buffer_store_b128(s1, rs_out, (int)seg_off(j, 1), 0, 0);
    }
    TD_STAMP(5);
    if (p.dbg && t == 0) p.dbg[(size_t)vb * 8 + 7] = wall_clock64();
    if (!more) break;
    vb = vb_next;
  }
#undef TD_STAMP
}

// ------------------------------------------------------------------------------------------------
// The phased main loop for 128 output channels (layer2's 3x3 layers and its conv1): 256 x 128 tiles, THREE 48-KiB stages.
// Same two wavefront groups one barrier apart, same counted waits and table walk as conv_gemm_big8_kernel; what differs:
//   * wavefront tile 64 x 64 (4 M x 2 N wavefronts), so a K tile is TWO phases of 16 MFMAs (M fragments 2p, 2p + 1);
//   * with three stages tile kt + 2 goes into the stage tile kt - 1 has left: all of its six pieces per wavefront (2 weight,
//     2 + 2 activation) are issued during tile kt - four in phase 0, two in phase 1 - into regions whose last read lies at least
//     three barrier intervals back; every piece has four phases of lead;
//   * waits: before phase 0 of a tile vmcnt(8), before phase 1 vmcnt(10) (the pieces issued since the needed one);
//   * the loop is unrolled over three tiles (stage = compile-time constant); the table entry that drives the pieces of tile
//     T + 2 is read in phase 1 of tile T - 1 and returns with that phase's fragments.
template <bool TU>
__global__ __launch_bounds__(512, 1) void conv_gemm_big8n_kernel(GemmParams p) {
  using T = u16;
  constexpr int ES = 2, BM = 256, BN = 128, BK = 64, NW = 8, VEC = 8;
  constexpr int WM = 64, WN = 64, TM = 4, TN = 4;
  constexpr int WREG = BM * 128, STAGE = (BM + BN) * 128;
  constexpr uint32_t OOB = 0xFFFFFFF0u;
  constexpr int MAXT = 160;
  __shared__ __attribute__((aligned(16))) char smem[3 * STAGE];
  __shared__ __attribute__((aligned(16))) uint4 ktab[MAXT];

  const td_conv_desc& d = p.d;
  const int t = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const int NT = d.Nc / BN;
  const int xcd = blockIdx.x & 7, seq = blockIdx.x >> 3;
#if TD_BIG_XCD_CONTIG
  const int mtx = (cdiv(p.M, BM) + 7) / 8;  // an XCD takes a contiguous range of row tiles (halo rows shared in ITS L2: see conv_gemm_big8_kernel)
  const int mt = xcd * mtx + seq / NT, nt = seq - (seq / NT) * NT;
#else
  const int mt = (seq / NT) * 8 + xcd, nt = seq - (seq / NT) * NT;
#endif
  const int m0 = mt * BM, n0 = nt * BN;
  if (m0 >= p.M) return;
  const int lrow = lane >> 3;
  const int chunk = (lane & 7) ^ lrow;
  const int lane_c = chunk * VEC;
  const int HoWo = d.Ho * d.Wo;
  const int RS = d.R * d.S;
  const __amdgpu_buffer_rsrc_t rs_src = __builtin_amdgcn_make_buffer_rsrc((void*)p.src, 0, p.src_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, p.w_bytes, 0x00020000);
  const int wy = wave >> 1, wx = wave & 1;
  const int grp = wave >> 2;  // the wavefront's group (one wavefront of each group per SIMD)

  // activation piece (h, k): half h (the rows phase h consumes: M fragments 2h, 2h + 1 of every row group), this wavefront's
  // rows (wave >> 1) * 64 + h * 32 + ((wave & 1) * 2 + k) * 8 .. + 8
  uint32_t a_off[4], a_mask[4];
  const float rcp_howo = 1.f / (float)HoWo, rcp_wo = 1.f / (float)d.Wo;
  auto divmod = [](int a, int dv, float rcp, int& q, int& r) {
    q = (int)((float)a * rcp);
    r = a - q * dv;
    const int up = r >= dv, dn = r < 0;
    q += up - dn;
    r += (dn - up) * dv;
  };
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int m = m0 + (wave >> 1) * WM + (q >> 1) * 32 + ((wave & 1) * 2 + (q & 1)) * 8 + lrow;
    const bool ok = m < p.M;
    if constexpr (!TU) {
      a_off[q] = ((uint32_t)m * (uint32_t)p.K + (uint32_t)lane_c) * ES;
      a_mask[q] = ok ? 1u : 0u;
    } else {
      const int mm = ok ? m : 0;
      int n, rem, ho, wo;
      divmod(mm, HoWo, rcp_howo, n, rem);
      divmod(rem, d.Wo, rcp_wo, ho, wo);
      const int hb = d.mode == 0 ? ho * d.stride - d.pad : ho + d.pad;
      const int wb = d.mode == 0 ? wo * d.stride - d.pad : wo + d.pad;
      a_off[q] = ((uint32_t)(n * d.Hs * d.Ws + hb * d.Ws + wb) * (uint32_t)d.C + (uint32_t)lane_c) * ES;
      uint32_t cols = 0, msk = 0;
      for (int sx = 0; sx < d.S; ++sx) cols |= ((unsigned)(d.mode == 0 ? wb + sx : wb - sx) < (unsigned)d.Ws ? 1u : 0u) << sx;
      for (int r = 0; r < d.R; ++r) msk |= ((unsigned)(d.mode == 0 ? hb + r : hb - r) < (unsigned)d.Hs ? cols : 0u) << (r * d.S);
      a_mask[q] = ok ? msk : 0u;
    }
  }
  uint32_t b_off[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) b_off[i] = ((uint32_t)(n0 + (i * NW + wave) * 8 + lrow) * (uint32_t)p.K + (uint32_t)lane_c) * ES;
  const int nk = p.K / BK;
  const bool tap_inner = TU && p.tap_inner;
  if (t < nk + 6) {  // (the loop runs a multiple of three tiles and looks two ahead)
    uint32_t xo, tap = 0, wo;
    if constexpr (TU) {
      const int cpt = d.C / BK;
      const int chunkc = tap_inner ? t / RS : t % cpt;
      tap = tap_inner ? t - chunkc * RS : t / cpt;
      const int r = (int)tap / d.S, sx = (int)tap - r * d.S;
      const int pix = d.mode == 0 ? r * d.Ws + sx : -(r * d.Ws + sx);
      xo = (uint32_t)(pix * d.C + chunkc * BK) * ES;
      wo = (uint32_t)((int)tap * d.C + chunkc * BK) * ES;
    } else {
      xo = wo = (uint32_t)t * BK * ES;
    }
    ktab[t] = make_uint4(xo, t < nk ? tap : 0u, wo, t < nk ? 0xFFFFFFFFu : 0u);
  }
  auto issue_x = [&](char* stage, int q, const u32x4_t& e) {
    const uint32_t ok = (0u - ((a_mask[q] >> (e.y & 31)) & 1u)) & e.w;
    uint32_t off = a_off[q] + e.x;
    off = (off & ok) | (OOB & ~ok);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_src, (lds_ptr_t)(stage + ((wave >> 1) * WM + (q >> 1) * 32 + ((wave & 1) * 2 + (q & 1)) * 8) * 128), 16, off, 0, 0, 0);
  };
  auto issue_w = [&](char* stage, int i, const u32x4_t& e) {
    const uint32_t off = ((b_off[i] + e.z) & e.w) | (OOB & ~e.w);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, (lds_ptr_t)(stage + WREG + (i * NW + wave) * 1024), 16, off, 0, 0, 0);
  };

  const int lr = lane & 15, lg = lane >> 4;
  f32x4 acc[TN][TM];
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < TM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const uint32_t lds0 = (uint32_t)(uintptr_t)(lds_ptr_t)smem;
  const uint32_t xa0 = lds0 + (uint32_t)((wy * WM + lr) * 128 + ((lg ^ (lr & 7)) << 4));
  const uint32_t wa0 = lds0 + (uint32_t)(WREG + (wx * WN + lr) * 128 + ((lg ^ (lr & 7)) << 4));
  uint32_t xa[3][2], wa[3][2];  // [stage][k-step]
#pragma unroll
  for (int s_ = 0; s_ < 3; ++s_) {
    xa[s_][0] = xa0 + s_ * STAGE; xa[s_][1] = (xa0 ^ 64u) + s_ * STAGE;
    wa[s_][0] = wa0 + s_ * STAGE; wa[s_][1] = (wa0 ^ 64u) + s_ * STAGE;
  }
  u32x4_t wreg[2][TN], xreg[2][2];
  const uint32_t tab0 = (uint32_t)(uintptr_t)(lds_ptr_t)ktab;
  uint32_t taddr = tab0 + 3 * 16;
  u32x4_t e[3];
  // one phase of tile T in stage S: pieces of tile T + 2 (table entry e[(S + 2) % 3]) into stage (S + 2) % 3
  auto phase = [&](auto S_, auto P_) {
    constexpr int S = decltype(S_)::value, P = decltype(P_)::value, S2 = (S + 2) % 3;
    char* const nxt = smem + S2 * STAGE;
    if constexpr (P == 0) {
      wreg[0][0] = lds_read16<0 * 2048>(wa[S][0]); wreg[0][1] = lds_read16<1 * 2048>(wa[S][0]);
      wreg[0][2] = lds_read16<2 * 2048>(wa[S][0]); wreg[0][3] = lds_read16<3 * 2048>(wa[S][0]);
    }
    xreg[0][0] = lds_read16<(2 * P + 0) * 2048>(xa[S][0]);
    xreg[1][0] = lds_read16<(2 * P + 1) * 2048>(xa[S][0]);
    if constexpr (P == 0) {
      wreg[1][0] = lds_read16<0 * 2048>(wa[S][1]); wreg[1][1] = lds_read16<1 * 2048>(wa[S][1]);
      wreg[1][2] = lds_read16<2 * 2048>(wa[S][1]); wreg[1][3] = lds_read16<3 * 2048>(wa[S][1]);
    }
    xreg[0][1] = lds_read16<(2 * P + 0) * 2048>(xa[S][1]);
    xreg[1][1] = lds_read16<(2 * P + 1) * 2048>(xa[S][1]);
    if constexpr (P == 0) {
      issue_w(nxt, 0, e[S2]); issue_w(nxt, 1, e[S2]); issue_x(nxt, 0, e[S2]); issue_x(nxt, 1, e[S2]);
      wait_vmcnt<10>();  // activation half 1 of THIS tile has landed (issued since: 4 + 2 pieces of tile T + 1, 4 of tile T + 2)
    } else {
      e[S] = lds_read16<0>(taddr);  // entry T + 3: drives the pieces tile T + 1 issues
      taddr += 16;
      issue_x(nxt, 2, e[S2]); issue_x(nxt, 3, e[S2]);
      wait_vmcnt<8>();   // weights and activation half 0 of tile T + 1 have landed (issued since: its half 1, 6 pieces of tile T + 2)
    }
    __builtin_amdgcn_s_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < TN; ++i)
          asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc[i][2 * P + j]) : "v"(wreg[ks][i]), "v"(xreg[j][ks]));
    __builtin_amdgcn_s_setprio(0);
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
  };

  // ---- epilogue bookkeeping ----
  constexpr int CR = 16, NCH = WM / CR, EPL = 8, LPR = WN / EPL, RPI = 64 / LPR, NIT = CR / RPI, CPRW = WN / 4;
  const int cc = lane % LPR, rsub = lane / LPR;
  const int n = n0 + wx * WN + cc * EPL;
  uint32_t offs[2][NIT];
  bool live[2][NIT];
  uint4 res[2][NIT], msk[2][NIT];
  auto fetch_chunk = [&](int c, int b) {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int m = m0 + wy * WM + c * CR + it * RPI + rsub;
      live[b][it] = m < p.M;
      offs[b][it] = (uint32_t)min(m, p.M - 1) * (uint32_t)d.ldc + (uint32_t)n;
      if (p.residual) res[b][it] = ld16(p.residual + offs[b][it] * ES);
      if (p.mask_src) msk[b][it] = ld16(p.mask_src + offs[b][it] * ES);
    }
  };

#define TD_STAMP(i) do { if (p.dbg && t == 0) p.dbg[(size_t)blockIdx.x * 8 + (i)] = __builtin_readcyclecounter(); } while (0)
  TD_STAMP(0);
  __syncthreads();  // the K table is complete
  {
    const u32x4_t e0 = lds_read16<0>(tab0);
    const u32x4_t e1 = lds_read16<16>(tab0);
    e[2] = lds_read16<32>(tab0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    // the issue order of the steady state: per tile 2 weight pieces, activation half 0, activation half 1
    issue_w(smem, 0, e0); issue_w(smem, 1, e0); issue_x(smem, 0, e0); issue_x(smem, 1, e0); issue_x(smem, 2, e0); issue_x(smem, 3, e0);
    issue_w(smem + STAGE, 0, e1); issue_w(smem + STAGE, 1, e1); issue_x(smem + STAGE, 0, e1); issue_x(smem + STAGE, 1, e1);
    issue_x(smem + STAGE, 2, e1); issue_x(smem + STAGE, 3, e1);
  }
  wait_vmcnt<8>();  // weights and activation half 0 of tile 0 have landed
  __builtin_amdgcn_s_barrier();
  if (grp == 1) __builtin_amdgcn_s_barrier();  // the second group runs one barrier behind the first from here on
  TD_STAMP(1);
  const int ntri = (nk + 2) / 3;  // ONE loop over tile triples and nothing else (extra tiles: zero fill without traffic)
#pragma unroll 1
  for (int it = 0; it < ntri; ++it) {
    phase(ic<0>{}, ic<0>{}); phase(ic<0>{}, ic<1>{});
    phase(ic<1>{}, ic<0>{}); phase(ic<1>{}, ic<1>{});
    phase(ic<2>{}, ic<0>{}); phase(ic<2>{}, ic<1>{});
  }
  if (grp == 0) __builtin_amdgcn_s_barrier();  // pairs with the second group's last barrier
  TD_STAMP(2);
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // trailing zero-fill DMAs must not land in the staging regions below
  asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");           // the asm MFMAs' results are read below
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < TM; ++j) asm volatile("" : "+v"(acc[i][j]));
  fetch_chunk(0, 0);
  __builtin_amdgcn_s_barrier();  // every wavefront is done with the stage buffers: they become the staging regions
  TD_STAMP(3);
  float* stg = (float*)(smem + wave * (CR * WN * 4));
  const float alpha = p.alpha;
  float bias[EPL];
#pragma unroll
  for (int r = 0; r < EPL; ++r) bias[r] = p.bias ? p.bias[n + r] : 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int b = c & 1;
    {
      const int row = lr;
#pragma unroll
      for (int i = 0; i < TN; ++i) {
        const int cx = (i * 4 + lg) ^ (row & (CPRW - 1));
        const f32x4 a = acc[i][c];
        *(float4*)(stg + row * WN + cx * 4) = make_float4(a[0] * alpha, a[1] * alpha, a[2] * alpha, a[3] * alpha);
      }
    }
    if (c + 1 < NCH) fetch_chunk(c + 1, b ^ 1);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int row = it * RPI + rsub;
      const int sw = row & (CPRW - 1);
      float v[EPL];
#pragma unroll
      for (int q = 0; q < EPL / 4; ++q) {
        const float4 f = *(const float4*)(stg + row * WN + (((cc * (EPL / 4) + q) ^ sw) * 4));
        v[4 * q + 0] = f.x + bias[4 * q + 0]; v[4 * q + 1] = f.y + bias[4 * q + 1];
        v[4 * q + 2] = f.z + bias[4 * q + 2]; v[4 * q + 3] = f.w + bias[4 * q + 3];
      }
      if (p.residual) {
        float r8[EPL];
        unpack16<T>(res[b][it], r8);
#pragma unroll
        for (int r = 0; r < EPL; ++r) v[r] += r8[r];
      }
      if (p.relu) {
#pragma unroll
        for (int r = 0; r < EPL; ++r) v[r] = fmaxf(v[r], 0.f);
      }
      if (p.mask_src) {
        float m8[EPL];
        unpack16<T>(msk[b][it], m8);
#pragma unroll
        for (int r = 0; r < EPL; ++r) v[r] = m8[r] > 0.f ? v[r] : 0.f;
      }
      if (live[b][it]) st16(p.out + offs[b][it] * ES, pack16<T>(v));
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // staging reads retired before the next chunk overwrites the region
  }
  TD_STAMP(5);
#undef TD_STAMP
}

// ------------------------------------------------------------------------------------------------
// Persistent, weight-stationary instance for the HBM-bound pointwise layers with K <= 256 (bottleneck conv3 forward, conv1 input
// gradient, the encoder's 256 -> 2048 FFN layer: [M][K] x [Nc][K]^T with M in the 10^4..10^6 range).  In the tiled kernel above two
// thirds of such a workgroup's HBM -> LDS traffic is the weight tile it re-reads for every 64 rows, and with one K tile in flight per
// workgroup the chip holds too few bytes in flight to cover the HBM latency (2.9 TB/s measured).  Here two workgroups per CU keep
// their 128 x K weight tile as MFMA fragments IN REGISTERS for the whole launch and walk the 64-row M tiles of their group; the
// 128-row-of-N tiles of one M tile run on CUs of the same XCD at the same time, so the activation tile comes from HBM once per XCD.
// bf16, fused bias + residual + ReLU + mask (+ dropout) epilogue.  What bounds such a kernel is not bytes but requests in flight
// (the round-3 form, pw_resident_kernel, issued one activation tile + this tile's residual / mask rows per step and then spent the
// rest of the step - MFMAs, an accumulator transposition through the activation buffer itself, three more barriers, the stores -
// with nothing new on its way: 5.0 - 5.4 TB/s of its algorithmic bytes; removed in round 5, this kernel was bit-identical to it):
//   * the accumulator transposition has its own 4 KiB per wavefront (16 rows at a time; 2 x 32 KiB slots + 16 KiB = 80 KiB: still
//     two workgroups per CU), so the activation slot of tile t is free right after the barrier that follows its MFMAs: tile t + 2
//     is requested into it BEFORE the epilogue of tile t - two activation tiles in flight on a two-slot ring;
//   * residual / mask rows are requested ONE TILE AHEAD into a second register set (inline-asm loads with counted waits; the
//     compiler's own bookkeeping across the loop back edge would drain the queue), except for the residual + mask instances with
//     K = 256, whose 128 weight-fragment registers leave no room: they request this tile's rows before the MFMAs;
//   * two barriers per step.
// (Measured and dropped: the LDS-free epilogue of v_permlane16_swap - it stores 16 rows x 64 bytes per instruction instead of
// 8 rows x 128: 4.0 instead of 5.3 TB/s on the layer3 conv3 shape.  Half-line requests are what an HBM-bound kernel cannot afford.)
// Counted waits are derived from LOADS only (loads retire in issue order among themselves; stores in flight can only make a
// wait stricter).
template <int NKT, bool RES, bool MSK>
__global__ __launch_bounds__(256, 2) void pw_resident2_kernel(GemmParams p, int MT, int P) {
  using T = u16;
  constexpr int ES = 2;
  constexpr uint32_t OOB = 0xFFFFFFF0u;
  constexpr int WM = 32, WN = 64, TM = 2, TN = 4;
  constexpr int CPRW = WN / 4, EPL = 8, LPR = WN / EPL, RPI = 64 / LPR, NIT = WM / RPI;   // row-contiguous epilogue: 8 lanes x 16 bytes per 64-channel row segment
  constexpr int NOPS = NIT * ((RES ? 1 : 0) + (MSK ? 1 : 0));      // operand loads per lane and step
  constexpr bool AHEAD = NOPS > 0 && !(RES && MSK && NKT == 4);    // operand rows requested one tile ahead (register budget)
  constexpr int NA = 2 * NKT;                                      // DMA pieces per wavefront and activation tile
  constexpr int AUX_NT = (TD_NT & 2) ? 2 : 0;
  __shared__ __attribute__((aligned(16))) char sA0[32768];
  __shared__ __attribute__((aligned(16))) char sA1[32768];
  __shared__ __attribute__((aligned(16))) char sT[4 * 16 * WN * 4];  // transposition staging: 16 rows x 64 fp32 per wavefront
  const td_conv_desc& d = p.d;
  const int t = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const int NT = d.Nc >> 7;
  const int xcd = blockIdx.x & 7, local = blockIdx.x >> 3;
  const int GPX = P / NT;                      // M-tile groups per XCD
  const int nt = local % NT, gl = local / NT;
  if (gl >= GPX) return;
  const int gid = xcd * GPX + gl, G = 8 * GPX;
  const int lrow = lane >> 3, chunk = (lane & 7) ^ lrow;
  const uint32_t out_bytes = (uint32_t)p.M * (uint32_t)d.ldc * ES;  // (host: M * ldc < 2^31)
  const __amdgpu_buffer_rsrc_t rs_src = __builtin_amdgcn_make_buffer_rsrc((void*)p.src, 0, p.src_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc((void*)p.out, 0, out_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_res = __builtin_amdgcn_make_buffer_rsrc((void*)(RES ? p.residual : p.out), 0, out_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_msk = __builtin_amdgcn_make_buffer_rsrc((void*)(MSK ? p.mask_src : p.out), 0, out_bytes, 0x00020000);
  const int n0 = nt * 128;
  const int HoWo = d.Ho * d.Wo;
  const bool strided = d.stride != 1;
  auto issue_A = [&](char* buf, int mt) {
    const int m0 = mt * 64;
    uint32_t row[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int m = m0 + (i * 4 + wave) * 8 + lrow;
      int src_row = m;
      if (strided) {
        const int img = m / HoWo, rem = m - img * HoWo;
        const int ho = rem / d.Wo, wo = rem - ho * d.Wo;
        src_row = (img * d.Hs + ho * d.stride) * d.Ws + wo * d.stride;
      }
      row[i] = (mt < MT && m < p.M) ? (uint32_t)src_row * (uint32_t)p.K * ES : OOB;
    }
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const uint32_t off = row[i] != OOB ? row[i] + (uint32_t)(kt * 64 + chunk * 8) * ES : OOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_src, (lds_ptr_t)(buf + kt * 8192 + (i * 4 + wave) * 1024), 16, off, 0, 0, 0);
      }
  };
  const int wy = wave >> 1, wx = wave & 1;
  const int lr = lane & 15, lg = lane >> 4;
  const int cc = lane % LPR, rsub = lane / LPR;
  const int n = n0 + wx * WN + cc * EPL;
  float bias[EPL];
#pragma unroll
  for (int r = 0; r < EPL; ++r) bias[r] = p.bias ? p.bias[n + r] : 0.f;
  uint4 wfr[NKT][2][TN];
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i = 0; i < TN; ++i)
        wfr[kt][ks][i] = *(const uint4*)(p.w + ((size_t)(n0 + wx * WN + i * 16 + lr) * p.K + kt * 64 + ks * 32 + lg * 8) * ES);
  const uint32_t drop_seed = p.drop_thresh ? effective_seed(p.seed, p.seed_dev) : 0u;
  float* const stg = (float*)(sT + wave * (16 * WN * 4));

  // byte offset of this lane's 16-byte segment of row-iteration `it` of tile mt; rows past M / tiles past MT: out of range
  auto seg_off = [&](int mt, int it) -> uint32_t {
    const int m = mt * 64 + wy * WM + it * RPI + rsub;
    return (mt < MT && m < p.M) ? ((uint32_t)m * (uint32_t)d.ldc + (uint32_t)n) * ES : OOB;
  };
  u32x4_t res[2][NIT], msk[2][NIT];  // [register set][row iteration]
  auto fetch_ops = [&](int mt, int b) {  // inline asm: invisible to the compiler's wait-count pass, waited for by count below
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const uint32_t off = seg_off(mt, it);
      if constexpr (RES) asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen nt" : "=v"(res[b][it]) : "v"(off), "s"(rs_res) : "memory");
      if constexpr (MSK) asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen nt" : "=v"(msk[b][it]) : "v"(off), "s"(rs_msk) : "memory");
    }
  };

  // One step = tile mt in `cur`.  On entry: A(mt) and A(mt + G) are requested (in that order, into cur / nxt); with AHEAD the
  // operand rows of tile mt sit behind A(mt + G) in the queue, in register set B.
  auto step = [&](char* cur, char* nxt, int mt, auto B_) {
    constexpr int B = decltype(B_)::value;
    if constexpr (NOPS > 0 && !AHEAD) fetch_ops(mt, 0);
    // A(mt) has landed: loads younger than its last piece = A(mt + G) [NA], + the operand rows requested since
    wait_vmcnt<NA + NOPS>();
    __builtin_amdgcn_s_barrier();
    f32x4 acc[TN][TM];
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
      for (int j = 0; j < TM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int cidx = ks * 4 + lg;
        uint4 af[TM];
#pragma unroll
        for (int j = 0; j < TM; ++j) {
          const int row = wy * WM + j * 16 + lr;
          af[j] = *(const uint4*)(cur + kt * 8192 + row * 128 + ((cidx ^ (row & 7)) << 4));
        }
#pragma unroll
        for (int i = 0; i < TN; ++i)
#pragma unroll
          for (int j = 0; j < TM; ++j) Mfma<T>::run(wfr[kt][ks][i], af[j], acc[i][j]);
      }
    // every wavefront is done with the activation tile: its slot takes tile mt + 2G now, ahead of this tile's epilogue
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    issue_A(cur, mt + 2 * G);
    if constexpr (AHEAD) fetch_ops(mt + G, B ^ 1);
    // this tile's operand rows: younger loads = A(mt + 2G) [NA] (+ the rows of tile mt + G [NOPS]); without AHEAD they were
    // requested at the top of the step, ahead of nothing but A(mt + 2G)
    if constexpr (NOPS > 0) {
      wait_vmcnt<NA + (AHEAD ? NOPS : 0)>();
      __builtin_amdgcn_sched_barrier(0);
    }
    constexpr int RB = AHEAD ? B : 0;
#pragma unroll
    for (int j = 0; j < TM; ++j) {  // 16 rows at a time through the wavefront's private staging region (no workgroup barrier)
#pragma unroll
      for (int i = 0; i < TN; ++i) {
        const int c = (i * 4 + lg) ^ (lr & (CPRW - 1));
        const f32x4 a = acc[i][j];
        *(float4*)(stg + lr * WN + c * 4) = make_float4(a[0], a[1], a[2], a[3]);
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int h = 0; h < 16 / RPI; ++h) {
        const int it = j * (16 / RPI) + h;
        const int row = h * RPI + rsub;
        const int sw = row & (CPRW - 1);
        float v[EPL];
#pragma unroll
        for (int q = 0; q < EPL / 4; ++q) {
          const float4 f = *(const float4*)(stg + row * WN + (((cc * (EPL / 4) + q) ^ sw) * 4));
          v[4 * q + 0] = f.x + bias[4 * q + 0]; v[4 * q + 1] = f.y + bias[4 * q + 1];
          v[4 * q + 2] = f.z + bias[4 * q + 2]; v[4 * q + 3] = f.w + bias[4 * q + 3];
        }
        const uint32_t off = seg_off(mt, it);
        if constexpr (RES) {
          float r8[EPL];
          unpack16<T>(make_uint4(res[RB][it].x, res[RB][it].y, res[RB][it].z, res[RB][it].w), r8);
#pragma unroll
          for (int r = 0; r < EPL; ++r) v[r] += r8[r];
        }
        if (p.relu) {
#pragma unroll
          for (int r = 0; r < EPL; ++r) v[r] = fmaxf(v[r], 0.f);
        }
        if constexpr (MSK) {
          float m8[EPL];
          unpack16<T>(make_uint4(msk[RB][it].x, msk[RB][it].y, msk[RB][it].z, msk[RB][it].w), m8);
#pragma unroll
          for (int r = 0; r < EPL; ++r) v[r] = m8[r] > 0.f ? v[r] : 0.f;
        }
        if (p.drop_thresh) {  // (same element index as conv_gemm_kernel's epilogue and td_dropout: the backward regenerates this mask)
#pragma unroll
          for (int r = 0; r < EPL; ++r) v[r] = dropout_keep(drop_seed, off / ES + (uint32_t)r, p.drop_thresh) ? v[r] * p.drop_scale : 0.f;
        }
        const uint4 o = pack16<T>(v);
        __builtin_amdgcn_raw_buffer_store_b128(u32x4_t{o.x, o.y, o.z, o.w}, rs_out, (int)off, 0, AUX_NT);  // rows past M: discarded
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // staging reads retired before the next 16 rows overwrite the region
    }
  };

  int mt = gid;
  issue_A(sA0, mt);
  issue_A(sA1, mt + G);
  if constexpr (AHEAD) fetch_ops(mt, 0);
  while (mt < MT) {
    step(sA0, sA1, mt, ic<0>{});
    mt += G;
    if (mt >= MT) break;
    step(sA1, sA0, mt, ic<1>{});
    mt += G;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // trailing (out-of-range) requests must not outlive the workgroup's LDS / registers
}

}  // namespace td

using namespace td;

// ---- host side of td_conv_gemm / td_linear_ex ----
// Which kernel a call runs on is planned by gemm_route.h: a pure function of the call (descriptor, epilogue flags, dtype, CU count, knobs)
// that returns a GemmRoute, asserted case by case on the CPU through td_conv_gemm_route / td_linear_ex_route (tests/test_gemm_routes_cpu.py).
// This file fills GemmParams and launches the route: launch_route is the one place that names the instances of the four GEMM kernels.

// process-wide host state of this file and conv_wgrad.hip (gemm_host.h): the stamp-buffer hook and the dispatch knobs
static thread_local unsigned long long* g_dbg = nullptr;  // debug hook (tools/stamp_*.py): per calling thread
extern "C" int td_debug_set_stamp_buffer(unsigned long long* buf) { g_dbg = buf; return TD_OK; }
unsigned long long* td::stamp_buffer() { return g_dbg; }

// the dispatch knobs, read from the environment once per process
const GemmKnobs& td::gemm_knobs() {
  static const GemmKnobs knobs = [] {
    GemmKnobs k;
    const struct { const char* name; int* value; } vars[] = {
        {"TD_PW_PERSIST", &k.pw_persist}, {"TD_PW_PERSIST_MIN", &k.pw_persist_min}, {"TD_PW_PERSIST_DROPOUT", &k.pw_persist_dropout},
        {"TD_CONV_TAP_UNIFORM", &k.conv_tap_uniform}, {"TD_CONV_BIG", &k.conv_big}, {"TD_CONV_BIG_MIN_WG", &k.conv_big_min_wg},
        {"TD_CONV_TAP_INNER", &k.conv_tap_inner}, {"TD_CONV_BIG_PERSIST", &k.conv_big_persist}, {"TD_CONV_DEEP", &k.conv_deep},
        {"TD_DGRAD_S2_PARITY", &k.dgrad_s2_parity}, {"TD_WGRAD_BLOCKS", &k.wgrad_blocks}, {"TD_WGRAD_WIDE", &k.wgrad_wide},
        {"TD_WGRAD_WIDE_MIN_M", &k.wgrad_wide_min_m}, {"TD_WGRAD_SPLIT_STAGES", &k.wgrad_split_stages}};
    for (const auto& v : vars)
      if (const char* e = getenv(v.name)) *v.value = atoi(e);
    return k;
  }();
  return knobs;
}

static int fill_epilogue(GemmParams& p, const td_epilogue* e, const char* who) {
  p.alpha = 1.f;
  if (!e) return TD_OK;
  p.bias = e->bias;
  p.residual = (const char*)e->residual;
  p.mask_src = (const char*)e->mask_src;
  p.relu = e->relu;
  p.sigmoid = e->sigmoid;
  if (e->alpha != 0.f) p.alpha = e->alpha;
  if (e->dropout_p > 0.f) {
    TD_REQUIRE(e->dropout_p < 1.f, "%s: dropout_p must be < 1", who);
    p.drop_thresh = dropout_threshold(e->dropout_p);
    p.drop_scale = 1.f / (1.f - e->dropout_p);
    p.seed = e->dropout_seed;
    p.seed_dev = e->dropout_counter;
  }
  return TD_OK;
}

typedef void (*GemmKernel)(GemmParams);
typedef void (*PersistentKernel)(GemmParams, int, int);
template <typename T, int BM, int BN, int NST>
static GemmKernel tiled_instance(int walk) {
  switch (walk) {
    case TD_GEMM_WALK_POINTWISE: return conv_gemm_kernel<T, BM, BN, NST, true>;
    case TD_GEMM_WALK_TAP_UNIFORM: return conv_gemm_kernel<T, BM, BN, NST, false, true>;
    case TD_GEMM_WALK_GATHER: return conv_gemm_kernel<T, BM, BN, NST, false>;
    default: return conv_gemm_kernel<T, BM, BN, 2, true, false, true>;  // td_linear_ex: two stages on every tile
  }
}
template <int NKT>
static PersistentKernel persistent_instance(bool res, bool msk) {
  if (res) return msk ? pw_resident2_kernel<NKT, true, true> : pw_resident2_kernel<NKT, true, false>;
  return msk ? pw_resident2_kernel<NKT, false, true> : pw_resident2_kernel<NKT, false, false>;
}

// maps a route to its kernel instance and launches it, with the profiler's record around the launch
static int launch_route(const GemmRoute& r, GemmParams& p, hipStream_t st) {
  const bool bf16 = r.dtype == TD_BF16, tu = r.walk == TD_GEMM_WALK_TAP_UNIFORM;
  GemmKernel k = nullptr;
  PersistentKernel kp = nullptr;
  switch (r.kernel) {
    case TD_GEMM_KERNEL_PERSISTENT:
      kp = r.nkt == 1 ? persistent_instance<1>(r.res, r.msk) : r.nkt == 2 ? persistent_instance<2>(r.res, r.msk) :
           r.nkt == 3 ? persistent_instance<3>(r.res, r.msk) : persistent_instance<4>(r.res, r.msk);
      break;
    case TD_GEMM_KERNEL_BIG8:
      if (tu) k = r.res ? conv_gemm_big8_kernel<true, true> : conv_gemm_big8_kernel<true, false>;
      else k = r.res ? conv_gemm_big8_kernel<false, true> : conv_gemm_big8_kernel<false, false>;
      break;
    case TD_GEMM_KERNEL_BIG8N: k = tu ? conv_gemm_big8n_kernel<true> : conv_gemm_big8n_kernel<false>; break;
    default:
      if (r.bn == 64) k = bf16 ? tiled_instance<u16, 128, 64, 2>(r.walk) : tiled_instance<float, 128, 64, 2>(r.walk);
      else if (r.stages == 3) k = tiled_instance<u16, 64, 128, 3>(r.walk);
      else if (r.bm == 64) k = bf16 ? tiled_instance<u16, 64, 128, 2>(r.walk) : tiled_instance<float, 64, 128, 2>(r.walk);
      else k = bf16 ? tiled_instance<u16, 128, 128, 2>(r.walk) : tiled_instance<float, 128, 128, 2>(r.walk);
  }
  const bool prof = prof_on();
  if (prof) {
    prof_begin(r.family, r.dtype, 2.0 * r.M * r.N * r.K, st, r.M, r.N, r.K, r.R, r.stride, r.mode);
    prof_set_bytes(r.bytes);
  }
  if (kp) kp<<<r.grid, r.block, 0, st>>>(p, r.MTp, r.Pp);
  else k<<<r.grid, r.block, 0, st>>>(p);
  if (prof) prof_end(st);
  return check_launch(r.label);
}

// one launch of td_conv_gemm: plan it, then launch it - or, for the query, hand the plan back (no pointer is used, no device touched)
static int conv_gemm_launch(const void* src, const void* wmat, void* out, const td_conv_desc* d, const td_epilogue* e, int dtype, int n_cu,
                            const WeightSubset* sub, td_stream_t stream, td_gemm_route* report) {
  GemmRoute r;
  int rc = plan_conv_launch(d, epi_flags(e), dtype, n_cu, gemm_knobs(), sub, r);
  if (rc) return rc;
  GemmParams p;
  memset(&p, 0, sizeof(p));
  rc = fill_epilogue(p, e, "td_conv_gemm");
  if (rc) return rc;
  if (report) {
    *report = r;
    return TD_OK;
  }
  p.src = (const char*)src;
  p.w = (const char*)wmat;
  p.out = (char*)out;
  p.d = *d;
  if (p.d.out_sp < 1) p.d.out_sp = 1;
  p.M = r.M;
  p.K = r.K;
  p.src_bytes = r.src_bytes;
  p.w_bytes = r.w_bytes;
  if (sub) {
    p.w_ld = sub->w_ld;
    p.use_wtap = sub->ntap > 1;
    for (int i = 0; i < 4; ++i) p.wtap[i] = sub->wtap[i];
  }
  p.tap_inner = r.tap_inner;
  p.dbg = g_dbg;
  return launch_route(r, p, (hipStream_t)stream);
}

// the whole call: one launch, or the four parity classes of a stride-2 3x3 input gradient (gemm_route.h)
static int conv_gemm_call(const void* src, const void* wmat, void* out, const td_conv_desc* d, const td_epilogue* e, int dtype, int n_cu,
                          td_stream_t stream, td_gemm_route* report, int* n_report) {
  const bool split = conv_splits_by_parity(d, e, dtype, gemm_knobs());
  if (n_report) *n_report = split ? 4 : 1;
  if (!split) return conv_gemm_launch(src, wmat, out, d, e, dtype, n_cu, nullptr, stream, report);
  int rc = validate(d, dtype, "td_conv_gemm");
  for (int i = 0; i < 4 && !rc; ++i) {
    const ParityClass c = parity_class(d, i >> 1, i & 1);
    td_epilogue ec;
    memset(&ec, 0, sizeof(ec));
    if (e) ec = *e;
    if (ec.residual) ec.residual = (const char*)ec.residual + c.out_off;
    if (ec.mask_src) ec.mask_src = (const char*)ec.mask_src + c.out_off;
    if (report) rc = conv_gemm_launch(nullptr, nullptr, nullptr, &c.d, &ec, dtype, n_cu, &c.sub, stream, report + i);
    else rc = conv_gemm_launch(src, (const char*)wmat + c.w_off, (char*)out + c.out_off, &c.d, &ec, dtype, n_cu, &c.sub, stream, nullptr);
  }
  return rc;
}

extern "C" int td_conv_gemm(const void* src, const void* wmat, void* out, const td_conv_desc* d, const td_epilogue* e,
                            int dtype, td_stream_t stream) {
  TD_REQUIRE(src && wmat && out && d, "td_conv_gemm: null pointer");
  return conv_gemm_call(src, wmat, out, d, e, dtype, cu_count(), stream, nullptr, nullptr);
}

extern "C" int td_conv_gemm_route(const td_conv_desc* d, const td_epilogue* e, int dtype, int n_cu, td_gemm_route* routes, int* n_routes) {
  TD_REQUIRE(d && routes && n_routes, "td_conv_gemm: null pointer");
  TD_REQUIRE(n_cu >= 1, "td_conv_gemm_route: n_cu=%d", n_cu);
  return conv_gemm_call(nullptr, nullptr, nullptr, d, e, dtype, n_cu, nullptr, routes, n_routes);
}

// out[out_map[m]][n] = epilogue( [A1[a1_map[m]] | A2[a2_map[m]]] @ wmat[n][K1 + K2]^T (+ residual[res_map[m]][n]) )
static int linear_ex_call(const void* a1, const void* a2, const void* wmat, void* out, const td_linear_ex_desc* x, bool has_a2, const td_epilogue* e,
                          int dtype, td_stream_t stream, td_gemm_route* report) {
  GemmRoute r;
  int rc = plan_linear_ex(x, has_a2, epi_flags(e), dtype, r);
  if (rc) return rc;
  GemmParams p;
  memset(&p, 0, sizeof(p));
  rc = fill_epilogue(p, e, "td_linear_ex");
  if (rc) return rc;
  if (report) {
    *report = r;
    return TD_OK;
  }
  p.src = (const char*)a1;
  p.src2 = (const char*)a2;
  p.w = (const char*)wmat;
  p.out = (char*)out;
  p.M = r.M;
  p.K = r.K;
  p.K1 = x->K1;
  p.lda1 = x->lda1;
  p.lda2 = a2 ? x->lda2 : 0;
  p.ldr = x->ldr > 0 ? x->ldr : x->ldc;
  p.w_shared = (a2 && x->w_shared) ? 1 : 0;
  p.a1_map = x->a1_map;
  p.a2_map = a2 ? x->a2_map : nullptr;
  p.out_map = x->out_map;
  p.res_map = x->res_map;
  p.d.N = 1; p.d.Hs = x->M; p.d.Ws = 1; p.d.C = p.K; p.d.Ho = x->M; p.d.Wo = 1; p.d.R = p.d.S = 1; p.d.stride = 1; p.d.Nc = x->N; p.d.ldc = x->ldc; p.d.out_sp = 1;
  p.src_bytes = r.src_bytes;
  p.src2_bytes = r.src2_bytes;
  p.w_bytes = r.w_bytes;
  return launch_route(r, p, (hipStream_t)stream);
}

extern "C" int td_linear_ex(const void* a1, const void* a2, const void* wmat, void* out, const td_linear_ex_desc* x, const td_epilogue* e,
                            int dtype, td_stream_t stream) {
  TD_REQUIRE(a1 && wmat && out && x, "td_linear_ex: null pointer");
  return linear_ex_call(a1, a2, wmat, out, x, a2 != nullptr, e, dtype, stream, nullptr);
}

extern "C" int td_linear_ex_route(const td_linear_ex_desc* x, int has_a2, const td_epilogue* e, int dtype, int n_cu, td_gemm_route* routes, int* n_routes) {
  TD_REQUIRE(x && routes && n_routes, "td_linear_ex: null pointer");
  (void)n_cu;  // td_linear_ex's tile rule does not read the CU count
  *n_routes = 1;
  return linear_ex_call(nullptr, nullptr, nullptr, nullptr, x, has_a2 != 0, e, dtype, nullptr, routes);
}
