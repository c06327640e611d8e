// Shot cuts in decoded frames: td_frame_stats and td_shot_cuts (include/tubedetr_hip.h has the rules).
//
// td_frame_stats.  The sampled rows of a job are cut into UNITS of 16 pixels (16 luma bytes; 48 rgb24 bytes), numbered row after
// row.  A workgroup owns a band of 2048 (rgb24: 1024) consecutive units - 25 (13) rows of 1280 pixels - and walks it through a
// segment of consecutive frames of the job (64 of them; down to 8 in a launch of few bands, whose workgroups would be too few):
//   * lane l owns units l, l + 256, ... of the band (neighbouring lanes load neighbouring 16 bytes).  Where a unit lies in a
//     frame, which of its 16 pixels are sampled (inside the row, column % step == 0) and the LDS copy the lane counts into do not
//     depend on the frame: they are worked out once, in front of the frame loop;
//   * a frame's band is fetched once, with load_run's 16-byte global loads; the luma of the frame before stays in registers (4
//     dwords per unit, unsampled bytes zeroed), so the difference costs one v_sad_u8 per 4 pixels and no second fetch.  Only a
//     band's first frame of a segment other than the first is fetched twice (1 / 64 .. 1 / 8 of the bytes);
//   * the histogram is counted with LDS atomics into kCopies copies of the 64 bins, a lane using copy l % kCopies, the copies
//     kBins + 1 words apart: neighbouring pixels fall into the same bin, and one copy would serialise a wave on it.  The frame's
//     copies are summed once per band, four lanes per bin, and go to memory as 64 integer atomics; the lanes' differences as one.
//     Two sets of copies alternate by frame parity, so one barrier per frame is enough: a set is flushed and zeroed while the
//     other one counts;
//   * step > 1 skips whole rows, so the bytes read fall with it; inside a sampled row every byte is read and the unit's mask
//     decides which pixels count; for a step of 2, 4 or 8 the columns that no unit samples are skipped by a uniform branch.
// The outputs are zeroed by a small kernel in front (same stream, same table), then only added to: integer sums, the same bits
// on every run.  td_shot_cuts is one workgroup per job over 256 frames at a time, d staged in LDS with a halo of 16 frames.
#include "frame_jobs.h"

namespace td {

namespace {

constexpr int kUnitPx = 16;
constexpr int kLumaUnitsPerLane = 8, kRgbUnitsPerLane = 4;  // 32 KiB of luma, 48 KiB of rgb24 per band and frame
constexpr int kSegFrames = 64, kMinSegFrames = 8;  // frames that a workgroup walks: a segment but the first fetches one frame twice
constexpr int kLaunchGroups = 2048;                // a launch of few bands gets shorter segments, until it has about this many workgroups
constexpr int kBins = 64, kCopies = 32, kCopyStride = kBins + 1;
constexpr int kHistWords = kCopies * kCopyStride;  // word kHistWords of a set: the band's sum of differences
constexpr int kMaxPixels = 1 << 24;
constexpr int kMaxStatStep = 8;
constexpr int kZeroWordsPerBlock = kThreads * 16;

struct StatsParams {
  const unsigned char* src;  // plane 0: the only one that is read
  long long stride;
  uint32_t* hist;
  uint32_t* sad;
  int pitch, rgb, T, sw, step;
  int upr;      // units per row
  int n_units;  // of a frame
  int bands;    // workgroups per frame segment
  int seg;      // frames per segment
  int colmask;  // the pixels of a unit that any row samples: a unit begins at a multiple of 16, so a step of 2, 4 or 8 has ONE mask for all units
  int zero_y;   // record 0: workgroups per job of the zeroing kernel
  int block_begin;
};

__global__ __launch_bounds__(kThreads) void frame_stats_zero_kernel(const StatsParams* __restrict__ tab, int n_jobs) {
  const int zy = tab[0].zero_y;
  const int job = blockIdx.x / zy, part = blockIdx.x - job * zy;
  if (job >= n_jobs) return;
  const StatsParams* p = tab + job;
  const long long nh = (long long)kBins * p->T, n = nh + p->T;
  TD_GLOBAL uint32_t* hist = (TD_GLOBAL uint32_t*)p->hist;
  TD_GLOBAL uint32_t* sad = (TD_GLOBAL uint32_t*)p->sad;
  for (long long i = (long long)part * kThreads + threadIdx.x; i < n; i += (long long)zy * kThreads) {
    if (i < nh) { if (hist) hist[i] = 0; }
    else if (sad) sad[i - nh] = 0;
  }
}

// bits 0..3 -> 0xFF in bytes 0..3
__device__ __forceinline__ uint32_t byte_mask(uint32_t bits4) { return ((bits4 * 0x00204081u) & 0x01010101u) * 0xFFu; }

// bytes [0, n) of `at` (n < 16: the rest zero; n <= 0: none): one 16-byte load as in load_run where the address allows it, four
// dwords at a 4-byte address; the end of a row and rows at odd addresses (a tight pitch that is no multiple of 4) go byte by
// byte, in a loop that is NOT unrolled: eight units of load_run's unrolled byte path cost the frame loop its registers
__device__ __forceinline__ void load_bytes(const unsigned char* at, int n, uint32_t in[4]) {
  if (n >= kRun && ((uintptr_t)at & 15) == 0) {
    const u32x4 v = *(const TD_GLOBAL u32x4*)at;
    in[0] = v.x; in[1] = v.y; in[2] = v.z; in[3] = v.w;
  } else if (n >= kRun && ((uintptr_t)at & 3) == 0) {
#pragma unroll
    for (int k = 0; k < 4; k++) in[k] = ((const TD_GLOBAL uint32_t*)at)[k];
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      uint32_t v = 0;
      const int nb = min(n - 4 * k, 4);
#pragma nounroll
      for (int j = 0; j < nb; j++) v |= (uint32_t)((gcbyte_ptr)at)[4 * k + j] << (8 * j);
      in[k] = v;
    }
  }
}

// the luma of a unit's 16 pixels, one byte each, the bytes outside the mask zero.  `at` is the unit's first byte; mk holds the
// mask of its sampled pixels (bits 0..15) and, above it, the bytes that the row has from `at` on (at most 48).  No byte outside
// the row is read.
template <bool RGB>
__device__ __forceinline__ void load_luma(const unsigned char* at, uint32_t mk, uint32_t cur[4]) {
  asm volatile("" : "+v"(mk));  // what follows from mk is the same in every frame: hoisted out of the frame loop it would cost 4 registers per unit
  const uint32_t m16 = mk & 0xFFFFu;
  const int left = (int)(mk >> 16);
  if (m16 == 0) {
    cur[0] = cur[1] = cur[2] = cur[3] = 0;
    return;
  }
  if (!RGB) {
    load_bytes(at, left, cur);
  } else {
    uint32_t raw[12];
#pragma unroll
    for (int r = 0; r < 3; r++) load_bytes(at + kRun * r, left - kRun * r, raw + 4 * r);
    cur[0] = cur[1] = cur[2] = cur[3] = 0;
#pragma unroll
    for (int px = 0; px < kUnitPx; px++) {
      uint32_t c[3];
#pragma unroll
      for (int k = 0; k < 3; k++) c[k] = (raw[(3 * px + k) >> 2] >> (8 * ((3 * px + k) & 3))) & 255u;
      cur[px >> 2] |= ((77u * c[0] + 150u * c[1] + 29u * c[2] + 128u) >> 8) << (8 * (px & 3));
    }
  }
#pragma unroll
  for (int d = 0; d < 4; d++) cur[d] &= byte_mask((m16 >> (4 * d)) & 15u);
}

template <bool RGB>
__device__ __forceinline__ void frame_stats_band(const StatsParams* __restrict__ p, int local, uint32_t (*acc)[kHistWords + 1]) {
  constexpr int kUnitsPerLane = RGB ? kRgbUnitsPerLane : kLumaUnitsPerLane, kBandUnits = kThreads * kUnitsPerLane;
  const int tid = threadIdx.x;
  const int seg = local / p->bands, band = local - seg * p->bands;
  const int t_begin = seg * p->seg, t_end = min(t_begin + p->seg, p->T);
  const int sw = p->sw, step = p->step, row_bytes = RGB ? 3 * sw : sw;
  const bool want_hist = p->hist != nullptr, want_sad = p->sad != nullptr;
  const uint32_t colmask = (uint32_t)p->colmask;
  for (int i = tid; i < 2 * (kHistWords + 1); i += kThreads) (&acc[0][0])[i] = 0;

  // where the lane's units lie in a frame, and which of their pixels count
  long long off[kUnitsPerLane];
  uint32_t mk[kUnitsPerLane];
#pragma unroll
  for (int k = 0; k < kUnitsPerLane; k++) {
    const int i = band * kBandUnits + k * kThreads + tid;
    off[k] = 0; mk[k] = 0;
    if (i < p->n_units) {
      const int ry = i / p->upr, ux = i - ry * p->upr;
      const int o0 = ux * kUnitPx * (RGB ? 3 : 1);
      off[k] = (long long)ry * step * p->pitch + o0;
      mk[k] = (uint32_t)min(row_bytes - o0, 3 * kRun) << 16;
      const int c0 = ux * kUnitPx, n_px = min(sw - c0, kUnitPx);
#pragma nounroll
      for (int j = (step - c0 % step) % step; j < n_px; j += step) mk[k] |= 1u << j;
    }
  }
  __syncthreads();

  uint32_t prev[kUnitsPerLane][4];
#pragma unroll
  for (int k = 0; k < kUnitsPerLane; k++) prev[k][0] = prev[k][1] = prev[k][2] = prev[k][3] = 0;
  if (want_sad && t_begin > 0) {
    const unsigned char* frame = p->src + (long long)(t_begin - 1) * p->stride;
#pragma unroll
    for (int k = 0; k < kUnitsPerLane; k++) load_luma<RGB>(frame + off[k], mk[k], prev[k]);
  }

  const int copy = (tid & (kCopies - 1)) * kCopyStride;
  for (int t = t_begin; t < t_end; t++) {
    uint32_t* h = acc[t & 1];
    const unsigned char* frame = p->src + (long long)t * p->stride;
    uint32_t cur[kUnitsPerLane][4];
#pragma unroll
    for (int k = 0; k < kUnitsPerLane; k++) load_luma<RGB>(frame + off[k], mk[k], cur[k]);
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < kUnitsPerLane; k++) {
      if (want_hist && (mk[k] & 0xFFFFu) != 0) {
        uint32_t m = mk[k];
        asm volatile("" : "+v"(m));  // (as in load_luma: 16 hoisted predicates per unit would cost the frame loop its registers)
        const bool whole = (m & colmask) == colmask;  // all but a row's last unit, at steps 1, 2, 4 and 8: no test per pixel
#pragma unroll
        for (int j = 0; j < kUnitPx; j++) {
          if (!((colmask >> j) & 1u)) continue;  // uniform: a step of 2, 4 or 8 issues an eighth .. a half of the atomics
          const uint32_t L = (cur[k][j >> 2] >> (8 * (j & 3))) & 255u;
          if (whole || ((m >> j) & 1u)) atomicAdd(&h[copy + (L >> 2)], 1u);
        }
      }
      if (want_sad) {
#pragma unroll
        for (int d = 0; d < 4; d++) {
          s = __builtin_amdgcn_sad_u8(cur[k][d], prev[k][d], s);
          prev[k][d] = cur[k][d];
        }
      }
    }
    if (want_sad && t > 0) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
      if ((tid & 63) == 0 && s != 0) atomicAdd(&h[kHistWords], s);
    }
    __syncthreads();
    // flush set t & 1 and zero it; the next frame counts into the other set, and the barrier behind it orders this zeroing
    // in front of the frame after that
    if (want_hist) {
      const int bin = tid >> 2, q = tid & 3;
      uint32_t sum = 0;
#pragma unroll
      for (int c = 0; c < kCopies / 4; c++) {
        const int at = (q * (kCopies / 4) + c) * kCopyStride + bin;
        sum += h[at];
        h[at] = 0;
      }
      sum += __shfl_xor(sum, 1);
      sum += __shfl_xor(sum, 2);
      if (q == 0 && sum != 0) atomicAdd((uint32_t*)((TD_GLOBAL uint32_t*)p->hist + (long long)t * kBins + bin), sum);
    }
    if (want_sad && tid == 0) {
      const uint32_t v = h[kHistWords];
      h[kHistWords] = 0;
      if (v != 0) atomicAdd((uint32_t*)((TD_GLOBAL uint32_t*)p->sad + t), v);
    }
  }
}

__global__ __launch_bounds__(kThreads, 4) void frame_stats_kernel(const StatsParams* __restrict__ tab, int n_jobs) {
  __shared__ uint32_t acc[2][kHistWords + 1];
  const StatsParams* p = tab + find_job(tab, n_jobs, blockIdx.x);
  const int local = blockIdx.x - p->block_begin;
  if (p->rgb) frame_stats_band<true>(p, local, acc);
  else frame_stats_band<false>(p, local, acc);
}

// ---- td_shot_cuts -------------------------------------------------------------------------------------------------------------
constexpr int kMaxWindow = 16;
constexpr int kMaxCutT = 1 << 20, kMaxFrac = 1 << 20;

struct CutsParams {
  const uint32_t* hist;
  const uint32_t* sad;
  uint32_t* d;
  unsigned char* cut;
  int* shot;
  int* n_shots;
  int T, N, hist_num, hist_den, sad_num, sad_den, peak_num, peak_den, w;
};

__global__ __launch_bounds__(kThreads) void shot_cuts_kernel(const CutsParams* __restrict__ tab, int n_jobs) {
  __shared__ uint32_t dl[kThreads + 2 * kMaxWindow];
  __shared__ int scan[kThreads];
  const int tid = threadIdx.x;
  const CutsParams* p = tab + blockIdx.x;
  const int T = p->T, w = p->w;
  const TD_GLOBAL uint32_t* hist = (const TD_GLOBAL uint32_t*)p->hist;
  const unsigned long long N = (unsigned long long)p->N;
  int carry = 0;
  for (int c0 = 0; c0 < T; c0 += kThreads) {
    for (int j = tid; j < kThreads + 2 * kMaxWindow; j += kThreads) {  // d of frames c0 - 16 .. c0 + 256 + 15
      const int t = c0 - kMaxWindow + j;
      uint32_t d = 0;
      if (t >= 1 && t < T) {
        const TD_GLOBAL uint32_t* h1 = hist + (long long)t * kBins;
        const TD_GLOBAL uint32_t* h0 = h1 - kBins;
        for (int bin = 0; bin < kBins; bin++) {
          const uint32_t x = h1[bin], y = h0[bin];
          d += x > y ? x - y : y - x;
        }
      }
      dl[j] = d;
    }
    __syncthreads();
    const int t = c0 + tid;
    int c = 0;
    if (t >= 1 && t < T) {
      const unsigned long long d = dl[tid + kMaxWindow];
      const int lo = max(1, t - w), hi = min(T - 1, t + w);
      bool peak = true;
      unsigned long long sum = 0;
      for (int q = lo; q <= hi; q++) {
        if (q == t) continue;
        const unsigned long long dq = dl[q - c0 + kMaxWindow];
        sum += dq;
        peak = peak && (q < t ? dq < d : dq <= d);
      }
      const unsigned long long cnt = (unsigned long long)(hi - lo);  // |Q|: the range without t itself
      const unsigned long long sad = ((const TD_GLOBAL uint32_t*)p->sad)[t];
      const bool g1 = d * (unsigned long long)p->hist_den > (unsigned long long)p->hist_num * 2ull * N;
      const bool g2 = sad * (unsigned long long)p->sad_den > (unsigned long long)p->sad_num * N;
      const bool g4 = cnt == 0 || d * (unsigned long long)p->peak_den * cnt > (unsigned long long)p->peak_num * sum;
      c = g1 && g2 && peak && g4 ? 1 : 0;
    }
    if (t < T && p->d) ((TD_GLOBAL uint32_t*)p->d)[t] = dl[tid + kMaxWindow];
    scan[tid] = c;
    __syncthreads();
    for (int o = 1; o < kThreads; o <<= 1) {
      const int v = tid >= o ? scan[tid - o] : 0;
      __syncthreads();
      scan[tid] += v;
      __syncthreads();
    }
    if (t < T) {
      ((gbyte_ptr)p->cut)[t] = (unsigned char)c;
      ((TD_GLOBAL int*)p->shot)[t] = carry + scan[tid];
    }
    carry += scan[kThreads - 1];
    __syncthreads();
  }
  if (tid == 0) *(TD_GLOBAL int*)p->n_shots = T > 0 ? carry + 1 : 0;
}

}  // namespace

}  // namespace td

using namespace td;

extern "C" size_t td_frame_stats_table_bytes(int n_jobs) { return table_bytes<StatsParams>(n_jobs); }

extern "C" int td_frame_stats(const td_stats_job* jobs, int n_jobs, void* table_host, void* table_dev, size_t table_bytes, td_stream_t stream) {
  const char* who = "td_frame_stats";
  if (int rc = check_workspace<StatsParams>(who, jobs, n_jobs, table_host, table_dev, table_bytes)) return rc;
  StatsParams* host = (StatsParams*)table_host;
  int n = 0, max_T = 0;
  long long blocks = 0, band_frames = 0;
  for (int i = 0; i < n_jobs; i++) {
    const td_stats_job& j = jobs[i];
    TD_REQUIRE(j.fmt == TD_SRC_RGB24 || j.fmt == TD_SRC_I420 || j.fmt == TD_SRC_NV12, "%s: job %d: unknown fmt %d", who, i, j.fmt);
    TD_REQUIRE(j.T >= 0, "%s: job %d: negative frame count T = %d", who, i, j.T);
    TD_REQUIRE(j.sh > 0 && j.sw > 0 && j.sh <= kMaxSide && j.sw <= kMaxSide, "%s: job %d: sh x sw = %d x %d outside 1..%d", who, i, j.sh, j.sw, kMaxSide);
    TD_REQUIRE((long long)j.sh * j.sw <= kMaxPixels, "%s: job %d: sh * sw = %lld pixels is above %d (sad would not fit 32 bits)", who, i, (long long)j.sh * j.sw, kMaxPixels);
    TD_REQUIRE(j.step >= 1 && j.step <= kMaxStatStep, "%s: job %d: step = %d outside 1..%d", who, i, j.step, kMaxStatStep);
    TD_REQUIRE(j.hist || j.sad, "%s: job %d: hist and sad are both null", who, i);
    const PlaneGeom g = plane_geom(j.fmt, j.sh, j.sw);
    const PlaneSet set = {"src", {j.src0, j.src1, j.src2}, {j.src_pitch0, j.src_pitch1, j.src_pitch2}, j.src_frame_stride};
    if (int rc = check_planes(who, i, g, &set, 1)) return rc;
    if (j.T == 0) continue;
    StatsParams p{};
    p.src = (const unsigned char*)j.src0; p.stride = j.src_frame_stride; p.pitch = j.src_pitch0;
    p.hist = j.hist; p.sad = j.sad;
    p.rgb = j.fmt == TD_SRC_RGB24; p.T = j.T; p.sw = j.sw; p.step = j.step;
    p.colmask = j.step == 2 ? 0x5555 : j.step == 4 ? 0x1111 : j.step == 8 ? 0x0101 : 0xFFFF;
    p.upr = cdiv(j.sw, kUnitPx);
    p.n_units = cdiv(j.sh, j.step) * p.upr;
    p.bands = cdiv(p.n_units, kThreads * (p.rgb ? kRgbUnitsPerLane : kLumaUnitsPerLane));
    max_T = std::max(max_T, j.T);
    band_frames += (long long)j.T * p.bands;
    host[n++] = p;
  }
  if (n == 0) return TD_OK;
  const int seg = (int)std::min<long long>(kSegFrames, std::max<long long>(kMinSegFrames, (band_frames + kLaunchGroups - 1) / kLaunchGroups));
  for (int i = 0; i < n; i++) {
    host[i].seg = seg;
    if (int rc = add_blocks(who, blocks, (long long)host[i].bands * cdiv(host[i].T, seg), host[i].block_begin)) return rc;
  }
  const int zero_y = (int)std::min<long long>(std::max<long long>(((long long)(kBins + 1) * max_T + kZeroWordsPerBlock - 1) / kZeroWordsPerBlock, 1), 64);
  host[0].zero_y = zero_y;
  if (int rc = upload_and_launch(frame_stats_zero_kernel, (long long)n * zero_y, 0, host, table_dev, n, stream, who)) return rc;
  hipLaunchKernelGGL(frame_stats_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, (const StatsParams*)table_dev, n);
  return check_launch(who);
}

extern "C" size_t td_shot_cuts_table_bytes(int n_jobs) { return table_bytes<CutsParams>(n_jobs); }

extern "C" int td_shot_cuts(const td_cuts_job* jobs, int n_jobs, void* table_host, void* table_dev, size_t table_bytes, td_stream_t stream) {
  const char* who = "td_shot_cuts";
  if (int rc = check_workspace<CutsParams>(who, jobs, n_jobs, table_host, table_dev, table_bytes)) return rc;
  CutsParams* host = (CutsParams*)table_host;
  for (int i = 0; i < n_jobs; i++) {
    const td_cuts_job& j = jobs[i];
    TD_REQUIRE(j.hist, "%s: job %d: hist is null", who, i);
    TD_REQUIRE(j.sad, "%s: job %d: sad is null", who, i);
    TD_REQUIRE(j.cut, "%s: job %d: cut is null", who, i);
    TD_REQUIRE(j.shot, "%s: job %d: shot is null", who, i);
    TD_REQUIRE(j.n_shots, "%s: job %d: n_shots is null", who, i);
    TD_REQUIRE(j.T >= 0 && j.T <= kMaxCutT, "%s: job %d: T = %d outside 0..%d", who, i, j.T, kMaxCutT);
    TD_REQUIRE(j.N >= 1 && j.N <= kMaxPixels, "%s: job %d: N = %d outside 1..%d", who, i, j.N, kMaxPixels);
    TD_REQUIRE(j.w >= 0 && j.w <= kMaxWindow, "%s: job %d: w = %d outside 0..%d", who, i, j.w, kMaxWindow);
    const struct { const char* name; int num, den; } frac[3] = {{"hist", j.hist_num, j.hist_den}, {"sad", j.sad_num, j.sad_den}, {"peak", j.peak_num, j.peak_den}};
    for (const auto& f : frac) {
      TD_REQUIRE(f.num >= 0 && f.num <= kMaxFrac, "%s: job %d: %s_num = %d outside 0..%d", who, i, f.name, f.num, kMaxFrac);
      TD_REQUIRE(f.den >= 1 && f.den <= kMaxFrac, "%s: job %d: %s_den = %d outside 1..%d", who, i, f.name, f.den, kMaxFrac);
    }
    CutsParams p{};
    p.hist = j.hist; p.sad = j.sad; p.d = j.d; p.cut = j.cut; p.shot = j.shot; p.n_shots = j.n_shots;
    p.T = j.T; p.N = j.N; p.hist_num = j.hist_num; p.hist_den = j.hist_den; p.sad_num = j.sad_num; p.sad_den = j.sad_den;
    p.peak_num = j.peak_num; p.peak_den = j.peak_den; p.w = j.w;
    host[i] = p;
  }
  return upload_and_launch(shot_cuts_kernel, n_jobs, 0, host, table_dev, n_jobs, stream, who);
}
