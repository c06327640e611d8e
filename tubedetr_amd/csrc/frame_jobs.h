// What the "job table" kernels on decoded frames share: td_clip_resample / td_clip_resample_src (augment.hip), td_tube_overlay
// (overlay.hip), td_tube_overlay_multi (overlay_multi.hip), td_tube_crop (tube_crop.hip), td_tube_redact (redact.hip), td_tube_densify (tube_dense.hip), the stage in front
// of the last three, and td_frame_export (frame_export.hip), the stage behind them all.  One launch serves a table of job records; a
// workgroup finds its job by block_begin.  include/tubedetr_hip.h defines the crop's and the redaction's rectangles by reference
// to the overlay's ("rounding is td_tube_overlay's", "the margin is td_tube_crop's step 4"): each step of that rule exists once,
// here, and the three kernels compose the steps.  The host half is the plane geometry of a pixel format, the checks of a job's
// planes that the entry points have in common (their message texts are part of the interface: tests/test_frame_jobs_cpu.py),
// and the table upload + launch.  Plain functions: a new kernel of the family includes this and writes only its own middle.
#pragma once
#include <algorithm>
#include <cmath>

#include "td_common.h"

namespace td {

constexpr int kThreads = 256;
constexpr int kMaxSide = 16384;       // (2 v + 1) * side (augment: * sw; overlay: * 256 * 128 / side) stays below 2^30
constexpr int kMaxMarginDen = 1024;
constexpr int kRun = 16;              // bytes of a row per lane (load_run / store_run)

// ---- device: addressing ---------------------------------------------------------------------------------------------------
// the table's pointers are loaded from memory, so the compiler cannot see that they are global: say so (global_load / global_store
// instead of flat ones, which also occupy the LDS path that the kernels' tables need)
#define TD_GLOBAL __attribute__((address_space(1)))
typedef const TD_GLOBAL unsigned char* gcbyte_ptr;
typedef TD_GLOBAL unsigned char* gbyte_ptr;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// last job whose first block is <= b (b = blockIdx.x: uniform, so the search runs on scalar loads)
template <typename P>
__device__ __forceinline__ int find_job(const P* __restrict__ tab, int n_jobs, int b) {
  int lo = 0, hi = n_jobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].block_begin <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// ---- device: byte runs ----------------------------------------------------------------------------------------------------
// A lane owns an ALIGNED run of kRun bytes of a destination row.  Only the first / last run of a tile's row, which it shares with
// the row padding or with the neighbour tile, is loaded and stored by bytes - so no lane reads or writes a byte that another
// lane or workgroup writes, which is what makes the in-place case free of hazards.
// bytes [o0, o0 + 16) of a row, of which [v0, v1) belong to the tile: no other byte is touched
__device__ __forceinline__ void load_run(const unsigned char* rowp, int o0, int v0, int v1, uint32_t in[4]) {
  const unsigned char* a = rowp + o0;
  const bool full = v0 == o0 && v1 == o0 + kRun;
  if (full && ((uintptr_t)a & 15) == 0) {
    const u32x4 v = *(const TD_GLOBAL u32x4*)a;
    in[0] = v.x; in[1] = v.y; in[2] = v.z; in[3] = v.w;
  } else if (full && ((uintptr_t)a & 3) == 0) {
#pragma unroll
    for (int k = 0; k < 4; k++) in[k] = ((const TD_GLOBAL uint32_t*)a)[k];
  } else {
    in[0] = in[1] = in[2] = in[3] = 0;
#pragma unroll
    for (int j = 0; j < kRun; j++)
      if (o0 + j >= v0 && o0 + j < v1) in[j >> 2] |= (uint32_t)((gcbyte_ptr)a)[j] << (8 * (j & 3));
  }
}

// rowp + o0 is 16-byte aligned
__device__ __forceinline__ void store_run(unsigned char* rowp, int o0, int v0, int v1, const uint32_t out[4]) {
  unsigned char* a = rowp + o0;
  if (v0 == o0 && v1 == o0 + kRun) {
    u32x4 v;
    v.x = out[0]; v.y = out[1]; v.z = out[2]; v.w = out[3];
    *(TD_GLOBAL u32x4*)a = v;
  } else {
#pragma unroll
    for (int j = 0; j < kRun; j++)
      if (o0 + j >= v0 && o0 + j < v1) ((gbyte_ptr)a)[j] = (unsigned char)(out[j >> 2] >> (8 * (j & 3)));
  }
}

// ---- device: the tube rule (include/tubedetr_hip.h), one function per step ---------------------------------------------------
// the tube row of frame t
__device__ __forceinline__ int tube_row(const int* frame_map, int t) { return frame_map ? ((const TD_GLOBAL int*)frame_map)[t] : t; }

// row r lies in the span of tube k (int64 [K][2], both ends included); no span: every row does
__device__ __forceinline__ bool row_in_span(const long long* span, int k, int r) {
  if (!span) return true;
  const long long s0 = ((const TD_GLOBAL long long*)span)[2 * k], s1 = ((const TD_GLOBAL long long*)span)[2 * k + 1];
  return r >= s0 && r <= s1;
}

__device__ __forceinline__ int round_coord(float v) { return (int)floorf(fminf(fmaxf(v, -1048576.f), 1048576.f) + 0.5f); }

// the rounded corners of box `idx` (fp32 xyxy); false - the box is absent - for a corner that is not finite (the outputs are then
// left alone) and for x1 <= x0 or y1 <= y0
__device__ __forceinline__ bool rounded_box(const float* boxes, long long idx, int& x0, int& y0, int& x1, int& y1) {
  const TD_GLOBAL float* bx = (const TD_GLOBAL float*)boxes + 4 * idx;
  const float c0 = bx[0], c1 = bx[1], c2 = bx[2], c3 = bx[3];
  if (!(isfinite(c0) && isfinite(c1) && isfinite(c2) && isfinite(c3))) return false;
  x0 = round_coord(c0); y0 = round_coord(c1); x1 = round_coord(c2); y1 = round_coord(c3);
  return x1 > x0 && y1 > y0;
}

// margin_num / margin_den of the box's side added on every side (the division truncates; its operands are not negative), then the
// clamp to the sh x sw frame: the window of cw x ch pixels at (wx0, wy0); false when nothing of it lies in the frame.  (Origin and
// size, not two corners: handed the far corner, tube_crop_kernel's register allocation comes out differently.)
__device__ __forceinline__ bool grow_and_clamp(int x0, int y0, int x1, int y1, int margin_num, int margin_den, int sh, int sw, int& wx0, int& wy0, int& cw, int& ch) {
  const int mx = (int)(((long long)(x1 - x0) * margin_num) / margin_den), my = (int)(((long long)(y1 - y0) * margin_num) / margin_den);
  wx0 = max(x0 - mx, 0); wy0 = max(y0 - my, 0);
  cw = min(x1 + mx, sw) - wx0; ch = min(y1 + my, sh) - wy0;
  return cw > 0 && ch > 0;
}

// ---- device: the overlays' pixel rule (td_tube_overlay, td_tube_overlay_multi) -------------------------------------------------
// where column xl of the tile lives in the column table: the lanes of a wave read columns 16 apart (a luma run; 32 for an I420 chroma
// run), which would all fall into 4 (2) of the 64 LDS banks; one spare slot per 16 columns makes the lane stride 17 (34) dwords
__device__ __forceinline__ int col_slot(int xl) { return xl + (xl >> 4); }

// kind of a byte row
enum { kRgb = 0,      // 3 bytes per pixel
       kLuma = 1,     // 1 byte per pixel
       kChroma = 2,   // 1 byte per 2 x 2 block (I420: U, V, or both rows together)
       kPairs = 3 };  // 2 bytes per block (NV12)

__device__ __forceinline__ uint32_t blend(uint32_t v, uint32_t c, uint32_t a) { return (v * (256u - a) + c * a + 128u) >> 8; }

// g = clamp(((2 v + 1) m 128) / n - 128, 0, 256 (m - 1))
__device__ __forceinline__ int map_coord(int v, int m, int n) { return min(max(((2 * v + 1) * m * 128) / n - 128, 0), 256 * (m - 1)); }

// a colour of a job record as the kernels carry it: byte k = component k
inline uint32_t pack3(const unsigned char c[3]) { return (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16); }

// ---- host: the planes of a job ----------------------------------------------------------------------------------------------
// rgb24: one plane of 3 sw bytes per row; I420: Y, U, V; NV12: Y and the interleaved UV plane.  cols counts samples.
struct PlaneGeom { int n_planes, row_bytes[3], rows[3], cols[3]; };

inline PlaneGeom plane_geom(int fmt, int sh, int sw) {
  const int cw = (sw + 1) / 2, ch = (sh + 1) / 2;
  const int row_bytes[3] = {fmt == TD_SRC_RGB24 ? 3 * sw : sw, fmt == TD_SRC_NV12 ? 2 * cw : cw, cw};
  const int rows[3] = {sh, ch, ch}, cols[3] = {sw, cw, cw};
  PlaneGeom g{};
  g.n_planes = fmt == TD_SRC_RGB24 ? 1 : fmt == TD_SRC_NV12 ? 2 : 3;
  for (int k = 0; k < 3; k++) { g.row_bytes[k] = row_bytes[k]; g.rows[k] = rows[k]; g.cols[k] = cols[k]; }
  return g;
}

// bytes of plane k from the first row of frame 0 to the last row of frame T - 1 (T = 1: what a frame stride has to hold)
inline long long plane_extent(const PlaneGeom& g, int k, int pitch, long long frame_stride = 0, int T = 1) {
  return (long long)(T - 1) * frame_stride + (long long)pitch * (g.rows[k] - 1) + g.row_bytes[k];
}

// one side of a job as its record names it: `stem` is "src" / "dst" (src0, src_pitch0, src_frame_stride) or "" (plane0, pitch0, frame_stride)
struct PlaneSet {
  const char* stem;
  const void* p[3];
  int pitch[3];
  long long frame_stride;
};

// per plane, for every set in turn: the pointer is not null, the pitch holds a row, the frame stride holds the plane
inline int check_planes(const char* who, int i, const PlaneGeom& g, const PlaneSet* sets, int n_sets) {
  for (int k = 0; k < g.n_planes; k++) {
    for (int s = 0; s < n_sets; s++) TD_REQUIRE(sets[s].p[k], "%s: job %d: %s%d is null", who, i, sets[s].stem[0] ? sets[s].stem : "plane", k);
    for (int s = 0; s < n_sets; s++)
      TD_REQUIRE(sets[s].pitch[k] >= g.row_bytes[k], "%s: job %d: %s%spitch%d = %d is below its row of %d bytes", who, i, sets[s].stem, sets[s].stem[0] ? "_" : "", k,
                 sets[s].pitch[k], g.row_bytes[k]);
    for (int s = 0; s < n_sets; s++)
      TD_REQUIRE(sets[s].frame_stride >= plane_extent(g, k, sets[s].pitch[k]), "%s: job %d: %s%sframe_stride %lld is smaller than plane %d needs (%d rows of pitch %d)", who, i,
                 sets[s].stem, sets[s].stem[0] ? "_" : "", sets[s].frame_stride, k, g.rows[k], sets[s].pitch[k]);
  }
  return TD_OK;
}

// destination plane k is its source plane (pointer, pitch and frame stride; *inplace says so), or its bytes over T frames touch no
// source plane; a job without frames has no bytes that could overlap
inline int check_inplace_or_apart(const char* who, int i, const PlaneGeom& g, const PlaneSet& s, const PlaneSet& d, int T, int k, bool* inplace = nullptr) {
  const bool same = d.p[k] == s.p[k] && d.pitch[k] == s.pitch[k] && d.frame_stride == s.frame_stride;
  if (inplace) *inplace = same;
  if (same || T == 0) return TD_OK;
  const unsigned char* d0 = (const unsigned char*)d.p[k];
  for (int m = 0; m < g.n_planes; m++)
    TD_REQUIRE(d0 + plane_extent(g, k, d.pitch[k], d.frame_stride, T) <= s.p[m] || (const unsigned char*)s.p[m] + plane_extent(g, m, s.pitch[m], s.frame_stride, T) <= d0,
               "%s: job %d: dst%d overlaps src%d without being the same plane (pointer, pitch and frame stride)", who, i, k, m);
  return TD_OK;
}

// ---- host: the job table and the launch ---------------------------------------------------------------------------------------
template <typename P>
size_t table_bytes(int n_jobs) { return n_jobs > 0 ? (((size_t)n_jobs * sizeof(P)) + 255) & ~(size_t)255 : 0; }

// what every entry point asks before it reads a job; `who` is the entry point's name, <who>_table_bytes its sizing function
template <typename P>
int check_workspace(const char* who, const void* jobs, int n_jobs, const void* table_host, const void* table_dev, size_t bytes) {
  TD_REQUIRE(jobs && n_jobs > 0 && n_jobs <= 65536, "%s: no jobs (or more than 65536)", who);
  TD_REQUIRE(table_host && table_dev && bytes >= table_bytes<P>(n_jobs), "%s: job-table workspace missing or smaller than %s_table_bytes(%d)", who, who, n_jobs);
  return TD_OK;
}

// a job of job_blocks workgroups begins at block_begin, behind the `blocks` of the jobs before it
inline int add_blocks(const char* who, long long& blocks, long long job_blocks, int& block_begin) {
  block_begin = (int)blocks;
  blocks += job_blocks;
  TD_REQUIRE(blocks < (1LL << 31), "%s: too many workgroups", who);
  return TD_OK;
}

// the n records that the jobs with frames left in table_host go to the device and the kernel runs over all of their workgroups
template <typename P>
int upload_and_launch(void (*kernel)(const P*, int), long long blocks, size_t lds, const P* table_host, void* table_dev, int n, td_stream_t stream, const char* who) {
  if (n == 0) return TD_OK;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemcpyAsync(table_dev, table_host, (size_t)n * sizeof(P), hipMemcpyHostToDevice, st) != hipSuccess) {
    set_error("%s: job table upload failed", who);
    return TD_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kThreads), lds, st, (const P*)table_dev, n);
  return check_launch(who);
}

}  // namespace td
