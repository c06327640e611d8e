// Boxes that follow the object's pixels between sampled frames: td_tube_follow (include/tubedetr_hip.h has the rule).
//
// A unit of work is one (job, frame t, tube k): one workgroup, found with find_job.  A unit that is COPIED (an anchor frame, an
// absent box, no anchor within reach, an anchor box outside the frame) is decided from a few uniform loads and written by one
// lane before any pixel is touched.  A unit that matches walks the 16 rows of the sample grid; per grid row
//   * the 16 neighbourhoods of (2 R + 1)^2 luma bytes of frame t are staged in LDS TRANSPOSED: position (dy, dx) owns 16 bytes,
//     byte j that of sample j, so a candidate's 16 differences are one 16-byte LDS read and four v_sad_u8.  A staging task is
//     (row dy, 4 neighbouring dx, 4 neighbouring samples): where the four pixels of a sample lie inside the row, which is
//     everywhere but at the frame's border, they are ONE 4-byte load at whatever address the pitch gives (rgb24: three, and the
//     luma is computed on the way in); at the border every pixel is clamped and fetched by itself.  The 4 x 4 bytes are transposed
//     in registers and go to LDS as four dwords.  No read leaves the row: both paths stay inside [0, sw);
//   * candidate c = (dy + R) (2 R + 1) + (dx + R) belongs to lane c % 256, at most five per lane at R = 16, which keeps the
//     sums in registers across the grid rows: 17 KiB of LDS for the neighbourhoods whatever the box's size.
// There is no early exit for a candidate whose partial sum is past the accept bound: cost is an output for rejected units too.
// The best candidate is the minimum of one 64-bit key (c, dy^2 + dx^2, dy + R, dx + R) per lane, over the wave by shuffles and
// over the four waves through LDS: a minimum does not depend on the order it is taken in.
#include "frame_jobs.h"

namespace td {

namespace {

constexpr int kMaxRadius = 16, kMaxReach = 64, kMaxFollowK = 8, kMaxAccept = 1 << 20;
constexpr int kGrid = 16;                                           // sample points per side
constexpr int kMaxCand = (2 * kMaxRadius + 1) * (2 * kMaxRadius + 1);  // 1089
constexpr int kCandPerLane = (kMaxCand + kThreads - 1) / kThreads;     // 5

struct FollowParams {
  const unsigned char* src;  // plane 0: the only one that is read
  long long stride;
  const float* boxes;
  const unsigned char* anchor;
  const int* shot;
  float* out;
  int* offset;
  uint32_t* cost;
  unsigned char* status;
  int pitch, rgb, T, sh, sw, K, radius, reach, accept_num, accept_den;
  int block_begin;
};

typedef uint32_t __attribute__((aligned(1))) u32_any;  // a dword at any address

__device__ __forceinline__ bool finite_bits(uint32_t b) { return (b & 0x7F800000u) != 0x7F800000u; }

__device__ __forceinline__ bool load_box(const float* boxes, long long idx, uint32_t b[4]) {
  const TD_GLOBAL uint32_t* at = (const TD_GLOBAL uint32_t*)boxes + 4 * idx;
#pragma unroll
  for (int c = 0; c < 4; c++) b[c] = at[c];
  return finite_bits(b[0]) && finite_bits(b[1]) && finite_bits(b[2]) && finite_bits(b[3]);
}

__device__ __forceinline__ uint32_t luma_of(uint32_t r, uint32_t g, uint32_t b) { return (77u * r + 150u * g + 29u * b + 128u) >> 8; }

// L of pixel x of the row at rowp
template <bool RGB>
__device__ __forceinline__ uint32_t luma_at(gcbyte_ptr rowp, int x) {
  if (!RGB) return rowp[x];
  gcbyte_ptr a = rowp + 3 * x;
  return luma_of(a[0], a[1], a[2]);
}

// L of pixels xb .. xb + 3 of the row, clamped to [0, sw), byte u that of pixel xb + u
template <bool RGB>
__device__ __forceinline__ uint32_t luma4(gcbyte_ptr rowp, int xb, int sw) {
  if (xb >= 0 && xb + 3 < sw) {
    if (!RGB) return *(const TD_GLOBAL u32_any*)(rowp + xb);
    const TD_GLOBAL u32_any* a = (const TD_GLOBAL u32_any*)(rowp + 3 * xb);
    const uint32_t d0 = a[0], d1 = a[1], d2 = a[2];
    return luma_of(d0 & 255u, (d0 >> 8) & 255u, (d0 >> 16) & 255u) | luma_of(d0 >> 24, d1 & 255u, (d1 >> 8) & 255u) << 8 |
           luma_of((d1 >> 16) & 255u, d1 >> 24, d2 & 255u) << 16 | luma_of((d2 >> 8) & 255u, (d2 >> 16) & 255u, d2 >> 24) << 24;
  }
  uint32_t v = 0;
#pragma unroll
  for (int u = 0; u < 4; u++) v |= luma_at<RGB>(rowp, min(max(xb + u, 0), sw - 1)) << (8 * u);
  return v;
}

__device__ __forceinline__ void write_unit(const FollowParams* p, long long idx, const uint32_t o[4], int dy, int dx, uint32_t cost, int status) {
  TD_GLOBAL uint32_t* out = (TD_GLOBAL uint32_t*)p->out + 4 * idx;
#pragma unroll
  for (int c = 0; c < 4; c++) out[c] = o[c];
  if (p->offset) {
    TD_GLOBAL int* off = (TD_GLOBAL int*)p->offset + 2 * idx;
    off[0] = dy; off[1] = dx;
  }
  if (p->cost) ((TD_GLOBAL uint32_t*)p->cost)[idx] = cost;
  if (p->status) ((gbyte_ptr)p->status)[idx] = (unsigned char)status;
}

template <bool RGB>
__device__ __forceinline__ void follow_unit(const FollowParams* __restrict__ p, int t, int g, long long idx, const uint32_t B[4], const uint32_t A[4], u32x4* nb,
                                            uint32_t* tem, unsigned long long* best) {
  const int tid = threadIdx.x;
  const int sh = p->sh, sw = p->sw, R = p->radius;
  // steps 3 - 5
  const int ax0 = round_coord(__uint_as_float(A[0])), ay0 = round_coord(__uint_as_float(A[1])), ax1 = round_coord(__uint_as_float(A[2])), ay1 = round_coord(__uint_as_float(A[3]));
  const int bx0 = round_coord(__uint_as_float(B[0])), by0 = round_coord(__uint_as_float(B[1])), bx1 = round_coord(__uint_as_float(B[2])), by1 = round_coord(__uint_as_float(B[3]));
  const int x0 = max(ax0, 0), y0 = max(ay0, 0), w = min(ax1, sw) - x0, h = min(ay1, sh) - y0;
  if (w <= 0 || h <= 0) {
    if (tid == 0) write_unit(p, idx, B, 0, 0, 0, 0);
    return;
  }
  const int ddx = ((bx0 + bx1) - (ax0 + ax1)) >> 1, ddy = ((by0 + by1) - (ay0 + ay1)) >> 1;
  gcbyte_ptr frame_g = (gcbyte_ptr)p->src + (long long)g * p->stride;
  gcbyte_ptr frame_t = (gcbyte_ptr)p->src + (long long)t * p->stride;
  {  // the template: lane (i, j) fetches its sample of the anchor frame
    const int i = tid >> 4, j = tid & 15;
    const int py = y0 + ((2 * i + 1) * h) / 32, px = x0 + ((2 * j + 1) * w) / 32;
    ((unsigned char*)tem)[tid] = (unsigned char)luma_at<RGB>(frame_g + (long long)py * p->pitch, px);
  }
  const int S = 2 * R + 1, n_cand = S * S, n_chunk = (S + 3) >> 2, n_task = S * n_chunk * 4;
  uint32_t* nbw = (uint32_t*)nb;
  uint32_t acc[kCandPerLane];
#pragma unroll
  for (int m = 0; m < kCandPerLane; m++) acc[m] = 0;
  for (int i = 0; i < kGrid; i++) {
    __syncthreads();  // the candidates of the grid row before have read nb (first row: tem is written)
    const int yb = y0 + ((2 * i + 1) * h) / 32 + ddy - R;
    for (int q = tid; q < n_task; q += kThreads) {
      const int jg = q & 3, r = q >> 2, dyi = r / n_chunk, dxi = 4 * (r - dyi * n_chunk);
      gcbyte_ptr rowp = frame_t + (long long)min(max(yb + dyi, 0), sh - 1) * p->pitch;
      uint32_t v[4];
#pragma unroll
      for (int s = 0; s < 4; s++) v[s] = luma4<RGB>(rowp, x0 + ((2 * (4 * jg + s) + 1) * w) / 32 + ddx - R + dxi, sw);
#pragma unroll
      for (int u = 0; u < 4; u++)
        if (dxi + u < S)
          nbw[4 * (dyi * S + dxi + u) + jg] = ((v[0] >> (8 * u)) & 255u) | ((v[1] >> (8 * u)) & 255u) << 8 | ((v[2] >> (8 * u)) & 255u) << 16 | ((v[3] >> (8 * u)) & 255u) << 24;
    }
    __syncthreads();
    const uint32_t t0 = tem[4 * i], t1 = tem[4 * i + 1], t2 = tem[4 * i + 2], t3 = tem[4 * i + 3];
#pragma unroll
    for (int m = 0; m < kCandPerLane; m++) {
      const int c = tid + m * kThreads;
      if (c < n_cand) {
        const u32x4 v = nb[c];
        acc[m] = __builtin_amdgcn_sad_u8(v.x, t0, acc[m]);
        acc[m] = __builtin_amdgcn_sad_u8(v.y, t1, acc[m]);
        acc[m] = __builtin_amdgcn_sad_u8(v.z, t2, acc[m]);
        acc[m] = __builtin_amdgcn_sad_u8(v.w, t3, acc[m]);
      }
    }
  }
  // step 7: the smallest (c, dy^2 + dx^2, dy, dx), as one key
  unsigned long long key = ~0ull;
#pragma unroll
  for (int m = 0; m < kCandPerLane; m++) {
    const int c = tid + m * kThreads;
    if (c < n_cand) {
      const int dyi = c / S, dxi = c - dyi * S, dy = dyi - R, dx = dxi - R;
      const unsigned long long k = (unsigned long long)acc[m] << 32 | (unsigned long long)(dy * dy + dx * dx) << 16 | (unsigned long long)(dyi << 8 | dxi);
      key = k < key ? k : key;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(key, o, 64);
    key = other < key ? other : key;
  }
  if ((tid & 63) == 0) best[tid >> 6] = key;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int wv = 1; wv < kThreads / 64; wv++) key = best[wv] < key ? best[wv] : key;
    const uint32_t c = (uint32_t)(key >> 32);
    const int dy = (int)((key >> 8) & 255u) - R, dx = (int)(key & 255u) - R;
    // step 8
    const bool ok = (unsigned long long)c * (unsigned long long)p->accept_den <= (unsigned long long)p->accept_num * 256ull;
    if (ok && (dy != 0 || dx != 0)) {
      const float fx = (float)dx, fy = (float)dy;
      const uint32_t o[4] = {__float_as_uint(__uint_as_float(B[0]) + fx), __float_as_uint(__uint_as_float(B[1]) + fy), __float_as_uint(__uint_as_float(B[2]) + fx),
                             __float_as_uint(__uint_as_float(B[3]) + fy)};
      write_unit(p, idx, o, dy, dx, c, 1);
    } else {
      write_unit(p, idx, B, 0, 0, c, ok ? 1 : 2);
    }
  }
}

__global__ __launch_bounds__(kThreads) void tube_follow_kernel(const FollowParams* __restrict__ tab, int n_jobs) {
  __shared__ u32x4 nb[kMaxCand];
  __shared__ uint32_t tem[kGrid * kGrid / 4];
  __shared__ unsigned long long best[kThreads / 64];
  const FollowParams* p = tab + find_job(tab, n_jobs, blockIdx.x);
  const int unit = blockIdx.x - p->block_begin, K = p->K, T = p->T;
  const int t = unit / K, k = unit - t * K;
  const long long idx = (long long)t * K + k;
  // steps 1 and 2: uniform, so every lane takes the same way
  uint32_t B[4], A[4];
  const bool present = load_box(p->boxes, idx, B);
  int g = -1;
  if (present && ((gcbyte_ptr)p->anchor)[t] == 0) {
    const TD_GLOBAL int* shot = (const TD_GLOBAL int*)p->shot;
    const int own = shot ? shot[t] : 0;
    for (int d = 1; d <= p->reach && g < 0; d++) {
#pragma unroll
      for (int s = 0; s < 2; s++) {
        const int q = s ? t + d : t - d;
        if (g >= 0 || q < 0 || q >= T) continue;
        if (((gcbyte_ptr)p->anchor)[q] == 0 || (shot && shot[q] != own)) continue;
        if (load_box(p->boxes, (long long)q * K + k, A)) g = q;
      }
    }
  }
  if (g < 0) {
    if (threadIdx.x == 0) write_unit(p, idx, B, 0, 0, 0, 0);
    return;
  }
  if (p->rgb) follow_unit<true>(p, t, g, idx, B, A, nb, tem, best);
  else follow_unit<false>(p, t, g, idx, B, A, nb, tem, best);
}

}  // namespace

}  // namespace td

using namespace td;

extern "C" size_t td_tube_follow_table_bytes(int n_jobs) { return table_bytes<FollowParams>(n_jobs); }

extern "C" int td_tube_follow(const td_follow_job* jobs, int n_jobs, void* table_host, void* table_dev, size_t table_bytes, td_stream_t stream) {
  const char* who = "td_tube_follow";
  if (int rc = check_workspace<FollowParams>(who, jobs, n_jobs, table_host, table_dev, table_bytes)) return rc;
  FollowParams* host = (FollowParams*)table_host;
  int n = 0;
  long long blocks = 0;
  for (int i = 0; i < n_jobs; i++) {
    const td_follow_job& j = jobs[i];
    TD_REQUIRE(j.fmt == TD_SRC_RGB24 || j.fmt == TD_SRC_I420 || j.fmt == TD_SRC_NV12, "%s: job %d: unknown fmt %d", who, i, j.fmt);
    TD_REQUIRE(j.T >= 0, "%s: job %d: negative frame count T = %d", who, i, j.T);
    TD_REQUIRE(j.sh > 0 && j.sw > 0 && j.sh <= kMaxSide && j.sw <= kMaxSide, "%s: job %d: sh x sw = %d x %d outside 1..%d", who, i, j.sh, j.sw, kMaxSide);
    TD_REQUIRE(j.K >= 1 && j.K <= kMaxFollowK, "%s: job %d: K = %d outside 1..%d", who, i, j.K, kMaxFollowK);
    TD_REQUIRE(j.radius >= 0 && j.radius <= kMaxRadius, "%s: job %d: radius = %d outside 0..%d", who, i, j.radius, kMaxRadius);
    TD_REQUIRE(j.reach >= 1 && j.reach <= kMaxReach, "%s: job %d: reach = %d outside 1..%d", who, i, j.reach, kMaxReach);
    TD_REQUIRE(j.accept_num >= 0 && j.accept_num <= kMaxAccept, "%s: job %d: accept_num = %d outside 0..%d", who, i, j.accept_num, kMaxAccept);
    TD_REQUIRE(j.accept_den >= 1 && j.accept_den <= kMaxAccept, "%s: job %d: accept_den = %d outside 1..%d", who, i, j.accept_den, kMaxAccept);
    TD_REQUIRE(j.boxes, "%s: job %d: boxes is null", who, i);
    TD_REQUIRE(j.anchor, "%s: job %d: anchor is null", who, i);
    TD_REQUIRE(j.out, "%s: job %d: out is null", who, i);
    const PlaneGeom g = plane_geom(j.fmt, j.sh, j.sw);
    const PlaneSet set = {"src", {j.src0, j.src1, j.src2}, {j.src_pitch0, j.src_pitch1, j.src_pitch2}, j.src_frame_stride};
    if (int rc = check_planes(who, i, g, &set, 1)) return rc;
    if (j.T == 0) continue;
    FollowParams p{};
    p.src = (const unsigned char*)j.src0; p.stride = j.src_frame_stride; p.pitch = j.src_pitch0;
    p.boxes = j.boxes; p.anchor = j.anchor; p.shot = j.shot;
    p.out = j.out; p.offset = j.offset; p.cost = j.cost; p.status = j.status;
    p.rgb = j.fmt == TD_SRC_RGB24; p.T = j.T; p.sh = j.sh; p.sw = j.sw; p.K = j.K;
    p.radius = j.radius; p.reach = j.reach; p.accept_num = j.accept_num; p.accept_den = j.accept_den;
    if (int rc = add_blocks(who, blocks, (long long)j.T * j.K, p.block_begin)) return rc;
    host[n++] = p;
  }
  return upload_and_launch(tube_follow_kernel, blocks, 0, host, table_dev, n, stream, who);
}
