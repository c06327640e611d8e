// Grounded tubes interpolated to every decoded frame: td_tube_densify (include/tubedetr_hip.h has the rule).
//
// A workgroup owns a run of `fpb` dense frames of one job (fpb K <= 256; fewer frames when the job has attention maps, so that
// a workgroup moves about 8 KiB of them) and does everything those frames need:
//   * the table of sampled frame numbers is staged in LDS when it has at most kTableRows rows, and searched there; a longer
//     one is searched in global memory, and first / step needs no table at all.  The search is the header's, over the WHOLE
//     table, so a table that does not increase gives what the header says, and no index leaves [0, n_tube);
//   * lanes 0 .. frames - 1 place their frame (row a, num, den) once, into LDS: the K rectangles of a frame and every byte run
//     of its attention map read the placement instead of searching again;
//   * the presence bits (bit k of a byte per tube row: inside span k and four finite coordinates) of the rows that the run can
//     ask for - from row a of its first frame, less the smoothing radius, to row b of its last frame, plus the radius - are
//     staged in LDS; a row outside that window (only a table that does not increase asks for one) is evaluated from memory, so
//     the window is a cache and never decides a result;
//   * lane (frame, k) then computes the working boxes of rows a and b on the fly (at most 33 rows per coordinate each, added
//     in ascending order) and the mode's box.  The arithmetic goes through add_rn / sub_rn / mul_rn / div_rn below: one
//     rounding per operation, no fused multiply-add, which is what makes numpy float32 reproduce it;
//   * the attention maps are byte work: a frame's map is one row of mh mw bytes, and a lane owns ALIGNED runs of 16 bytes of
//     it (load_run / store_run of frame_jobs.h), loaded with one 16-byte load where the source row has the same alignment;
//   * lanes 0 .. K - 1 of a job's first workgroup write dense_span; a job with T = 0 has that workgroup only;
//   * td_tube_densify_shots hands the job an array of shot ids by frame number.  A lane then looks up the shot of its frame and
//     of rows a and b (and of every row of a smoothing window) in memory; a row on the other side of a cut drops out and its
//     neighbour stands alone.  Without the array - td_tube_densify - no lookup is made and every branch goes as it did.
// No atomics, no scratch; plain C++ and vector stores.  The job search, the span test, the byte runs, the workspace checks and
// the launch are the family's: frame_jobs.h.
#include "frame_jobs.h"

namespace td {

namespace {

constexpr int kMaxRects = 8;
constexpr int kMaxSmooth = 16;
constexpr int kTableRows = 1024;                    // rows of row_frame that LDS holds
constexpr int kWindow = kThreads + 2 + 2 * kMaxSmooth + 30;  // presence bits: a strictly increasing table needs frames + 1 + 2 w rows
constexpr int kHeatBytes = 8192;                    // attention-map bytes per workgroup, about
constexpr int kMaxDen = 1 << 24;
constexpr int kMaxT = 1 << 20, kMaxFrameNo = 1 << 23, kMaxStep = 1 << 16, kMaxMap = 256;
constexpr uint32_t kQuietNaN = 0x7FC00000u;

struct DenseParams {
  const float* boxes;
  const long long* span;
  const int* row_frame;
  const unsigned char* heat;
  float* dense;
  unsigned char* valid;
  long long* dense_span;
  unsigned char* dense_heat;
  int n_tube, K, T, t0, first, step, mode, smooth;
  int map_bytes;  // mh mw; 0: no attention maps
  int fpb;        // dense frames per workgroup
  int block_begin;
  const int* shot;  // td_tube_densify_shots: the shot of frame number shot_t0 + i, i < shot_T; null: no shots
  int shot_t0, shot_T;
};

// the shot of frame number f; kAnyShot - unknown - outside the array: it matches every shot
constexpr long long kAnyShot = 1LL << 40;
__device__ __forceinline__ long long shot_of(const DenseParams* p, long long f) {
  const long long i = f - p->shot_t0;
  return i >= 0 && i < p->shot_T ? (long long)((const TD_GLOBAL int*)p->shot)[i] : kAnyShot;
}
__device__ __forceinline__ bool one_shot(long long x, long long y) { return x == y || x == kAnyShot || y == kAnyShot; }

// the frame number of tube row r (0 <= r < n_tube)
__device__ __forceinline__ long long row_frame_at(const DenseParams* p, const int* lds_table, int r) {
  if (!p->row_frame) return (long long)p->first + (long long)r * p->step;
  return lds_table ? lds_table[r] : ((const TD_GLOBAL int*)p->row_frame)[r];
}

// step 1 from memory
__device__ __forceinline__ bool present_in_memory(const DenseParams* p, int r, int k) {
  if (!row_in_span(p->span, k, r)) return false;
  const TD_GLOBAL float* bx = (const TD_GLOBAL float*)p->boxes + 4 * ((long long)r * p->K + k);
  return isfinite(bx[0]) && isfinite(bx[1]) && isfinite(bx[2]) && isfinite(bx[3]);
}

// step 3: row a of frame number f; den = -1: the frame is absent; num = 0: it sits on row a; else 0 < num < den <= 2^24
__device__ __forceinline__ void place_frame(const DenseParams* p, const int* lds_table, long long f, int& a, int& num, int& den) {
  const int n = p->n_tube;
  a = 0; num = 0; den = -1;
  if (f < row_frame_at(p, lds_table, 0)) return;
  if (f > row_frame_at(p, lds_table, n - 1)) { a = n - 1; return; }
  if (!p->row_frame) {
    const long long q = (f - p->first) / p->step;  // the operands are not negative
    a = (int)(q < n - 1 ? q : n - 1);
  } else {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
      const int mid = (int)(((long long)lo + hi + 1) >> 1);
      if (row_frame_at(p, lds_table, mid) <= f) lo = mid; else hi = mid - 1;
    }
    a = lo;
  }
  const long long fa = row_frame_at(p, lds_table, a);
  if (f == fa) { den = 1; return; }
  if (a + 1 >= n) return;
  const long long d = row_frame_at(p, lds_table, a + 1) - fa, m = f - fa;
  if (d <= 0 || d > kMaxDen || m <= 0 || m >= d) return;
  num = (int)m; den = (int)d;
}

}  // namespace

// One IEEE operation each, and none of them may be fused with its neighbour.  HIP's __fadd_rn / __fsub_rn / __fmul_rn / __fdiv_rn
// do NOT give that: the headers define them as the plain operators, compiled under hipcc's default -ffp-contract=fast, so once
// they are inlined the backend fuses A + wgt * (B - A) into v_pk_fma_f32 all the same (seen in this kernel's assembly).  The
// operators written HERE, under the pragma, carry no permission to contract, whatever the command line says; the division is
// the correctly rounded one (hipcc's default, -fhip-fp32-correctly-rounded-divide-sqrt).
#pragma clang fp contract(off)
__device__ __forceinline__ float add_rn(float x, float y) { return x + y; }
__device__ __forceinline__ float sub_rn(float x, float y) { return x - y; }
__device__ __forceinline__ float mul_rn(float x, float y) { return x * y; }
__device__ __forceinline__ float div_rn(float x, float y) { return x / y; }

__global__ __launch_bounds__(kThreads) void tube_dense_kernel(const DenseParams* __restrict__ tab, int n_jobs) {
  __shared__ int table[kTableRows];
  __shared__ int fr_a[kThreads], fr_num[kThreads], fr_den[kThreads];
  __shared__ unsigned char window[kWindow];
  const int tid = threadIdx.x, b = blockIdx.x;
  const DenseParams* p = tab + find_job(tab, n_jobs, b);
  const int local = b - p->block_begin;
  const int n = p->n_tube, K = p->K, mode = p->mode, w = p->smooth;
  const int i0 = local * p->fpb, nf = min(p->fpb, p->T - i0);  // the run's frames; none for the only workgroup of a T = 0 job

  const int* lds_table = nullptr;
  if (p->row_frame && n <= kTableRows) {
    for (int r = tid; r < n; r += kThreads) table[r] = ((const TD_GLOBAL int*)p->row_frame)[r];
    lds_table = table;
  }
  __syncthreads();

  // ---- step 6
  if (local == 0 && tid < K && p->dense_span) {
    long long s0 = 0, s1 = n - 1;
    if (p->span) {
      s0 = max(((const TD_GLOBAL long long*)p->span)[2 * tid], 0LL);
      s1 = min(((const TD_GLOBAL long long*)p->span)[2 * tid + 1], (long long)(n - 1));
    }
    long long d0 = 0, d1 = -1;
    if (s0 <= s1) {
      d0 = row_frame_at(p, lds_table, (int)s0) - p->t0;
      d1 = row_frame_at(p, lds_table, (int)s1) - p->t0;
      if (mode == TD_DENSE_HULL) {
        if (s0 > 0) d0 = row_frame_at(p, lds_table, (int)s0 - 1) + 1 - p->t0;
        if (s1 < n - 1) d1 = row_frame_at(p, lds_table, (int)s1 + 1) - 1 - p->t0;
      }
    }
    TD_GLOBAL long long* ds = (TD_GLOBAL long long*)p->dense_span + 2 * tid;
    ds[0] = d0; ds[1] = d1;
  }
  if (nf <= 0) return;  // uniform

  // ---- step 3, once per frame
  if (tid < nf) {
    int a, num, den;
    place_frame(p, lds_table, (long long)p->t0 + i0 + tid, a, num, den);
    fr_a[tid] = a; fr_num[tid] = num; fr_den[tid] = den;
  }
  __syncthreads();

  // ---- step 1 for the rows that the run can ask for
  const int win_lo = max(fr_a[0] - w, 0);
  const int win_n = max(min(min(fr_a[nf - 1] + 1 + w, n - 1) - win_lo + 1, kWindow), 0);
  for (int j = tid; j < win_n; j += kThreads) {
    uint32_t bits = 0;
    for (int k = 0; k < K; k++) bits |= present_in_memory(p, win_lo + j, k) ? 1u << k : 0u;
    window[j] = (unsigned char)bits;
  }
  __syncthreads();

  if (tid < nf * K) {
    const int fi = tid / K, k = tid - fi * K;
    const int a = fr_a[fi], num = fr_num[fi], den = fr_den[fi];
    const bool shots = p->shot != nullptr;  // uniform
    auto present = [&](int r) -> bool {
      const int j = r - win_lo;
      return (j >= 0 && j < win_n) ? ((window[j] >> k) & 1) != 0 : present_in_memory(p, r, k);
    };
    // step 2: the working box of a present row
    auto working = [&](int r, float v[4]) {
      const TD_GLOBAL float* base = (const TD_GLOBAL float*)p->boxes + 4 * (long long)k;
      if (w == 0) {
        const TD_GLOBAL float* bx = base + 4 * (long long)r * K;
#pragma unroll
        for (int c = 0; c < 4; c++) v[c] = bx[c];
        return;
      }
      float s[4] = {0.f, 0.f, 0.f, 0.f};
      int count = 0;
      const long long sr = shots ? shot_of(p, row_frame_at(p, lds_table, r)) : kAnyShot;
      for (int q = max(r - w, 0); q <= min(r + w, n - 1); q++) {
        if (!present(q)) continue;
        if (shots && !one_shot(shot_of(p, row_frame_at(p, lds_table, q)), sr)) continue;
        const TD_GLOBAL float* bx = base + 4 * (long long)q * K;
#pragma unroll
        for (int c = 0; c < 4; c++) s[c] = add_rn(s[c], bx[c]);
        count++;
      }
      const float cnt = (float)count;
#pragma unroll
      for (int c = 0; c < 4; c++) v[c] = div_rn(s[c], cnt);
    };
    float v[4];
    bool have = false;
    if (den > 0) {
      const bool pa = present(a);
      bool ia = true, ib = true;  // rows a and b are in one shot with the frame
      if (shots && num != 0) {
        const long long sf = shot_of(p, (long long)p->t0 + i0 + fi);
        ia = one_shot(shot_of(p, row_frame_at(p, lds_table, a)), sf);
        ib = one_shot(shot_of(p, row_frame_at(p, lds_table, a + 1)), sf);
      }
      if (!(ia && ib)) {  // a cut between the frame and a row: the other row alone, in every mode
        if (ia ? pa : (ib && present(a + 1))) { working(ia ? a : a + 1, v); have = true; }
      } else if (num == 0 || mode == TD_DENSE_HOLD) {
        if (pa) { working(a, v); have = true; }
      } else {
        const bool pb = present(a + 1);
        if (pa && pb) {
          float A[4], B[4];
          working(a, A); working(a + 1, B);
          if (mode == TD_DENSE_LERP) {
            const float wgt = div_rn((float)num, (float)den);
#pragma unroll
            for (int c = 0; c < 4; c++) v[c] = add_rn(A[c], mul_rn(wgt, sub_rn(B[c], A[c])));
          } else {
            v[0] = B[0] < A[0] ? B[0] : A[0]; v[1] = B[1] < A[1] ? B[1] : A[1];
            v[2] = B[2] > A[2] ? B[2] : A[2]; v[3] = B[3] > A[3] ? B[3] : A[3];
          }
          have = true;
        } else if (mode == TD_DENSE_HULL && (pa || pb)) {
          working(pa ? a : a + 1, v);
          have = true;
        }
      }
    }
    // step 5
    uint32_t bits[4];
    bool ok = have;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      bits[c] = have ? __float_as_uint(v[c]) : kQuietNaN;
      if ((bits[c] & 0x7fffffffu) > 0x7f800000u) bits[c] = kQuietNaN;
      if ((bits[c] & 0x7f800000u) == 0x7f800000u) ok = false;
    }
    const long long o = (long long)(i0 + fi) * K + k;
    TD_GLOBAL uint32_t* dp = (TD_GLOBAL uint32_t*)p->dense + 4 * o;
#pragma unroll
    for (int c = 0; c < 4; c++) dp[c] = bits[c];
    if (p->valid) ((gbyte_ptr)p->valid)[o] = ok ? 1 : 0;
  }

  // ---- step 7: a frame's map is a row of map_bytes bytes
  const int mb = p->map_bytes;
  if (mb == 0) return;
  unsigned char* d0 = p->dense_heat + (long long)i0 * mb;
  // runs per frame: exact when every frame's map has the alignment of the first, else the most a map can have
  const int n_run = (mb & (kRun - 1)) ? (mb + 2 * (kRun - 1)) / kRun : ((int)((uintptr_t)d0 & (kRun - 1)) + mb + kRun - 1) / kRun;
  for (int idx = tid; idx < nf * n_run; idx += kThreads) {
    const int fi = idx / n_run, d = idx - fi * n_run;
    unsigned char* drow = d0 + (long long)fi * mb;
    const int o0 = kRun * d - (int)((uintptr_t)drow & (kRun - 1));
    if (o0 >= mb) continue;
    const int v0 = max(o0, 0), v1 = min(o0 + kRun, mb);
    const int a = fr_a[fi], num = fr_num[fi], den = fr_den[fi];
    uint32_t out[4] = {0, 0, 0, 0};
    bool ia = true, ib = true;
    if (p->shot && den > 0 && num != 0) {
      const long long sf = shot_of(p, (long long)p->t0 + i0 + fi);
      ia = one_shot(shot_of(p, row_frame_at(p, lds_table, a)), sf);
      ib = one_shot(shot_of(p, row_frame_at(p, lds_table, a + 1)), sf);
    }
    if (den > 0 && !(ia && ib)) {  // a cut between the frame and a row: the other row's bytes, or none
      if (ia || ib) load_run(p->heat + (long long)(ia ? a : a + 1) * mb, o0, v0, v1, out);
    } else if (den > 0) {
      const unsigned char* ra = p->heat + (long long)a * mb;
      load_run(ra, o0, v0, v1, out);
      if (num != 0 && mode != TD_DENSE_HOLD) {
        uint32_t nb[4];
        load_run(ra + mb, o0, v0, v1, nb);
#pragma unroll
        for (int j = 0; j < kRun; j++) {
          const uint32_t qa = (out[j >> 2] >> (8 * (j & 3))) & 255u, qb = (nb[j >> 2] >> (8 * (j & 3))) & 255u;
          const uint32_t q = mode == TD_DENSE_HULL ? max(qa, qb) : (qa * (uint32_t)(den - num) + qb * (uint32_t)num + (uint32_t)den / 2) / (uint32_t)den;
          out[j >> 2] = (out[j >> 2] & ~(255u << (8 * (j & 3)))) | (q << (8 * (j & 3)));
        }
      }
    }
    store_run(drow, o0, v0, v1, out);
  }
}

}  // namespace td

using namespace td;

extern "C" size_t td_tube_densify_table_bytes(int n_jobs) { return table_bytes<DenseParams>(n_jobs); }

// td_tube_densify is td_tube_densify_shots without shots: one list of checks, one kernel
static int densify(const char* who, const td_dense_job* jobs, const td_dense_shots* shots, int n_jobs, void* table_host, void* table_dev, size_t table_bytes, td_stream_t stream) {
  if (int rc = check_workspace<DenseParams>(who, jobs, n_jobs, table_host, table_dev, table_bytes)) return rc;
  DenseParams* host = (DenseParams*)table_host;
  int n = 0;
  long long blocks = 0;
  for (int i = 0; i < n_jobs; i++) {
    const td_dense_job& j = jobs[i];
    TD_REQUIRE(j.boxes, "%s: job %d: boxes is null", who, i);
    TD_REQUIRE(j.dense, "%s: job %d: dense is null", who, i);
    TD_REQUIRE(j.n_tube >= 1, "%s: job %d: n_tube = %d is below 1", who, i, j.n_tube);
    TD_REQUIRE(j.K >= 1 && j.K <= kMaxRects, "%s: job %d: K = %d outside 1..%d", who, i, j.K, kMaxRects);
    TD_REQUIRE(j.T >= 0 && j.T <= kMaxT, "%s: job %d: T = %d outside 0..%d", who, i, j.T, kMaxT);
    TD_REQUIRE(j.t0 >= -kMaxFrameNo && j.t0 <= kMaxFrameNo, "%s: job %d: t0 = %d outside +-%d", who, i, j.t0, kMaxFrameNo);
    if (!j.row_frame) {
      TD_REQUIRE(j.first >= -kMaxFrameNo && j.first <= kMaxFrameNo, "%s: job %d: first = %d outside +-%d", who, i, j.first, kMaxFrameNo);
      TD_REQUIRE(j.step >= 1 && j.step <= kMaxStep, "%s: job %d: step = %d outside 1..%d", who, i, j.step, kMaxStep);
    }
    TD_REQUIRE(j.smooth >= 0 && j.smooth <= kMaxSmooth, "%s: job %d: smooth = %d outside 0..%d", who, i, j.smooth, kMaxSmooth);
    TD_REQUIRE(j.mode == TD_DENSE_HOLD || j.mode == TD_DENSE_LERP || j.mode == TD_DENSE_HULL, "%s: job %d: unknown mode %d", who, i, j.mode);
    TD_REQUIRE(!j.heat || j.dense_heat, "%s: job %d: heat is given but dense_heat is null", who, i);
    TD_REQUIRE(!j.dense_heat || j.heat, "%s: job %d: dense_heat is given but heat is null", who, i);
    if (j.heat) TD_REQUIRE(j.mh >= 1 && j.mh <= kMaxMap && j.mw >= 1 && j.mw <= kMaxMap, "%s: job %d: mh x mw = %d x %d outside 1..%d", who, i, j.mh, j.mw, kMaxMap);
    const bool with_shots = shots && shots[i].shot;
    if (with_shots) {
      TD_REQUIRE(shots[i].shot_T >= 0 && shots[i].shot_T <= kMaxT, "%s: job %d: shot_T = %d outside 0..%d", who, i, shots[i].shot_T, kMaxT);
      TD_REQUIRE(shots[i].shot_t0 >= -kMaxFrameNo && shots[i].shot_t0 <= kMaxFrameNo, "%s: job %d: shot_t0 = %d outside +-%d", who, i, shots[i].shot_t0, kMaxFrameNo);
    }
    if (j.T == 0 && !j.dense_span) continue;
    DenseParams p{};
    if (with_shots) { p.shot = shots[i].shot; p.shot_t0 = shots[i].shot_t0; p.shot_T = shots[i].shot_T; }
    p.boxes = j.boxes; p.span = j.span; p.row_frame = j.row_frame; p.heat = j.heat;
    p.dense = j.dense; p.valid = j.valid; p.dense_span = j.dense_span; p.dense_heat = j.dense_heat;
    p.n_tube = j.n_tube; p.K = j.K; p.T = j.T; p.t0 = j.t0; p.mode = j.mode; p.smooth = j.smooth;
    p.first = j.row_frame ? 0 : j.first; p.step = j.row_frame ? 1 : j.step;
    p.map_bytes = j.heat ? j.mh * j.mw : 0;
    p.fpb = kThreads / j.K;
    if (p.map_bytes) p.fpb = std::min(p.fpb, std::max(1, kHeatBytes / p.map_bytes));
    if (int rc = add_blocks(who, blocks, std::max(1, cdiv(j.T, p.fpb)), p.block_begin)) return rc;
    host[n++] = p;
  }
  return upload_and_launch(tube_dense_kernel, blocks, 0, host, table_dev, n, stream, who);
}

extern "C" int td_tube_densify(const td_dense_job* jobs, int n_jobs, void* table_host, void* table_dev, size_t table_bytes, td_stream_t stream) {
  return densify("td_tube_densify", jobs, nullptr, n_jobs, table_host, table_dev, table_bytes, stream);
}

extern "C" size_t td_tube_densify_shots_table_bytes(int n_jobs) { return table_bytes<DenseParams>(n_jobs); }

extern "C" int td_tube_densify_shots(const td_dense_job* jobs, const td_dense_shots* shots, int n_jobs, void* table_host, void* table_dev, size_t table_bytes, td_stream_t stream) {
  return densify("td_tube_densify_shots", jobs, shots, n_jobs, table_host, table_dev, table_bytes, stream);
}
