// Scored K-best moments: td_sted_topk (include/tubedetr_hip.h has the rule; this file only has to agree with it).
//
// One workgroup of 16 waves per video, one launch for all K rounds.  In LDS for the whole kernel: ls / le (the two
// log-probability vectors), and per end e the best admissible start: best[e] = its score, arg[e] = its index.
//   * the log-softmax is td_sted_decode's, lane for lane (the first 256 lanes own the positions j = t (mod 256), four wave
//     sums added in wave order), so ls / le are its bits and row 0 is its answer;
//   * round 0 fills best / arg the way td_sted_decode does: a lane per end walks the starts below it;
//   * every round selects the best end with one block arg-max (larger score, then smaller e) - the pick;
//   * a pick invalidates best[e] only where arg[e] itself became inadmissible (the admissible sets only shrink), and a
//     lane per end tests that with the suppression predicate alone.  The ends that fail are recomputed by their WAVE:
//     for a fixed end e and an earlier pick (a, b) the suppressed starts are ONE interval that touches a
//     (suppressed_starts below: the union is constant for s >= a, the intersection for s < a, so both bounds are closed
//     integer forms), lane i computes the interval of pick i, the picks are kept sorted by a, and because interval i
//     touches a_i the admissible starts between a_(i-1) and a_i are exactly those above the prefix maximum of the upper
//     bounds and below the suffix minimum of the lower bounds.  That gives the <= k + 1 admissible ranges from uniform
//     lane reads (no cross-lane permutes, which would cost more than the walk), and the 64 lanes walk them together,
//     stride 64 (conflict-free LDS reads), comparing ls[s] + le[e] like round 0.
// No array lives in registers (no scratch), no atomics; every store is a vector store from one lane.
#include <climits>
#include <cmath>

#include "td_common.h"

namespace td {

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kSoftmaxLanes = 256;  // td_sted_decode's workgroup: its partition of the two sums
constexpr int kMaxK = 32;
constexpr int kMaxPositions = 3840;

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// reductions over the first four waves (the other lanes carry the identity), combined in td_sted_decode's order
__device__ __forceinline__ float block_sum4(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0 && threadIdx.x < kSoftmaxLanes) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}
__device__ __forceinline__ float block_max4(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0 && threadIdx.x < kSoftmaxLanes) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// n >= 0, d > 0
__device__ __forceinline__ long long div_floor(long long n, long long d) {
  if ((((unsigned long long)n | (unsigned long long)d) >> 32) == 0) return (long long)((unsigned)n / (unsigned)d);
  return n / d;
}

// the header's predicate: is (s, e) suppressed by the pick (a, b)?
__device__ __forceinline__ bool suppresses(int s, int e, int a, int b, long long num, long long den) {
  long long inter = (long long)min(e, b) - max(s, a) + 1;
  if (inter < 0) inter = 0;
  const long long uni = (long long)(e - s + 1) + (b - a + 1) - inter;
  return inter * den > num * uni;
}

// The starts s < e that the pick (a, b) takes from end e - suppressed, or the pick itself - as one interval [lo, hi];
// lo > hi: none.  A non-empty interval has lo <= a and hi >= a - 1.
//   s >= a (and s <= top = min(e, b), else nothing is shared): union = U0 = max(e, b) - a + 1, inter = top - s + 1, so
//     suppressed iff top - s + 1 > floor(num U0 / den), i.e. s <= top - floor(num U0 / den);
//   s <  a: inter = I0 = top - a + 1, union = (e - s + 1) + (b - a + 1) - I0, so suppressed iff
//     num (e - s + 1) < X = I0 den - num (b - a + 1 - I0): never for X <= 0, every s for num = 0, else
//     e - s + 1 <= ceil(X / num) - 1, i.e. s >= e + 2 - ceil(X / num).
__device__ __forceinline__ void suppressed_starts(int e, int a, int b, long long num, long long den, int& lo, int& hi) {
  lo = a;
  hi = a - 1;
  const int top = min(e, b);
  if (top >= a) {
    const long long U0 = (long long)max(e, b) - a + 1;
    const long long R = top - div_floor(num * U0, den);
    if (R >= a) hi = (int)R;
    const long long I0 = (long long)top - a + 1;
    if (num == 0) {
      lo = 0;
    } else {
      const long long X = I0 * den - num * ((long long)(b - a + 1) - I0);
      if (X > 0) {
        const long long L = max((long long)e + 2 - div_floor(X + num - 1, num), 0ll);
        if (L < a) lo = (int)L;
      }
    }
  }
  if (e == b) {  // the pick itself (its IoU of 1 is not above a threshold of 1)
    lo = min(lo, a);
    hi = max(hi, a);
  }
  hi = min(hi, e - 1);
}

__device__ __forceinline__ int wave_min_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}

// larger score first, then the smaller index; (-inf, INT_MAX) is "none"
__device__ __forceinline__ void wave_argbest(float& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (ov > v || (ov == v && oi < i)) {
      v = ov;
      i = oi;
    }
  }
}

__global__ __launch_bounds__(kThreads) void sted_topk_kernel(const float* __restrict__ steds, const unsigned char* __restrict__ valid,
                                                              const int* __restrict__ win_ptr, int n_windows, int T, int max_windows, int K,
                                                              long long num, long long den, long long* __restrict__ pairs,
                                                              float* __restrict__ scores, int* __restrict__ count) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ float red[4];
  __shared__ float sel_v[kWaves];
  __shared__ int sel_e[kWaves];
  __shared__ int pick_a[kMaxK], pick_b[kMaxK];  // the picks so far, sorted by a
  const int v = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int w0 = v, nw = 1;
  if (win_ptr) {
    w0 = win_ptr[v];
    nw = min(max(win_ptr[v + 1] - w0, 0), max_windows);
  }
  const int P = nw * T;  // <= max_windows * T <= kMaxPositions: what the launch sized smem for
  float* ls = smem;
  float* le = smem + P;
  float* best = smem + 2 * P;
  int* arg = (int*)(smem + 3 * P);

  for (int p = t; p < P; p += kThreads) {
    const int q = p / T;
    const int w = min(max(w0 + q, 0), n_windows - 1);
    const size_t idx = (size_t)w * T + (p - q * T);
    const bool ok = !valid || valid[idx] != 0;
    ls[p] = ok ? steds[idx * 2 + 0] : -INFINITY;
    le[p] = ok ? steds[idx * 2 + 1] : -INFINITY;
  }
  __syncthreads();
  for (int c = 0; c < 2; ++c) {
    float* d = c == 0 ? ls : le;
    float mx = -INFINITY;
    if (t < kSoftmaxLanes)
      for (int j = t; j < P; j += kSoftmaxLanes) mx = fmaxf(mx, d[j]);
    mx = block_max4(mx, red);
    float se = 0.f;
    if (t < kSoftmaxLanes)
      for (int j = t; j < P; j += kSoftmaxLanes) se += expf(d[j] - mx);
    se = block_sum4(se, red);  // its second barrier stands behind every read of the logits
    const float lse = logf(se);
    for (int j = t; j < P; j += kThreads) d[j] = (d[j] - mx) - lse;
  }
  __syncthreads();
  // round 0: per end the best start below it (td_sted_decode's loop)
  for (int e = t; e < P; e += kThreads) {
    float bv = -INFINITY;
    int bs = 0;
    const float lee = le[e];
    int s = 0;
    for (; s + 4 <= e; s += 4) {  // four starts per LDS read (ls is 16-byte aligned), compared in order
      const float4 q = *(const float4*)(ls + s);
      const float v0 = q.x + lee, v1 = q.y + lee, v2 = q.z + lee, v3 = q.w + lee;
      if (v0 > bv) { bv = v0; bs = s; }
      if (v1 > bv) { bv = v1; bs = s + 1; }
      if (v2 > bv) { bv = v2; bs = s + 2; }
      if (v3 > bv) { bv = v3; bs = s + 3; }
    }
    for (; s < e; ++s) {
      const float val = ls[s] + lee;
      if (val > bv) {
        bv = val;
        bs = s;
      }
    }
    best[e] = bv;
    arg[e] = bs;
  }

  int cnt = 0, na = 0, nb = 0;  // picks made; the newest one
  for (int k = 0; k < K; ++k) {
    if (k > 0) {
      // wave `wave` owns the ends e = wave (mod kWaves): 64 of them per step, a lane each, for the test
      for (int c = 0; c * 64 * kWaves < P; ++c) {
        const int e = (c * 64 + lane) * kWaves + wave;
        bool redo = false;
        if (e < P && finite_f(best[e])) {
          const int s = arg[e];
          redo = (s == na && e == nb) || suppresses(s, e, na, nb, num, den);
        }
        unsigned long long todo = __ballot(redo);
        while (todo) {
          const int l = __ffsll((long long)todo) - 1;
          todo &= todo - 1;
          const int ee = (c * 64 + l) * kWaves + wave;  // wave-uniform from here
          int a_i = ee, lo = INT_MAX, hi = -1;
          if (lane < k) {
            a_i = pick_a[lane];
            suppressed_starts(ee, a_i, pick_b[lane], num, den, lo, hi);
            if (lo > hi) {
              lo = INT_MAX;
              hi = -1;
            }
          }
          // lane i: the suffix minimum of the lower bounds, min over j >= i (k uniform lane reads instead of a wave scan)
          int sm = lo;
          for (int j = 1; j < k; ++j) {
            const int lo_j = __builtin_amdgcn_readlane(lo, j);
            if (lane < j) sm = min(sm, lo_j);
          }
          // range i <= k: the admissible starts of [a_(i-1), a_i - 1], with a_(-1) = 0 and a_k = e (lane k holds a_i = e,
          // no interval); pm = the prefix maximum of the upper bounds.  All wave-uniform.
          float bv = -INFINITY;
          int bs = INT_MAX;
          const float lee = le[ee];
          int pm = -1, a_prev = 0;
          for (int i = 0; i <= k; ++i) {
            const int a_cur = __builtin_amdgcn_readlane(a_i, i);
            const int l0 = max(a_prev, pm + 1);
            const int r0 = min(min(a_cur - 1, __builtin_amdgcn_readlane(sm, i) - 1), ee - 1);
#pragma unroll 4
            for (int p = l0 + lane; p <= r0; p += 64) {
              const float val = ls[p] + lee;
              if (val > bv) {
                bv = val;
                bs = p;
              }
            }
            pm = max(pm, __builtin_amdgcn_readlane(hi, i));
            a_prev = a_cur;
          }
          // the largest score, then the smallest start among the lanes that hold it: nearly always one lane
          const float m = wave_max(bv);
          const unsigned long long holders = __ballot(bv == m && bs != INT_MAX);
          if (holders == 0) {
            bs = 0;  // no admissible start is left: m = -inf keeps the end out of every later round
          } else if ((holders & (holders - 1)) == 0) {
            bs = __builtin_amdgcn_readlane(bs, __ffsll((long long)holders) - 1);
          } else {
            bs = wave_min_int(bv == m ? bs : INT_MAX);
          }
          bv = m;
          if (lane == 0) {
            best[ee] = bv;
            arg[ee] = bs;
          }
        }
      }
    }
    __syncthreads();
    float bv = -INFINITY;
    int be = INT_MAX;
    for (int e = t; e < P; e += kThreads) {
      const float x = best[e];
      if (finite_f(x) && x > bv) {
        bv = x;
        be = e;
      }
    }
    wave_argbest(bv, be);
    if (lane == 0) {
      sel_v[wave] = bv;
      sel_e[wave] = be;
    }
    __syncthreads();
    bv = sel_v[0];
    be = sel_e[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
      const float ov = sel_v[w];
      const int oe = sel_e[w];
      if (ov > bv || (ov == bv && oe < be)) {
        bv = ov;
        be = oe;
      }
    }
    if (be == INT_MAX) break;  // block-uniform: no admissible pair is left
    na = arg[be];
    nb = be;
    if (t == 0) {
      const size_t row = (size_t)v * K + k;
      pairs[row * 2 + 0] = na;
      pairs[row * 2 + 1] = nb;
      scores[row] = bv;
      int i = cnt;
      for (; i > 0 && pick_a[i - 1] > na; --i) {
        pick_a[i] = pick_a[i - 1];
        pick_b[i] = pick_b[i - 1];
      }
      pick_a[i] = na;
      pick_b[i] = nb;
    }
    ++cnt;
    __syncthreads();
  }
  for (int k = cnt + t; k < K; k += kThreads) {
    const size_t row = (size_t)v * K + k;
    pairs[row * 2 + 0] = -1;
    pairs[row * 2 + 1] = -1;
    scores[row] = -INFINITY;
  }
  if (t == 0) count[v] = cnt;
}

}  // namespace

}  // namespace td

extern "C" int td_sted_topk(const float* steds, const unsigned char* valid, const int* win_ptr, int n_videos, int n_windows, int T,
                            int max_windows, int K, int nms_num, int nms_den, long long* pairs, float* scores, int* count,
                            td_stream_t stream) {
  TD_REQUIRE(steds && pairs && scores && count, "td_sted_topk: null pointer (steds, pairs, scores, count)");
  TD_REQUIRE(n_videos >= 1 && T >= 1 && max_windows >= 1, "td_sted_topk: n_videos=%d, T=%d, max_windows=%d must be >= 1", n_videos, T, max_windows);
  TD_REQUIRE(n_windows >= (win_ptr ? 1 : n_videos), "td_sted_topk: n_windows=%d for %d videos", n_windows, n_videos);
  TD_REQUIRE(K >= 1 && K <= td::kMaxK, "td_sted_topk: K=%d outside 1..%d", K, td::kMaxK);
  TD_REQUIRE(nms_den >= 1 && nms_num >= 0 && nms_num <= nms_den, "td_sted_topk: nms %d/%d is not a fraction in [0, 1]", nms_num, nms_den);
  TD_REQUIRE((long long)max_windows * T <= td::kMaxPositions, "td_sted_topk: max_windows * T = %lld too long (max 3840 positions per video)",
             (long long)max_windows * T);
  const size_t lds = (size_t)4 * max_windows * T * sizeof(float);
  td::sted_topk_kernel<<<n_videos, td::kThreads, lds, (hipStream_t)stream>>>(steds, valid, win_ptr, n_windows, T, max_windows, K, nms_num, nms_den,
                                                                            pairs, scores, count);
  return td::check_launch("td_sted_topk");
}
