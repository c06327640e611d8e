// Optimizer-side tail of a training step as three HBM-bound launches over FLAT fp32 buffers (all trainable
// parameters of the model back to back, gradients in the same order - the buffer the data-parallel exchange already
// produces): gradient-norm partial sums, norm finalize (clip coefficient + step counter), fused clip + AdamW + EMA.
// Replaces, per step, ~3 elementwise torch launches for each of the 923 state-dict entries:
//   torch.nn.utils.clip_grad_norm_ + optimizer.step()            engine.py:147-151
//   torch.optim.AdamW with three name-based parameter groups      main.py:381-413
//   update_ema(model, model_ema, decay)                           util/optim.py:8-25
// Learning rates (adjust_learning_rate, util/optim.py:28-95, stays host code: three scalars) and the step counter live in
// device memory, so the whole tail can be captured in a HIP graph behind the backward pass.
#include "td_common.h"

namespace td {

struct Segs {
  td_optim_segment s[TD_OPTIM_MAX_SEGMENTS];
  int n;
};

__device__ __forceinline__ int find_seg(const Segs& sg, long long i) {
  int k = 0;
#pragma unroll 4
  for (int j = 1; j < sg.n; ++j) k = (i >= sg.s[j].begin) ? j : k;
  return k;
}

// tree sums of N doubles per thread over the 256 threads of a workgroup (red: N rows of 256); every one of the N sums is
// formed in the same order whatever N is; the results are valid in thread 0
template <int N>
__device__ __forceinline__ void block_sum(double (&acc)[N], double* red) {
#pragma unroll
  for (int q = 0; q < N; ++q) red[q * 256 + threadIdx.x] = acc[q];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
#pragma unroll
      for (int q = 0; q < N; ++q) red[q * 256 + threadIdx.x] += red[q * 256 + threadIdx.x + o];
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < N; ++q) acc[q] = red[q * 256];
}

// per-group sums beside the total.  A thread's grid-stride steps are gridDim.x * 1024 elements apart, so the group changes a
// handful of times per thread: the terms go into ONE running sum (one extra add per term), which is moved into its group's
// slot - an add of +0.0 to the others, no runtime-indexed register array - only when the group changes and at the end
struct GroupAcc {
  double a[TD_OPTIM_MAX_GROUPS] = {0.0, 0.0, 0.0, 0.0};
  double run = 0.0;
  int cur = 0;
  __device__ __forceinline__ void flush() {
#pragma unroll
    for (int q = 0; q < TD_OPTIM_MAX_GROUPS; ++q) a[q] += (cur == q) ? run : 0.0;
    run = 0.0;
  }
  __device__ __forceinline__ void add(int group, double s) {
    if (group != cur) {
      flush();
      cur = group;
    }
    run += s;
  }
};
struct NoGroupAcc {
  __device__ __forceinline__ void add(int, double) {}
};

// sum of g^2 over the workgroup's grid-stride share (inactive segments = parameters without a gradient are skipped like
// clip_grad_norm_ skips p.grad is None); `ga` sees every term that `acc` sees, and never changes what `acc` becomes
template <class GA>
__device__ __forceinline__ double grad_sq_thread(const float* __restrict__ g, long long n, const Segs& sg, GA& ga) {
  const long long nv = n >> 2;
  double acc = 0.0;
  for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < nv; v += (long long)gridDim.x * 256) {
    const float4 x = ((const float4*)g)[v];
    const long long i0 = v << 2;
    const int k0 = find_seg(sg, i0), k1 = find_seg(sg, i0 + 3);
    if (k0 == k1) {
      if (sg.s[k0].active) {
        const double s = (double)x.x * x.x + (double)x.y * x.y + (double)x.z * x.z + (double)x.w * x.w;
        acc += s;
        ga.add(sg.s[k0].group, s);
      }
    } else {
      const float e[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = find_seg(sg, i0 + q);
        if (sg.s[k].active) {
          const double s = (double)e[q] * e[q];
          acc += s;
          ga.add(sg.s[k].group, s);
        }
      }
    }
  }
  if (blockIdx.x == 0)
    for (long long i = (nv << 2) + threadIdx.x; i < n; i += 256) {
      const int k = find_seg(sg, i);
      if (sg.s[k].active) {
        const double s = (double)g[i] * g[i];
        acc += s;
        ga.add(sg.s[k].group, s);
      }
    }
  return acc;
}

// partial[block] = the workgroup's sum
__global__ __launch_bounds__(256) void grad_sq_partial_kernel(const float* __restrict__ g, long long n, Segs sg, double* partial) {
  __shared__ double red[256];
  NoGroupAcc ga;
  double t[1] = {grad_sq_thread(g, n, sg, ga)};
  block_sum(t, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = t[0];
}

// the same, plus gpartial[group][block] (row stride TD_OPTIM_NORM_BLOCKS) = the workgroup's sum over each group's active elements
__global__ __launch_bounds__(256) void grad_sq_partial_groups_kernel(const float* __restrict__ g, long long n, Segs sg, double* partial,
                                                                     double* gpartial) {
  __shared__ double red[(1 + TD_OPTIM_MAX_GROUPS) * 256];
  GroupAcc ga;
  double t[1 + TD_OPTIM_MAX_GROUPS];
  t[0] = grad_sq_thread(g, n, sg, ga);
  ga.flush();
#pragma unroll
  for (int q = 0; q < TD_OPTIM_MAX_GROUPS; ++q) t[1 + q] = ga.a[q];
  block_sum(t, red);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = t[0];
#pragma unroll
    for (int q = 0; q < TD_OPTIM_MAX_GROUPS; ++q) gpartial[(size_t)q * TD_OPTIM_NORM_BLOCKS + blockIdx.x] = t[1 + q];
  }
}

// one workgroup: total norm, clip coefficient min(1, max_norm / (norm + 1e-6)) (max_norm <= 0: no clipping), step += 1
__global__ __launch_bounds__(256) void grad_norm_finalize_kernel(const double* partial, int nblocks, float max_norm, float* norm_clip, int* step) {
  __shared__ double red[256];
  double acc[1] = {0.0};
  for (int i = threadIdx.x; i < nblocks; i += 256) acc[0] += partial[i];
  block_sum(acc, red);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(acc[0]);
    norm_clip[0] = norm;
    float c = 1.f;
    if (max_norm > 0.f) c = fminf(max_norm / (norm + 1e-6f), 1.f);
    norm_clip[1] = c;
    if (step) step[0] += 1;
  }
}

// device block of the guarded tail (td_guard_bytes): header + ring of td_step_record
struct GuardHeader {
  int attempts, skipped, consecutive_skipped, applied_now;
};
static_assert(sizeof(GuardHeader) == 16 && sizeof(td_step_record) == 40, "layout documented in include/tubedetr_hip.h");

// one workgroup: the total exactly as grad_norm_finalize_kernel forms it (the group sums ride along in the same tree); then
// thread 0 decides on the fp32 norm it writes.  Finite: clip coefficient and step += 1 as above.  Not finite: coefficient 0,
// step untouched, the update that follows returns at once (adamw_ema_guarded_kernel reads applied_now).  Counters and one
// ring record are written either way.
__global__ __launch_bounds__(256) void grad_norm_finalize_guarded_kernel(const double* partial, const double* gpartial, int nblocks, float max_norm,
                                                                         float* norm_clip, int* step, const float* loss, GuardHeader* guard,
                                                                         int history) {
  __shared__ double red[(1 + TD_OPTIM_MAX_GROUPS) * 256];
  double acc[1 + TD_OPTIM_MAX_GROUPS] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = threadIdx.x; i < nblocks; i += 256) {
    acc[0] += partial[i];
#pragma unroll
    for (int q = 0; q < TD_OPTIM_MAX_GROUPS; ++q) acc[1 + q] += gpartial[(size_t)q * TD_OPTIM_NORM_BLOCKS + i];
  }
  block_sum(acc, red);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(acc[0]);
    const bool ok = isfinite(norm);
    float c = 0.f;
    if (ok) {
      c = 1.f;
      if (max_norm > 0.f) c = fminf(max_norm / (norm + 1e-6f), 1.f);
      if (step) step[0] += 1;
    }
    norm_clip[0] = norm;
    norm_clip[1] = c;
    GuardHeader h = *guard;
    h.attempts += 1;
    h.applied_now = ok ? 1 : 0;
    h.skipped += ok ? 0 : 1;
    h.consecutive_skipped = ok ? 0 : h.consecutive_skipped + 1;
    *guard = h;
    if (history > 0) {
      td_step_record r;
      r.attempt = h.attempts;
      r.step = step ? step[0] : 0;
      r.applied = h.applied_now;
      r.norm = norm;
      r.clip = c;
      r.loss = loss ? loss[0] : __builtin_nanf("");
#pragma unroll
      for (int q = 0; q < TD_OPTIM_MAX_GROUPS; ++q) r.group_norm[q] = (float)sqrt(acc[1 + q]);
      ((td_step_record*)(guard + 1))[(unsigned)(h.attempts - 1) % (unsigned)history] = r;
    }
  }
}

struct AdamArgs {
  float b1, b2, eps, wd, ema_decay;
};

__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, float* ema, float lr, float clip, float bc1, float bc2s, const AdamArgs& a) {
  g *= clip;
  p *= 1.f - lr * a.wd;                 // decoupled weight decay
  m += (g - m) * (1.f - a.b1);          // exp_avg.lerp_(grad, 1 - beta1)
  v = v * a.b2 + (1.f - a.b2) * g * g;  // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
  const float denom = sqrtf(v) / bc2s + a.eps;
  p -= (lr / bc1) * (m / denom);
  if (ema) *ema = *ema * a.ema_decay + (1.f - a.ema_decay) * p;
}

// a parameter without a gradient keeps its value and its moments, but update_ema (util/optim.py:8-25) still moves its EMA
__device__ __forceinline__ float ema_only(float e, float p, const AdamArgs& a) { return e * a.ema_decay + (1.f - a.ema_decay) * p; }

__device__ __forceinline__ void adamw_ema_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                               float* __restrict__ ema, long long n, const Segs& sg, const float* __restrict__ lr_dev,
                                               const float* __restrict__ norm_clip, const int* __restrict__ step_dev, const AdamArgs& a) {
  const float clip = norm_clip ? norm_clip[1] : 1.f;
  const int step = step_dev[0];  // already incremented for this update
  // 1 - beta^t as -expm1(t * log(beta)): 1.f - powf(beta2, t) cancels while t is small (t = 3: 0.997 -> 0.003 carries the
  // rounding of 0.997, 1e-5 relative in every update); beta - 1 is exact in fp32
  const float bc1 = -expm1f((float)step * log1pf(a.b1 - 1.f));
  const float bc2s = sqrtf(-expm1f((float)step * log1pf(a.b2 - 1.f)));
  float lrs[TD_OPTIM_MAX_GROUPS];
#pragma unroll
  for (int q = 0; q < TD_OPTIM_MAX_GROUPS; ++q) lrs[q] = lr_dev[q];
  const long long nv = n >> 2;
  for (long long vi = (long long)blockIdx.x * 256 + threadIdx.x; vi < nv; vi += (long long)gridDim.x * 256) {
    const long long i0 = vi << 2;
    const int k0 = find_seg(sg, i0), k1 = find_seg(sg, i0 + 3);
    if (k0 == k1 && !sg.s[k0].active) {
      if (ema) {
        const float4 P = ((const float4*)p)[vi];
        float4 E = ((float4*)ema)[vi];
        E.x = ema_only(E.x, P.x, a); E.y = ema_only(E.y, P.y, a); E.z = ema_only(E.z, P.z, a); E.w = ema_only(E.w, P.w, a);
        ((float4*)ema)[vi] = E;
      }
      continue;
    }
    float4 P = ((float4*)p)[vi], G = ((const float4*)g)[vi], M = ((float4*)m)[vi], V = ((float4*)v)[vi], E = make_float4(0, 0, 0, 0);
    if (ema) E = ((float4*)ema)[vi];
    float* pe = (float*)&P; float* ge = (float*)&G; float* me = (float*)&M; float* ve = (float*)&V; float* ee = (float*)&E;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k = (k0 == k1) ? k0 : find_seg(sg, i0 + q);
      if (!sg.s[k].active) {
        if (ema) ee[q] = ema_only(ee[q], pe[q], a);
        continue;
      }
      adam_elem(pe[q], ge[q], me[q], ve[q], ema ? &ee[q] : nullptr, lrs[sg.s[k].group], clip, bc1, bc2s, a);
    }
    ((float4*)p)[vi] = P; ((float4*)m)[vi] = M; ((float4*)v)[vi] = V;
    if (ema) ((float4*)ema)[vi] = E;
  }
  if (blockIdx.x == 0)
    for (long long i = (nv << 2) + threadIdx.x; i < n; i += 256) {
      const int k = find_seg(sg, i);
      if (!sg.s[k].active) {
        if (ema) ema[i] = ema_only(ema[i], p[i], a);
        continue;
      }
      adam_elem(p[i], g[i], m[i], v[i], ema ? &ema[i] : nullptr, lrs[sg.s[k].group], clip, bc1, bc2s, a);
    }
}

__global__ __launch_bounds__(256) void adamw_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, float* __restrict__ ema, long long n, Segs sg,
                                                        const float* __restrict__ lr_dev, const float* __restrict__ norm_clip,
                                                        const int* __restrict__ step_dev, AdamArgs a) {
  adamw_ema_body(p, g, m, v, ema, n, sg, lr_dev, norm_clip, step_dev, a);
}

// the same update behind the decision of grad_norm_finalize_guarded_kernel: one read of applied_now per workgroup, and a
// skipped step returns before any load or store of p / m / v / ema (the EMA of inactive segments included)
__global__ __launch_bounds__(256) void adamw_ema_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                float* __restrict__ v, float* __restrict__ ema, long long n, Segs sg,
                                                                const float* __restrict__ lr_dev, const float* __restrict__ norm_clip,
                                                                const int* __restrict__ step_dev, AdamArgs a, const GuardHeader* guard) {
  __shared__ int applied;
  if (threadIdx.x == 0) applied = guard->applied_now;
  __syncthreads();
  if (!applied) return;
  adamw_ema_body(p, g, m, v, ema, n, sg, lr_dev, norm_clip, step_dev, a);
}

static int fill_segs(Segs& sg, const td_optim_segment* segs, int n_segs, size_t n, const char* who) {
  TD_REQUIRE(segs && n_segs >= 1 && n_segs <= TD_OPTIM_MAX_SEGMENTS, "%s: 1..%d segments expected", who, TD_OPTIM_MAX_SEGMENTS);
  long long at = 0;
  for (int i = 0; i < n_segs; ++i) {
    TD_REQUIRE(segs[i].begin == at && segs[i].end > segs[i].begin, "%s: segments must tile [0, n) in order", who);
    TD_REQUIRE(segs[i].group >= 0 && segs[i].group < TD_OPTIM_MAX_GROUPS, "%s: group out of range", who);
    sg.s[i] = segs[i];
    at = segs[i].end;
  }
  TD_REQUIRE((size_t)at == n, "%s: segments cover %lld of %zu elements", who, at, n);
  sg.n = n_segs;
  return TD_OK;
}

static unsigned opt_grid(size_t n) {
  size_t b = (n / 4 + 255) / 256;
  if (b < 1) b = 1;
  if (b > TD_OPTIM_NORM_BLOCKS) b = TD_OPTIM_NORM_BLOCKS;
  return (unsigned)b;
}

static unsigned adam_grid(size_t n) {
  size_t b = (n / 4 + 255) / 256;
  if (b > 8192) b = 8192;
  if (b < 1) b = 1;
  return (unsigned)b;
}

}  // namespace td
using namespace td;

extern "C" size_t td_grad_norm_ws_bytes(void) { return (size_t)TD_OPTIM_NORM_BLOCKS * sizeof(double); }

extern "C" int td_grad_norm_clip(const float* grad, size_t n, const td_optim_segment* segs, int n_segs, float max_norm, void* ws,
                                 size_t ws_bytes, float* norm_clip, int* step, td_stream_t stream) {
  TD_REQUIRE(grad && ws && norm_clip && n > 0, "td_grad_norm_clip: null pointer / empty buffer");
  TD_REQUIRE(ws_bytes >= td_grad_norm_ws_bytes(), "td_grad_norm_clip: workspace smaller than td_grad_norm_ws_bytes()");
  TD_REQUIRE(((uintptr_t)grad & 15) == 0, "td_grad_norm_clip: the flat buffer must be 16-byte aligned");
  Segs sg;
  int rc = fill_segs(sg, segs, n_segs, n, "td_grad_norm_clip");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const unsigned g = opt_grid(n);
  grad_sq_partial_kernel<<<g, 256, 0, st>>>(grad, (long long)n, sg, (double*)ws);
  grad_norm_finalize_kernel<<<1, 256, 0, st>>>((const double*)ws, (int)g, max_norm, norm_clip, step);
  return check_launch("td_grad_norm_clip");
}

extern "C" int td_adamw_ema_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, size_t n,
                                 const td_optim_segment* segs, int n_segs, const float* lr_dev, const float* norm_clip,
                                 const int* step_dev, float beta1, float beta2, float eps, float weight_decay, float ema_decay,
                                 td_stream_t stream) {
  TD_REQUIRE(param && grad && exp_avg && exp_avg_sq && lr_dev && step_dev && n > 0, "td_adamw_ema_step: null pointer / empty buffer");
  TD_REQUIRE((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)ema) & 15) == 0,
             "td_adamw_ema_step: flat buffers must be 16-byte aligned");
  Segs sg;
  int rc = fill_segs(sg, segs, n_segs, n, "td_adamw_ema_step");
  if (rc) return rc;
  AdamArgs a = {beta1, beta2, eps, weight_decay, ema_decay};
  adamw_ema_kernel<<<adam_grid(n), 256, 0, (hipStream_t)stream>>>(param, grad, exp_avg, exp_avg_sq, ema, (long long)n, sg, lr_dev, norm_clip,
                                                                step_dev, a);
  return check_launch("td_adamw_ema_step");
}

extern "C" size_t td_grad_norm_guard_ws_bytes(void) { return (size_t)(1 + TD_OPTIM_MAX_GROUPS) * TD_OPTIM_NORM_BLOCKS * sizeof(double); }

extern "C" size_t td_guard_bytes(int history) { return sizeof(GuardHeader) + (size_t)(history > 0 ? history : 0) * sizeof(td_step_record); }

extern "C" int td_grad_norm_clip_guarded(const float* grad, size_t n, const td_optim_segment* segs, int n_segs, float max_norm, void* ws,
                                         size_t ws_bytes, float* norm_clip, int* step, const float* loss, void* guard, int history,
                                         td_stream_t stream) {
  TD_REQUIRE(grad && ws && norm_clip && n > 0, "td_grad_norm_clip_guarded: null pointer / empty buffer");
  TD_REQUIRE(guard, "td_grad_norm_clip_guarded: null guard block");
  TD_REQUIRE(history >= 0 && history <= TD_GUARD_HISTORY_MAX, "td_grad_norm_clip_guarded: history %d outside 0..%d", history, TD_GUARD_HISTORY_MAX);
  TD_REQUIRE(ws_bytes >= td_grad_norm_guard_ws_bytes(), "td_grad_norm_clip_guarded: workspace smaller than td_grad_norm_guard_ws_bytes()");
  TD_REQUIRE(((uintptr_t)grad & 15) == 0, "td_grad_norm_clip_guarded: the flat buffer must be 16-byte aligned");
  TD_REQUIRE(((uintptr_t)ws & 7) == 0 && ((uintptr_t)guard & 3) == 0, "td_grad_norm_clip_guarded: workspace (8 bytes) / guard block (4 bytes) not aligned");
  Segs sg;
  int rc = fill_segs(sg, segs, n_segs, n, "td_grad_norm_clip_guarded");
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const unsigned g = opt_grid(n);
  double* partial = (double*)ws;
  double* gpartial = partial + TD_OPTIM_NORM_BLOCKS;
  grad_sq_partial_groups_kernel<<<g, 256, 0, st>>>(grad, (long long)n, sg, partial, gpartial);
  grad_norm_finalize_guarded_kernel<<<1, 256, 0, st>>>(partial, gpartial, (int)g, max_norm, norm_clip, step, loss, (GuardHeader*)guard, history);
  return check_launch("td_grad_norm_clip_guarded");
}

extern "C" int td_adamw_ema_step_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, size_t n,
                                         const td_optim_segment* segs, int n_segs, const float* lr_dev, const float* norm_clip,
                                         const int* step_dev, float beta1, float beta2, float eps, float weight_decay, float ema_decay,
                                         const void* guard, td_stream_t stream) {
  TD_REQUIRE(param && grad && exp_avg && exp_avg_sq && lr_dev && step_dev && n > 0, "td_adamw_ema_step_guarded: null pointer / empty buffer");
  TD_REQUIRE(guard && ((uintptr_t)guard & 3) == 0, "td_adamw_ema_step_guarded: null / misaligned guard block");
  TD_REQUIRE((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)ema) & 15) == 0,
             "td_adamw_ema_step_guarded: flat buffers must be 16-byte aligned");
  Segs sg;
  int rc = fill_segs(sg, segs, n_segs, n, "td_adamw_ema_step_guarded");
  if (rc) return rc;
  AdamArgs a = {beta1, beta2, eps, weight_decay, ema_decay};
  adamw_ema_guarded_kernel<<<adam_grid(n), 256, 0, (hipStream_t)stream>>>(param, grad, exp_avg, exp_avg_sq, ema, (long long)n, sg, lr_dev, norm_clip,
                                                                        step_dev, a, (const GuardHeader*)guard);
  return check_launch("td_adamw_ema_step_guarded");
}
