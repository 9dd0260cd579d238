// Weight averaging (EMA / SWA), the exact exchange of two tensor lists and the learning-rate schedule on the device (DESIGN
// section 7, "8f-11"), on the multi-tensor frame of csrc/multi_tensor.hpp.  All operands f32.
//
// anemoi_average_constants: one wave, thread 0.  From the device counter n_averaged, optionally the optimizer's device step
// counter t (steps completed) and its list-wide skip flag, it writes avg[4] = {w, active, copy, n_after}:
//   active = !skip && (no t || (t >= start_step && (t - start_step) % every == 0))
//   active, n == 0:  copy = 1, w = 1
//   active, EMA:     w = 1 - d,  d = use_warmup ? min(decay, (1 + n) / (10 + n)) : decay
//   active, SWA:     w = 1 / (n + 1)
// w is evaluated in f64 and rounded once; n_averaged is advanced only when active; inactive: w = 0, n_after = n.
//
// anemoi_multi_average, per element (params are only read; 8 bytes read, 4 written):
//   inactive: the kernel returns before its first load;  copy: s <- p, bit for bit (no arithmetic touches the value);
//   else s <- fmaf(p - s, w, s): two roundings (the difference, the fmaf), torch's lerp / SWA form.
// The result is a function of the values alone: no sums, no atomics, every element owned by one thread.
//
// anemoi_multi_swap: a[i] <-> b[i]; an element is read by its one owner before that owner writes it.
//
// anemoi_lr_schedule: one wave, thread g = parameter group g.  From the group's device step counter t (steps completed):
//   t < warmup_steps:  warmup_start + t (base - warmup_start) / warmup_steps
//   else, tc = warmup_prefix ? t - warmup_steps : t:   tc < T:  lr_min + 0.5 (base - lr_min)(1 + cos(pi tc / T));   else lr_min
// in f64, rounded once to the group's device f32 lr.
#include "multi_tensor.hpp"

#pragma clang fp contract(off)

namespace anemoi {

constexpr int AVG_W = 0, AVG_ACTIVE = 1, AVG_COPY = 2, AVG_N_AFTER = 3, AVG_CONSTS = 4;
constexpr int AVG_KIND_EMA = 0, AVG_KIND_SWA = 1;

struct AverageArgs {
  OptFrame f;
  const float* p[OPT_MAX_TENSORS];
  float* s[OPT_MAX_TENSORS];
  const float* avg;
};
static_assert(sizeof(AverageArgs) <= 4096, "the argument block of one launch is limited to 4 KB");

struct SwapArgs {
  OptFrame f;
  float* a[OPT_MAX_TENSORS];
  float* b[OPT_MAX_TENSORS];
};

struct AverageConstantsArgs {
  float* n_averaged;
  const float* step;  // or null: every call counts
  const float* skip;  // or null
  float* avg;
  double decay;
  int64_t start_step, every;
  int32_t kind, use_warmup;
};

struct LrScheduleArgs {
  int32_t n_groups;
  const float* step[OPT_MAX_GROUPS];
  float* lr[OPT_MAX_GROUPS];
  double base[OPT_MAX_GROUPS], lr_min[OPT_MAX_GROUPS], warmup_start[OPT_MAX_GROUPS];
  int64_t warmup_steps[OPT_MAX_GROUPS], total_steps[OPT_MAX_GROUPS];
  int32_t warmup_prefix[OPT_MAX_GROUPS];
};
static_assert(sizeof(LrScheduleArgs) <= 4096, "the argument block of one launch is limited to 4 KB");

__global__ __launch_bounds__(64) void average_constants_kernel(const AverageConstantsArgs a) {
  if (threadIdx.x != 0) return;
  const float n = *a.n_averaged;
  bool active = a.skip == nullptr || *a.skip == 0.f;
  if (active && a.step != nullptr) {
    const int64_t t = (int64_t)*a.step;
    active = t >= a.start_step && (t - a.start_step) % a.every == 0;
  }
  float w = 0.f;
  bool copy = false;
  if (active) {
    if (n == 0.f) {
      copy = true;
      w = 1.f;
    } else if (a.kind == AVG_KIND_SWA) {
      w = (float)(1.0 / ((double)n + 1.0));
    } else {
      double d = a.decay;
      if (a.use_warmup) {
        const double ramp = (1.0 + (double)n) / (10.0 + (double)n);
        d = ramp < d ? ramp : d;
      }
      w = (float)(1.0 - d);
    }
  }
  const float n_after = active ? n + 1.f : n;
  a.avg[AVG_W] = w;
  a.avg[AVG_ACTIVE] = active ? 1.f : 0.f;
  a.avg[AVG_COPY] = copy ? 1.f : 0.f;
  a.avg[AVG_N_AFTER] = n_after;
  if (active) *a.n_averaged = n_after;
}

template <bool FULL>
__device__ __forceinline__ void avg_copy_chunk(const float* __restrict__ p, float* __restrict__ s, int cnt, bool vec) {
  float xp[OPT_PASSES][4];
#pragma unroll
  for (int u = 0; u < OPT_PASSES; ++u) opt_load4<FULL>(p, (u * 256 + (int)threadIdx.x) * 4, cnt, vec, xp[u]);
#pragma unroll
  for (int u = 0; u < OPT_PASSES; ++u) {
    const int i = (u * 256 + (int)threadIdx.x) * 4;
    if (!FULL && i >= cnt) break;
    opt_store4<FULL>(s, i, cnt, vec, xp[u]);
  }
}

template <bool FULL>
__device__ __forceinline__ void avg_lerp_chunk(const float* __restrict__ p, float* __restrict__ s, int cnt, bool vec, float w) {
  float xp[OPT_PASSES][4], xs[OPT_PASSES][4];
#pragma unroll
  for (int u = 0; u < OPT_PASSES; ++u) {
    const int i = (u * 256 + (int)threadIdx.x) * 4;
    opt_load4<FULL>(p, i, cnt, vec, xp[u]);
    opt_load4<FULL>(s, i, cnt, vec, xs[u]);
  }
#pragma unroll
  for (int u = 0; u < OPT_PASSES; ++u) {
    const int i = (u * 256 + (int)threadIdx.x) * 4;
    if (!FULL && i >= cnt) break;
#pragma unroll
    for (int k = 0; k < 4; ++k) xs[u][k] = fmaf(xp[u][k] - xs[u][k], w, xs[u][k]);
    opt_store4<FULL>(s, i, cnt, vec, xs[u]);
  }
}

template <bool FULL>
__device__ __forceinline__ void swap_chunk(float* __restrict__ a, float* __restrict__ b, int cnt, bool vec) {
  float xa[OPT_PASSES][4], xb[OPT_PASSES][4];
#pragma unroll
  for (int u = 0; u < OPT_PASSES; ++u) {
    const int i = (u * 256 + (int)threadIdx.x) * 4;
    opt_load4<FULL>(a, i, cnt, vec, xa[u]);
    opt_load4<FULL>(b, i, cnt, vec, xb[u]);
  }
#pragma unroll
  for (int u = 0; u < OPT_PASSES; ++u) {
    const int i = (u * 256 + (int)threadIdx.x) * 4;
    if (!FULL && i >= cnt) break;
    opt_store4<FULL>(a, i, cnt, vec, xb[u]);
    opt_store4<FULL>(b, i, cnt, vec, xa[u]);
  }
}

__global__ __launch_bounds__(256) void multi_average_kernel(const AverageArgs a) {
  const float* __restrict__ cs = a.avg;
  if (cs[AVG_ACTIVE] == 0.f) return;
  const float w = cs[AVG_W];
  const bool copy = cs[AVG_COPY] != 0.f;
  const int b = blockIdx.x, ti = opt_find(a.f, b);
  const int64_t e0 = (int64_t)(b - a.f.chunk_start[ti]) * OPT_CHUNK, left = a.f.numel[ti] - e0;
  const int cnt = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
  const float* __restrict__ p = a.p[ti] + e0;
  float* __restrict__ s = a.s[ti] + e0;
  const bool vec = ((((uintptr_t)a.p[ti] | (uintptr_t)a.s[ti]) & 15) == 0);
  const bool full = vec && cnt == OPT_CHUNK;
  if (copy) {
    if (full) avg_copy_chunk<true>(p, s, cnt, vec);
    else avg_copy_chunk<false>(p, s, cnt, vec);
  } else {
    if (full) avg_lerp_chunk<true>(p, s, cnt, vec, w);
    else avg_lerp_chunk<false>(p, s, cnt, vec, w);
  }
}

__global__ __launch_bounds__(256) void multi_swap_kernel(const SwapArgs a) {
  const int b = blockIdx.x, ti = opt_find(a.f, b);
  const int64_t e0 = (int64_t)(b - a.f.chunk_start[ti]) * OPT_CHUNK, left = a.f.numel[ti] - e0;
  const int cnt = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
  float* __restrict__ x = a.a[ti] + e0;
  float* __restrict__ y = a.b[ti] + e0;
  const bool vec = ((((uintptr_t)a.a[ti] | (uintptr_t)a.b[ti]) & 15) == 0);
  if (vec && cnt == OPT_CHUNK) swap_chunk<true>(x, y, cnt, vec);
  else swap_chunk<false>(x, y, cnt, vec);
}

__global__ __launch_bounds__(64) void lr_schedule_kernel(const LrScheduleArgs a) {
  const int g = threadIdx.x;
  if (g >= a.n_groups) return;
  const int64_t t = (int64_t)*a.step[g], wu = a.warmup_steps[g], T = a.total_steps[g];
  const double base = a.base[g], lo = a.lr_min[g];
  double lr;
  if (t < wu) {
    lr = a.warmup_start[g] + (double)t * (base - a.warmup_start[g]) / (double)wu;
  } else {
    const int64_t tc = a.warmup_prefix[g] ? t - wu : t;
    lr = tc < T ? lo + 0.5 * (base - lo) * (1.0 + cos(3.14159265358979323846 * (double)tc / (double)T)) : lo;
  }
  *a.lr[g] = (float)lr;
}

// the list of an entry point with its own argument block, as the frame's helpers take it
static anemoi_multi_tensor_args avg_as_list(int64_t n_tensors, const int64_t* numel) {
  anemoi_multi_tensor_args l = {};
  l.struct_bytes = (int64_t)sizeof(anemoi_multi_tensor_args);
  l.n_tensors = n_tensors;
  l.numel = numel;
  return l;
}

static bool avg_list_is_empty(const anemoi_multi_tensor_args& l) {
  for (int64_t i = 0; i < l.n_tensors; ++i)
    if (l.numel[i] > 0) return false;
  return true;
}


// While a launch trail is armed: one record per non-empty tensor of the list, "who:what[i]" with i the tensor's index in the list
// as [1, numel].  Unarmed this is one thread-local load.
static int avg_note_list(int rc, const char* who, const char* what, const anemoi_multi_tensor_args* a, void* const* tensors,
                         hipStream_t st) {
  if (rc != ANEMOI_OK || trail::armed_state() == nullptr) return rc;
  char tag[48];
  for (int64_t i = 0; i < a->n_tensors && rc == ANEMOI_OK; ++i) {
    if (a->numel[i] == 0) continue;
    snprintf(tag, sizeof(tag), "%s[%lld]", what, (long long)i);
    rc = trail::note(rc, who, tag, ANEMOI_F32, tensors[i], a->numel[i], 1, a->numel[i], st);
  }
  return rc;
}

}  // namespace anemoi

using namespace anemoi;

#define AVG_REQUIRE_BLOCK(a, type)                                                                                             \
  ANEMOI_REQUIRE((a) != nullptr, ANEMOI_ERR_INVALID, "%s: null argument block", who);                                          \
  ANEMOI_REQUIRE((a)->struct_bytes == (int64_t)sizeof(type), ANEMOI_ERR_INVALID,                                               \
                 "%s: argument block of %lld bytes, this library expects %lld (header / library out of sync)", who,            \
                 (long long)(a)->struct_bytes, (long long)sizeof(type))

extern "C" {

int anemoi_average_constants(const anemoi_average_constants_args* c, anemoi_stream_t stream) {
  const char* who = "anemoi_average_constants";
  AVG_REQUIRE_BLOCK(c, anemoi_average_constants_args);
  ANEMOI_REQUIRE(c->n_averaged != nullptr, ANEMOI_ERR_INVALID, "%s: null pointer (n_averaged)", who);
  ANEMOI_REQUIRE(c->avg != nullptr, ANEMOI_ERR_INVALID, "%s: null pointer (avg)", who);
  ANEMOI_REQUIRE(c->kind == ANEMOI_AVERAGE_EMA || c->kind == ANEMOI_AVERAGE_SWA, ANEMOI_ERR_INVALID,
                 "%s: kind %d is neither ANEMOI_AVERAGE_EMA nor ANEMOI_AVERAGE_SWA", who, (int)c->kind);
  ANEMOI_REQUIRE(c->decay >= 0.0 && c->decay < 1.0, ANEMOI_ERR_INVALID, "%s: decay = %g is not in [0, 1)", who, c->decay);
  ANEMOI_REQUIRE(c->every >= 1, ANEMOI_ERR_INVALID, "%s: every = %lld < 1", who, (long long)c->every);
  ANEMOI_REQUIRE(c->start_step >= 0, ANEMOI_ERR_INVALID, "%s: start_step = %lld < 0", who, (long long)c->start_step);
  static_assert(ANEMOI_AVERAGE_EMA == AVG_KIND_EMA && ANEMOI_AVERAGE_SWA == AVG_KIND_SWA, "header and kernel disagree");
  hipStream_t st = as_stream(stream);
  AverageConstantsArgs k = {};
  k.n_averaged = c->n_averaged;
  k.step = c->step;
  k.skip = c->skip;
  k.avg = c->avg;
  k.decay = c->decay;
  k.start_step = c->start_step;
  k.every = c->every;
  k.kind = c->kind;
  k.use_warmup = c->use_warmup != 0;
  hipLaunchKernelGGL(average_constants_kernel, dim3(1), dim3(64), 0, st, k);
  return trail::note(check_launch(who), who, "avg", ANEMOI_F32, c->avg, AVG_CONSTS, 1, AVG_CONSTS, st);
}

int anemoi_multi_average(const anemoi_multi_average_args* a, anemoi_stream_t stream) {
  const char* who = "anemoi_multi_average";
  AVG_REQUIRE_BLOCK(a, anemoi_multi_average_args);
  const anemoi_multi_tensor_args l = avg_as_list(a->n_tensors, a->numel);
  void* const* arrays[2] = {a->params, a->shadow};
  const char* names[2] = {"params", "shadow"};
  if (int rc = opt_check_list(who, &l, 2, arrays, names)) return rc;
  ANEMOI_REQUIRE(a->avg != nullptr, ANEMOI_ERR_INVALID, "%s: null pointer (avg)", who);
  if (avg_list_is_empty(l)) return ANEMOI_OK;
  hipStream_t st = as_stream(stream);
  opt_for_each_frame(&l, [&](const OptFrame& f, const int64_t* idx, int64_t) {
    AverageArgs k;
    k.f = f;
    for (int i = 0; i < f.n; ++i) {
      k.p[i] = static_cast<const float*>(a->params[idx[i]]);
      k.s[i] = static_cast<float*>(a->shadow[idx[i]]);
    }
    k.avg = a->avg;
    hipLaunchKernelGGL(multi_average_kernel, dim3((unsigned)f.chunk_start[f.n]), dim3(256), 0, st, k);
  });
  return avg_note_list(check_launch(who), who, "shadow", &l, a->shadow, st);
}

int anemoi_multi_swap(const anemoi_multi_swap_args* a, anemoi_stream_t stream) {
  const char* who = "anemoi_multi_swap";
  AVG_REQUIRE_BLOCK(a, anemoi_multi_swap_args);
  const anemoi_multi_tensor_args l = avg_as_list(a->n_tensors, a->numel);
  void* const* arrays[2] = {a->a, a->b};
  const char* names[2] = {"a", "b"};
  if (int rc = opt_check_list(who, &l, 2, arrays, names)) return rc;
  if (avg_list_is_empty(l)) return ANEMOI_OK;
  hipStream_t st = as_stream(stream);
  opt_for_each_frame(&l, [&](const OptFrame& f, const int64_t* idx, int64_t) {
    SwapArgs k;
    k.f = f;
    for (int i = 0; i < f.n; ++i) {
      k.a[i] = static_cast<float*>(a->a[idx[i]]);
      k.b[i] = static_cast<float*>(a->b[idx[i]]);
    }
    hipLaunchKernelGGL(multi_swap_kernel, dim3((unsigned)f.chunk_start[f.n]), dim3(256), 0, st, k);
  });
  const int rc = avg_note_list(check_launch(who), who, "a", &l, a->a, st);
  return avg_note_list(rc, who, "b", &l, a->b, st);
}

int anemoi_lr_schedule(const anemoi_lr_schedule_args* s, anemoi_stream_t stream) {
  const char* who = "anemoi_lr_schedule";
  AVG_REQUIRE_BLOCK(s, anemoi_lr_schedule_args);
  ANEMOI_REQUIRE(s->n_groups >= 0, ANEMOI_ERR_INVALID, "%s: negative n_groups %lld", who, (long long)s->n_groups);
  ANEMOI_REQUIRE(s->n_groups <= OPT_MAX_GROUPS, ANEMOI_ERR_INVALID, "%s: n_groups = %lld, at most %d per call", who,
                 (long long)s->n_groups, OPT_MAX_GROUPS);
  if (s->n_groups == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(s->step && s->lr && s->base && s->lr_min && s->warmup_start && s->warmup_steps && s->total_steps &&
                     s->warmup_prefix,
                 ANEMOI_ERR_INVALID,
                 "%s: null pointer (step / lr / base / lr_min / warmup_start / warmup_steps / total_steps / warmup_prefix)", who);
  LrScheduleArgs k = {};
  k.n_groups = (int32_t)s->n_groups;
  for (int64_t g = 0; g < s->n_groups; ++g) {
    ANEMOI_REQUIRE(s->step[g] != nullptr, ANEMOI_ERR_INVALID, "%s: null pointer (step[%lld])", who, (long long)g);
    ANEMOI_REQUIRE(s->lr[g] != nullptr, ANEMOI_ERR_INVALID, "%s: null pointer (lr[%lld])", who, (long long)g);
    ANEMOI_REQUIRE(s->base[g] >= 0.0, ANEMOI_ERR_INVALID, "%s: base[%lld] = %g < 0", who, (long long)g, s->base[g]);
    ANEMOI_REQUIRE(s->lr_min[g] >= 0.0, ANEMOI_ERR_INVALID, "%s: lr_min[%lld] = %g < 0", who, (long long)g, s->lr_min[g]);
    ANEMOI_REQUIRE(s->warmup_start[g] >= 0.0, ANEMOI_ERR_INVALID, "%s: warmup_start[%lld] = %g < 0", who, (long long)g,
                   s->warmup_start[g]);
    ANEMOI_REQUIRE(s->warmup_steps[g] >= 0, ANEMOI_ERR_INVALID, "%s: warmup_steps[%lld] = %lld < 0", who, (long long)g,
                   (long long)s->warmup_steps[g]);
    ANEMOI_REQUIRE(s->total_steps[g] >= 1, ANEMOI_ERR_INVALID, "%s: total_steps[%lld] = %lld < 1", who, (long long)g,
                   (long long)s->total_steps[g]);
    k.step[g] = static_cast<const float*>(s->step[g]);
    k.lr[g] = static_cast<float*>(s->lr[g]);
    k.base[g] = s->base[g];
    k.lr_min[g] = s->lr_min[g];
    k.warmup_start[g] = s->warmup_start[g];
    k.warmup_steps[g] = s->warmup_steps[g];
    k.total_steps[g] = s->total_steps[g];
    k.warmup_prefix[g] = s->warmup_prefix[g] != 0;
  }
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(lr_schedule_kernel, dim3(1), dim3(64), 0, st, k);
  int rc = check_launch(who);
  if (rc != ANEMOI_OK || trail::armed_state() == nullptr) return rc;
  char tag[24];
  for (int64_t g = 0; g < s->n_groups && rc == ANEMOI_OK; ++g) {  // the groups' learning rates are separate allocations
    snprintf(tag, sizeof(tag), "lr[%lld]", (long long)g);
    rc = trail::note(rc, who, tag, ANEMOI_F32, s->lr[g], 1, 1, 1, st);
  }
  return rc;
}

}  // extern "C"
