// The optimizer step ("8f-10"): global gradient norm, clip, decoupled weight decay, Adam moments, update and
// step count on one multi-tensor frame.  All operands f32; parameters, gradients and both moments are separate allocations of
// any length.
//
// The frame (csrc/multi_tensor.hpp, shared with csrc/average.hip): up to OPT_MAX_TENSORS tensors per launch, pointers by value in
// the argument block, chunks of OPT_CHUNK elements, pass u of thread t owning the four elements (u * 256 + t) * 4 .. + 3.
//
// anemoi_multi_sumsq, the determinism rule: the result is a function of the gradient VALUES and the ordered list of lengths
// alone -- not of addresses, alignment or what else ran.  Stage 1: a thread adds the squares of its elements in ascending index
// order (one fmaf each: the square is not rounded), the 64 lanes of a wave are summed by the fixed butterfly, the four waves in
// order; partial q of the list (q counts (tensor, chunk) pairs in list order) goes to workspace[q].  Stage 2: one workgroup of
// 1024 threads; thread t adds partials t, t + 1024, ... in ascending order in f64, the threads are summed in f64 by the fixed
// butterfly and in wave order, and the f32-rounded total is written.  No atomics.  The longest chain of f32 additions a term
// passes through is OPT_CHUNK / 256 + 6 + 3 (_lib.OPT_SUMSQ_DEPTH), whatever the chunk count (stage 2 adds in f64).
//
// anemoi_adamw_constants: one tiny kernel turns sumsq, the step counters and the learning rates into the f32 scalars of the
// step (OPT_CONSTS floats per block: block 0 for the list, block 1 + g for group g), which the update kernel reads through
// scalar loads.  Nothing is read back to the host.
//
// anemoi_multi_adamw, per element, g' = clip * g, every operation a correctly rounded f32 operation and none contracted beyond
// the fmaf written here (roundings on each output's path in brackets; tests/_optim_ref.py holds the bounds):
//   m  <- fmaf(g' - m, 1 - beta1, m)                              [3]
//   v  <- fmaf((1 - beta2) * g', g', beta2 * v)                   [5: g' enters twice]
//   p  <- fmaf(-(lr / bc1), m / (sqrtf(v) / sqrt(bc2) + eps), p * (1 - lr * wd))      [6, from the stored m and v]
// .grad is only read.  Under the skip flag the kernel returns before its first load.
#include "multi_tensor.hpp"

#pragma clang fp contract(off)

namespace anemoi {

constexpr int OPT_CONSTS = 8;       // floats per constants block
// constants block 0 (the list): norm, clip, finite, skip.  Block 1 + g (group g): clip, decay, step_size, sqrt(bc2), skip, lr, t.
constexpr int OPTC_NORM = 0, OPTC_CLIP_ALL = 1, OPTC_FINITE = 2, OPTC_SKIP_ALL = 3;
constexpr int OPTC_CLIP = 0, OPTC_DECAY = 1, OPTC_STEP_SIZE = 2, OPTC_BC2_SQRT = 3, OPTC_SKIP = 4, OPTC_LR = 5, OPTC_T = 6;

struct SumsqArgs {
  OptFrame f;
  const float* g[OPT_MAX_TENSORS];
};

struct ScaleArgs {
  OptFrame f;
  float* g[OPT_MAX_TENSORS];
};

struct AdamwArgs {
  OptFrame f;
  float* p[OPT_MAX_TENSORS];
  const float* g[OPT_MAX_TENSORS];
  float* m[OPT_MAX_TENSORS];
  float* v[OPT_MAX_TENSORS];
  const float* consts;  // this group's block
  float w1, beta2, w2, eps;
};
static_assert(sizeof(AdamwArgs) <= 4096, "the argument block of one launch is limited to 4 KB");

struct ConstantsArgs {
  int32_t n_groups, group0, has_max_norm, skip_nonfinite;
  float max_norm;
  const float* sumsq;  // or null: no norm was taken
  long long* skipped;  // or null
  float* consts;
  float* step[OPT_MAX_GROUPS];
  const float* lr_dev[OPT_MAX_GROUPS];  // or null: lr[g]
  double lr[OPT_MAX_GROUPS], beta1[OPT_MAX_GROUPS], beta2[OPT_MAX_GROUPS], weight_decay[OPT_MAX_GROUPS];
};
static_assert(sizeof(ConstantsArgs) <= 4096, "the argument block of one launch is limited to 4 KB");

template <bool FULL>
__device__ __forceinline__ float opt_sumsq_chunk(const float* __restrict__ g, int cnt, bool vec) {
  float x[OPT_PASSES][4];
#pragma unroll
  for (int u = 0; u < OPT_PASSES; ++u) opt_load4<FULL>(g, (u * 256 + (int)threadIdx.x) * 4, cnt, vec, x[u]);
  float acc = 0.f;
#pragma unroll
  for (int u = 0; u < OPT_PASSES; ++u)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc = fmaf(x[u][k], x[u][k], acc);
  return acc;
}

struct AdamwScalars {
  float clip, decay, step_size, bc2s, w1, beta2, w2, eps;
};

template <bool FULL>
__device__ __forceinline__ void opt_adamw_chunk(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                float* __restrict__ v, int cnt, bool vec, const AdamwScalars& c) {
  float xp[OPT_PASSES][4], xg[OPT_PASSES][4], xm[OPT_PASSES][4], xv[OPT_PASSES][4];
#pragma unroll
  for (int u = 0; u < OPT_PASSES; ++u) {
    const int i = (u * 256 + (int)threadIdx.x) * 4;
    opt_load4<FULL>(g, i, cnt, vec, xg[u]);
    opt_load4<FULL>(m, i, cnt, vec, xm[u]);
    opt_load4<FULL>(v, i, cnt, vec, xv[u]);
    opt_load4<FULL>(p, i, cnt, vec, xp[u]);
  }
#pragma unroll
  for (int u = 0; u < OPT_PASSES; ++u) {
    const int i = (u * 256 + (int)threadIdx.x) * 4;
    if (!FULL && i >= cnt) break;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float gc = c.clip * xg[u][k];
      const float mn = fmaf(gc - xm[u][k], c.w1, xm[u][k]);
      const float vn = fmaf(c.w2 * gc, gc, c.beta2 * xv[u][k]);
      const float denom = sqrtf(vn) / c.bc2s + c.eps;
      xp[u][k] = fmaf(-c.step_size, mn / denom, xp[u][k] * c.decay);
      xm[u][k] = mn;
      xv[u][k] = vn;
    }
    opt_store4<FULL>(m, i, cnt, vec, xm[u]);
    opt_store4<FULL>(v, i, cnt, vec, xv[u]);
    opt_store4<FULL>(p, i, cnt, vec, xp[u]);
  }
}

template <bool FULL>
__device__ __forceinline__ void opt_scale_chunk(float* __restrict__ g, int cnt, bool vec, float coef) {
  float x[OPT_PASSES][4];
#pragma unroll
  for (int u = 0; u < OPT_PASSES; ++u) opt_load4<FULL>(g, (u * 256 + (int)threadIdx.x) * 4, cnt, vec, x[u]);
#pragma unroll
  for (int u = 0; u < OPT_PASSES; ++u) {
    const int i = (u * 256 + (int)threadIdx.x) * 4;
    if (!FULL && i >= cnt) break;
#pragma unroll
    for (int k = 0; k < 4; ++k) x[u][k] *= coef;
    opt_store4<FULL>(g, i, cnt, vec, x[u]);
  }
}

__global__ __launch_bounds__(256) void multi_sumsq_kernel(const SumsqArgs a, float* __restrict__ partial) {
  __shared__ float sh4[4];
  const int b = blockIdx.x, ti = opt_find(a.f, b);
  const int64_t e0 = (int64_t)(b - a.f.chunk_start[ti]) * OPT_CHUNK, left = a.f.numel[ti] - e0;
  const int cnt = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
  const float* __restrict__ g = a.g[ti] + e0;
  const bool vec = ((uintptr_t)a.g[ti] & 15) == 0;
  float acc = vec && cnt == OPT_CHUNK ? opt_sumsq_chunk<true>(g, cnt, vec) : opt_sumsq_chunk<false>(g, cnt, vec);
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[b] = ((sh4[0] + sh4[1]) + sh4[2]) + sh4[3];
}

__global__ __launch_bounds__(1024) void multi_sumsq_finish_kernel(const float* __restrict__ partial, int64_t n,
                                                                  float* __restrict__ sumsq) {
  __shared__ double sh[16];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 1024) acc += (double)partial[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = sh[0];
    for (int w = 1; w < 16; ++w) s += sh[w];
    *sumsq = (float)s;
  }
}

// thread g < n_groups: group g of this launch (group0 + g of the optimizer); thread 0 of the launch with group0 == 0 also
// writes block 0 and advances the skip counter
__global__ __launch_bounds__(64) void adamw_constants_kernel(const ConstantsArgs a) {
  float norm = 0.f, clip = 1.f;
  bool finite = true;
  if (a.sumsq != nullptr) {
    norm = sqrtf(*a.sumsq);
    finite = isfinite(norm);
    if (a.has_max_norm) {
      const float c = a.max_norm / (norm + 1e-6f);
      clip = c > 1.f ? 1.f : c;  // (a NaN stays a NaN, as in torch's clamp)
    }
  }
  const bool skip = a.skip_nonfinite && !finite;
  if (threadIdx.x == 0 && a.group0 == 0) {
    float* c = a.consts;
    c[OPTC_NORM] = norm;
    c[OPTC_CLIP_ALL] = clip;
    c[OPTC_FINITE] = finite ? 1.f : 0.f;
    c[OPTC_SKIP_ALL] = skip ? 1.f : 0.f;
    for (int k = 4; k < OPT_CONSTS; ++k) c[k] = 0.f;
    if (skip && a.skipped != nullptr) *a.skipped += 1;
  }
  const int g = threadIdx.x;
  if (g >= a.n_groups) return;
  const double lr = a.lr_dev[g] != nullptr ? (double)*a.lr_dev[g] : a.lr[g];
  const float t = *a.step[g] + (skip ? 0.f : 1.f);
  const double bc1 = 1.0 - pow(a.beta1[g], (double)t), bc2 = 1.0 - pow(a.beta2[g], (double)t);
  float* c = a.consts + (int64_t)(1 + a.group0 + g) * OPT_CONSTS;
  c[OPTC_CLIP] = clip;
  c[OPTC_DECAY] = (float)(1.0 - lr * a.weight_decay[g]);
  c[OPTC_STEP_SIZE] = (float)(lr / bc1);
  c[OPTC_BC2_SQRT] = (float)sqrt(bc2);
  c[OPTC_SKIP] = skip ? 1.f : 0.f;
  c[OPTC_LR] = (float)lr;
  c[OPTC_T] = t;
  c[7] = 0.f;
  *a.step[g] = t;
}

__global__ __launch_bounds__(256) void multi_adamw_kernel(const AdamwArgs a) {
  const float* __restrict__ cs = a.consts;
  if (cs[OPTC_SKIP] != 0.f) return;
  const float clip = cs[OPTC_CLIP], decay = cs[OPTC_DECAY], step_size = cs[OPTC_STEP_SIZE], bc2s = cs[OPTC_BC2_SQRT];
  const int b = blockIdx.x, ti = opt_find(a.f, b);
  const int64_t e0 = (int64_t)(b - a.f.chunk_start[ti]) * OPT_CHUNK, left = a.f.numel[ti] - e0;
  const int cnt = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
  float* __restrict__ p = a.p[ti] + e0;
  const float* __restrict__ g = a.g[ti] + e0;
  float* __restrict__ m = a.m[ti] + e0;
  float* __restrict__ v = a.v[ti] + e0;
  const bool vec = ((((uintptr_t)a.p[ti] | (uintptr_t)a.g[ti] | (uintptr_t)a.m[ti] | (uintptr_t)a.v[ti]) & 15) == 0);
  const AdamwScalars c = {clip, decay, step_size, bc2s, a.w1, a.beta2, a.w2, a.eps};
  if (vec && cnt == OPT_CHUNK) opt_adamw_chunk<true>(p, g, m, v, cnt, vec, c);
  else opt_adamw_chunk<false>(p, g, m, v, cnt, vec, c);
}

__global__ __launch_bounds__(256) void multi_scale_kernel(const ScaleArgs a, const float* __restrict__ coef_dev) {
  const float coef = *coef_dev;
  const int b = blockIdx.x, ti = opt_find(a.f, b);
  const int64_t e0 = (int64_t)(b - a.f.chunk_start[ti]) * OPT_CHUNK, left = a.f.numel[ti] - e0;
  const int cnt = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
  float* __restrict__ g = a.g[ti] + e0;
  const bool vec = ((uintptr_t)a.g[ti] & 15) == 0;
  if (vec && cnt == OPT_CHUNK) opt_scale_chunk<true>(g, cnt, vec, coef);
  else opt_scale_chunk<false>(g, cnt, vec, coef);
}

// While a launch trail is armed: one record per non-empty tensor of the list, "who:what[i]" with i the tensor's index in the list
// as [1, numel].  Unarmed this is one thread-local load.
static int opt_note_list(int rc, const char* who, const char* what, const anemoi_multi_tensor_args* a, void* const* tensors,
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

extern "C" {

int anemoi_multi_tensor_max_tensors(void) { return OPT_MAX_TENSORS; }
int anemoi_multi_tensor_chunk(void) { return OPT_CHUNK; }

int64_t anemoi_multi_sumsq_workspace_floats(const int64_t* numel, int64_t n_tensors) {
  if (numel == nullptr || n_tensors <= 0) return 0;
  int64_t chunks = 0;
  for (int64_t i = 0; i < n_tensors; ++i)
    if (numel[i] > 0) chunks += opt_chunks(numel[i]);
  return chunks;
}

int anemoi_multi_sumsq(const anemoi_multi_tensor_args* a, anemoi_stream_t stream) {
  const char* who = "anemoi_multi_sumsq";
  void* const* arrays[1] = {a ? a->grads : nullptr};
  const char* names[1] = {"grads"};
  if (int rc = opt_check_list(who, a, 1, arrays, names)) return rc;
  ANEMOI_REQUIRE(a->sumsq != nullptr, ANEMOI_ERR_INVALID, "%s: null pointer (sumsq)", who);
  const int64_t need = anemoi_multi_sumsq_workspace_floats(a->numel, a->n_tensors);
  ANEMOI_REQUIRE(need == 0 || (a->workspace != nullptr && a->workspace_floats >= need), ANEMOI_ERR_INVALID,
                 "%s: workspace of %lld floats, %lld needed", who, (long long)a->workspace_floats, (long long)need);
  hipStream_t st = as_stream(stream);
  opt_for_each_frame(a, [&](const OptFrame& f, const int64_t* idx, int64_t chunks_before) {
    SumsqArgs k;
    k.f = f;
    for (int i = 0; i < f.n; ++i) k.g[i] = static_cast<const float*>(a->grads[idx[i]]);
    hipLaunchKernelGGL(multi_sumsq_kernel, dim3((unsigned)f.chunk_start[f.n]), dim3(256), 0, st, k,
                       a->workspace + chunks_before);
  });
  hipLaunchKernelGGL(multi_sumsq_finish_kernel, dim3(1), dim3(1024), 0, st, a->workspace, need, a->sumsq);
  return trail::note(check_launch(who), who, "sumsq", ANEMOI_F32, a->sumsq, 1, 1, 1, st);
}

int anemoi_adamw_constants(const anemoi_adamw_constants_args* c, anemoi_stream_t stream) {
  const char* who = "anemoi_adamw_constants";
  ANEMOI_REQUIRE(c != nullptr, ANEMOI_ERR_INVALID, "%s: null argument block", who);
  ANEMOI_REQUIRE(c->struct_bytes == (int64_t)sizeof(anemoi_adamw_constants_args), ANEMOI_ERR_INVALID,
                 "%s: argument block of %lld bytes, this library expects %lld (header / library out of sync)", who,
                 (long long)c->struct_bytes, (long long)sizeof(anemoi_adamw_constants_args));
  ANEMOI_REQUIRE(c->n_groups >= 0, ANEMOI_ERR_INVALID, "%s: negative n_groups %lld", who, (long long)c->n_groups);
  ANEMOI_REQUIRE(c->consts != nullptr, ANEMOI_ERR_INVALID, "%s: null pointer (consts)", who);
  ANEMOI_REQUIRE(!c->has_max_norm || c->sumsq != nullptr, ANEMOI_ERR_INVALID, "%s: max_norm without sumsq (null pointer)", who);
  ANEMOI_REQUIRE(!c->skip_nonfinite || c->sumsq != nullptr, ANEMOI_ERR_INVALID,
                 "%s: skip_nonfinite without sumsq (null pointer)", who);
  ANEMOI_REQUIRE(!c->has_max_norm || c->max_norm >= 0.f, ANEMOI_ERR_INVALID, "%s: max_norm %g < 0", who, c->max_norm);
  if (c->n_groups > 0) {
    ANEMOI_REQUIRE(c->step && c->lr && c->beta1 && c->beta2 && c->weight_decay, ANEMOI_ERR_INVALID,
                   "%s: null pointer (step / lr / beta1 / beta2 / weight_decay)", who);
    for (int64_t g = 0; g < c->n_groups; ++g) {
      ANEMOI_REQUIRE(c->step[g] != nullptr, ANEMOI_ERR_INVALID, "%s: null pointer (step[%lld])", who, (long long)g);
      ANEMOI_REQUIRE(c->beta1[g] >= 0.0 && c->beta1[g] < 1.0, ANEMOI_ERR_INVALID, "%s: beta1[%lld] = %g is not in [0, 1)", who,
                     (long long)g, c->beta1[g]);
      ANEMOI_REQUIRE(c->beta2[g] >= 0.0 && c->beta2[g] < 1.0, ANEMOI_ERR_INVALID, "%s: beta2[%lld] = %g is not in [0, 1)", who,
                     (long long)g, c->beta2[g]);
      ANEMOI_REQUIRE(c->weight_decay[g] >= 0.0, ANEMOI_ERR_INVALID, "%s: weight_decay[%lld] = %g < 0", who, (long long)g,
                     c->weight_decay[g]);
      const bool lr_on_device = c->lr_dev != nullptr && c->lr_dev[g] != nullptr;
      ANEMOI_REQUIRE(lr_on_device || c->lr[g] >= 0.0, ANEMOI_ERR_INVALID, "%s: lr[%lld] = %g < 0", who, (long long)g, c->lr[g]);
    }
  }
  hipStream_t st = as_stream(stream);
  int64_t g0 = 0;
  do {  // (n_groups == 0: block 0 alone, for the stand-alone clip)
    ConstantsArgs k = {};
    k.n_groups = (int32_t)(c->n_groups - g0 < OPT_MAX_GROUPS ? c->n_groups - g0 : OPT_MAX_GROUPS);
    k.group0 = (int32_t)g0;
    k.has_max_norm = c->has_max_norm != 0;
    k.skip_nonfinite = c->skip_nonfinite != 0;
    k.max_norm = c->max_norm;
    k.sumsq = c->sumsq;
    k.skipped = reinterpret_cast<long long*>(c->skipped);
    k.consts = c->consts;
    for (int g = 0; g < k.n_groups; ++g) {
      k.step[g] = static_cast<float*>(c->step[g0 + g]);
      k.lr_dev[g] = c->lr_dev != nullptr ? static_cast<const float*>(c->lr_dev[g0 + g]) : nullptr;
      k.lr[g] = c->lr[g0 + g];
      k.beta1[g] = c->beta1[g0 + g];
      k.beta2[g] = c->beta2[g0 + g];
      k.weight_decay[g] = c->weight_decay[g0 + g];
    }
    hipLaunchKernelGGL(adamw_constants_kernel, dim3(1), dim3(64), 0, st, k);
    g0 += OPT_MAX_GROUPS;
  } while (g0 < c->n_groups);
  return trail::note(check_launch(who), who, "consts", ANEMOI_F32, c->consts, OPT_CONSTS, 1 + c->n_groups, OPT_CONSTS, st);
}

int anemoi_multi_adamw(const anemoi_multi_tensor_args* a, anemoi_stream_t stream) {
  const char* who = "anemoi_multi_adamw";
  void* const* arrays[4] = {a ? a->params : nullptr, a ? a->grads : nullptr, a ? a->exp_avg : nullptr,
                            a ? a->exp_avg_sq : nullptr};
  const char* names[4] = {"params", "grads", "exp_avg", "exp_avg_sq"};
  if (int rc = opt_check_list(who, a, 4, arrays, names)) return rc;
  ANEMOI_REQUIRE(a->consts != nullptr, ANEMOI_ERR_INVALID, "%s: null pointer (consts)", who);
  ANEMOI_REQUIRE(a->beta1 >= 0.0 && a->beta1 < 1.0, ANEMOI_ERR_INVALID, "%s: beta1 = %g is not in [0, 1)", who, a->beta1);
  ANEMOI_REQUIRE(a->beta2 >= 0.0 && a->beta2 < 1.0, ANEMOI_ERR_INVALID, "%s: beta2 = %g is not in [0, 1)", who, a->beta2);
  ANEMOI_REQUIRE(a->eps >= 0.0, ANEMOI_ERR_INVALID, "%s: eps = %g < 0", who, a->eps);
  if (anemoi_multi_sumsq_workspace_floats(a->numel, a->n_tensors) == 0) return ANEMOI_OK;  // nothing but empty tensors
  hipStream_t st = as_stream(stream);
  const float w1 = (float)(1.0 - a->beta1), w2 = (float)(1.0 - a->beta2);
  opt_for_each_frame(a, [&](const OptFrame& f, const int64_t* idx, int64_t) {
    AdamwArgs k;
    k.f = f;
    for (int i = 0; i < f.n; ++i) {
      k.p[i] = static_cast<float*>(a->params[idx[i]]);
      k.g[i] = static_cast<const float*>(a->grads[idx[i]]);
      k.m[i] = static_cast<float*>(a->exp_avg[idx[i]]);
      k.v[i] = static_cast<float*>(a->exp_avg_sq[idx[i]]);
    }
    k.consts = a->consts;
    k.w1 = w1;
    k.beta2 = (float)a->beta2;
    k.w2 = w2;
    k.eps = (float)a->eps;
    hipLaunchKernelGGL(multi_adamw_kernel, dim3((unsigned)f.chunk_start[f.n]), dim3(256), 0, st, k);
  });
  int rc = opt_note_list(check_launch(who), who, "params", a, a->params, st);
  rc = opt_note_list(rc, who, "exp_avg", a, a->exp_avg, st);
  return opt_note_list(rc, who, "exp_avg_sq", a, a->exp_avg_sq, st);
}

int anemoi_multi_scale(const anemoi_multi_tensor_args* a, anemoi_stream_t stream) {
  const char* who = "anemoi_multi_scale";
  void* const* arrays[1] = {a ? a->grads : nullptr};
  const char* names[1] = {"grads"};
  if (int rc = opt_check_list(who, a, 1, arrays, names)) return rc;
  ANEMOI_REQUIRE(a->coef != nullptr, ANEMOI_ERR_INVALID, "%s: null pointer (coef)", who);
  if (anemoi_multi_sumsq_workspace_floats(a->numel, a->n_tensors) == 0) return ANEMOI_OK;  // nothing but empty tensors
  hipStream_t st = as_stream(stream);
  opt_for_each_frame(a, [&](const OptFrame& f, const int64_t* idx, int64_t) {
    ScaleArgs k;
    k.f = f;
    for (int i = 0; i < f.n; ++i) k.g[i] = static_cast<float*>(a->grads[idx[i]]);
    hipLaunchKernelGGL(multi_scale_kernel, dim3((unsigned)f.chunk_start[f.n]), dim3(256), 0, st, k, a->coef);
  });
  return opt_note_list(check_launch(who), who, "grads", a, a->grads, st);
}

}  // extern "C"
