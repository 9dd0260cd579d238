// Ensemble scores ("8f-7"): one reduction over E members and one target per point,
//
//   out[l, v] = scale * sum_{b, g} keep(g, v) ? row_w[g] * col_w[v] * S(c[v] x_1 .. c[v] x_E, c[v] y) : 0
//
// with S the almost-fair kernel CRPS, the squared error of the ensemble mean or the ensemble variance, and the element-wise
// backward of the CRPS with a per-variable upstream gradient.  pred is [n_groups * B * E * G, V] (member e of point (l, b, g) is
// row ((l B + b) E + e) G + g), target [n_groups * B * G, V].
//
// It is a column reduction of csrc/column_reduce.hpp (geometry, layout, sum order and determinism contract there) over points:
// one pass of the workgroup over L points reads, member by member, the contiguous floats point0 * V + t of that member's plane.
// E is a template argument: the E members of a point are loaded once, held in registers, and all E (E - 1) / 2 pair terms are
// formed there.  S is evaluated on e_j = c (x_j - y) (the same value: S takes differences only), so an additive offset common to
// members and target -- a normaliser's -- never meets the rounding.  Sums over members ascend in j; a pair sum is sum_j (sum_{k >
// j} term(j, k)), both ascending.  A thread adds the terms of its column in ascending point order (for E <= 4 with 4 or 2
// independent points of loads in flight).
#include "column_reduce.hpp"

namespace anemoi {

constexpr int ENS_AFCRPS = 0, ENS_MEAN_SE = 1, ENS_VARIANCE = 2;  // ANEMOI_ENS_* of include/anemoi_amd.h
constexpr int ENS_MAX_MEMBERS = 16;
constexpr int64_t ENS_MAX_BLOCKS = 2048;  // workgroups per group (the chunking does not depend on E)

// S of one point.  a1, a2 by kind: AFCRPS 2 / (E (E - 1)), eps / (E (E - 1)); MEAN_SE 1 / E, -; VARIANCE 1 / E, 1 / (E - 1).
//
// The CRPS is not evaluated as the difference of its two sums: with one member far from the rest (|e_m| = 100 against 0.7) both
// are ~ |e_m| and S is what is left of them, 4e-6 of rounding against S ~ 0.3.  Per pair, anemoi-training's form of the score is
//   |e_j| + |e_k| - (1 - eps) |e_j - e_k| = 2 min(|e_j|, |e_k|) [e_j e_k > 0] + eps |e_j - e_k|
// (opposite signs: |e_j - e_k| = |e_j| + |e_k|; equal signs: |e_j - e_k| = max - min), and the first term is |med3(e_j, e_k, 0)|
// exactly: one v_med3_f32.  Every term is >= 0, nothing cancels:  S = 2 / (E (E - 1)) P + eps / (E (E - 1)) Q  with
// P = sum_{j < k} |med3(e_j, e_k, 0)|, Q = sum_{j < k} |e_j - e_k|.
template <int KIND, int E>
__device__ __forceinline__ float ens_s(const float (&x)[E], float y, float c, float a1, float a2) {
  float e[E];
#pragma unroll
  for (int j = 0; j < E; ++j) e[j] = c * (x[j] - y);
  if constexpr (KIND == ENS_AFCRPS) {
    float sp = 0.f, sq = 0.f;
#pragma unroll
    for (int j = 0; j + 1 < E; ++j) {
      float tp = 0.f, tq = 0.f;
#pragma unroll
      for (int k = j + 1; k < E; ++k) {
        tp += fabsf(__builtin_amdgcn_fmed3f(e[j], e[k], 0.f));
        tq += fabsf(e[j] - e[k]);
      }
      sp += tp;
      sq += tq;
    }
    return a1 * sp + a2 * sq;
  } else {
    float m = 0.f;
#pragma unroll
    for (int j = 0; j < E; ++j) m += e[j];
    m *= a1;
    if constexpr (KIND == ENS_MEAN_SE) {
      return m * m;
    } else {  // the mean first, then the squares
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < E; ++j) s += (e[j] - m) * (e[j] - m);
      return s * a2;
    }
  }
}

// U consecutive passes of one thread: the U * E member loads and U target loads are issued before the first is used.  (b, g) is
// the thread's (batch, node) within the group; a pass moves it `lanes` points on.
template <int KIND, int E, int U>
__device__ __forceinline__ float ens_passes(const float* __restrict__ pgroup, const float*& q, unsigned& b, unsigned& g,
                                            unsigned step_b, unsigned step_g, int64_t G, int V, unsigned col, int64_t pass,
                                            const float* __restrict__ row_w, const float* __restrict__ mask, float cw, float c,
                                            float a1, float a2) {
  float x[U][E], y[U], w[U];
  bool keep[U];
  const int64_t plane = G * (int64_t)V;  // one member of one batch entry
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const float* p = pgroup + ((int64_t)b * E * G + g) * V + col;
#pragma unroll
    for (int j = 0; j < E; ++j) x[u][j] = p[j * plane];
    y[u] = q[u * pass];
    keep[u] = mask == nullptr || mask[(int64_t)g * V + col] != 0.f;  // a select: a masked NaN / Inf contributes exactly 0
    w[u] = row_w[g] * cw;
    g += step_g;
    b += step_b;
    if (g >= (unsigned)G) {
      g -= (unsigned)G;
      ++b;
    }
  }
  q += U * pass;
  float acc = 0.f;
#pragma unroll
  for (int u = 0; u < U; ++u) acc += keep[u] ? w[u] * ens_s<KIND, E>(x[u], y[u], c, a1, a2) : 0.f;
  return acc;
}

template <int KIND, int E>
__global__ __launch_bounds__(256) void ensemble_score_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                             int64_t points_per_group, int64_t chunk_points, int64_t G, int V,
                                                             const float* __restrict__ row_w,
                                                             const float* __restrict__ col_w,
                                                             const float* __restrict__ mask,
                                                             const float* __restrict__ diff_scale, float a1, float a2,
                                                             float* __restrict__ partial) {
  constexpr int U = E <= 2 ? 4 : (E <= 4 ? 2 : 1);
  __shared__ float sh[256];
  const unsigned t = threadIdx.x;
  const int lanes = V <= 256 ? 256 / V : 1;
  const int64_t r_begin = (int64_t)blockIdx.x * chunk_points;  // points within the group blockIdx.y
  const int64_t r_end = r_begin + chunk_points < points_per_group ? r_begin + chunk_points : points_per_group;
  const float* pgroup = pred + (int64_t)blockIdx.y * points_per_group * E * V;
  const float* tgroup = target + (int64_t)blockIdx.y * points_per_group * V;
  float* out = partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * V;
  const unsigned step_b = (unsigned)((int64_t)lanes / G), step_g = (unsigned)((int64_t)lanes % G);
  for (int tile0 = 0; tile0 < V; tile0 += 256) {
    const unsigned width = V - tile0 < 256 ? (unsigned)(V - tile0) : 256u;  // (= V when V <= 256)
    const unsigned lane = t / width, col = tile0 + (t - lane * width);
    const bool active = lane < (unsigned)lanes;
    float acc = 0.f;
    if (active && r_begin + lane < r_end) {
      const float cw = col_w != nullptr ? col_w[col] : 1.0f;
      const float c = diff_scale != nullptr ? diff_scale[col] : 1.0f;
      int64_t r = r_begin + lane;
      unsigned b = (unsigned)(r / G), g = (unsigned)(r % G);  // points_per_group = B * G: B, G < 2^31
      const int64_t pass = (int64_t)lanes * V;
      const float* q = tgroup + r * V + col;
      if constexpr (U > 1) {
        for (; r + (int64_t)(U - 1) * lanes < r_end; r += (int64_t)U * lanes)
          acc += ens_passes<KIND, E, U>(pgroup, q, b, g, step_b, step_g, G, V, col, pass, row_w, mask, cw, c, a1, a2);
      }
      for (; r < r_end; r += lanes)
        acc += ens_passes<KIND, E, 1>(pgroup, q, b, g, step_b, step_g, G, V, col, pass, row_w, mask, cw, c, a1, a2);
    }
    if (lanes > 1) {  // (then V <= 256: one tile, one trip through the barrier)
      sh[t] = acc;
      __syncthreads();
      if (t < (unsigned)V) {
        float s = sh[t];
        for (int k = 1; k < lanes; ++k) s += sh[t + k * V];
        out[t] = s;
      }
    } else if (active) {
      out[col] = acc;
    }
  }
}

// d AFCRPS / d members: one thread per (point, column) reads the E members and the target once and writes the E gradients.
// The signs come from comparing the raw members: equal values give exactly 0 whatever the scale and the flush mode.
template <int E>
__global__ __launch_bounds__(256) void ensemble_crps_backward_kernel(const float* __restrict__ pred,
                                                                     const float* __restrict__ target, int64_t n, int64_t B,
                                                                     int64_t G, int V, const float* __restrict__ row_w,
                                                                     const float* __restrict__ col_w,
                                                                     const float* __restrict__ mask,
                                                                     const float* __restrict__ diff_scale, float a1, float a2,
                                                                     float scale, const float* __restrict__ upstream,
                                                                     float* __restrict__ dpred) {
  const bool fits32 = n < ((int64_t)1 << 31);
  const int64_t plane = G * (int64_t)V;  // < 2^31
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {  // i = ((l B + b) G + g) V + v
    int64_t lb, r64;
    fast_divmod(i, plane, fits32, lb, r64);
    const unsigned r = (unsigned)r64, g = r / (unsigned)V, v = r - g * (unsigned)V;
    const int64_t l = fits32 ? (int64_t)((unsigned)lb / (unsigned)B) : lb / B;
    const float* p = pred + lb * E * plane + r;
    float* d = dpred + lb * E * plane + r;
    float x[E];
#pragma unroll
    for (int j = 0; j < E; ++j) x[j] = p[j * plane];
    const float y = target[i];
    const bool keep = mask == nullptr || mask[r] != 0.f;
    const float cw = col_w != nullptr ? col_w[v] : 1.0f;
    const float c = diff_scale != nullptr ? diff_scale[v] : 1.0f;
    const float coef = (((scale * upstream[l * V + v]) * row_w[g]) * cw) * fabsf(c);
#pragma unroll
    for (int j = 0; j < E; ++j) {
      int cnt = 0;  // sum_k sgn(x_j - x_k)
#pragma unroll
      for (int k = 0; k < E; ++k)
        if (k != j) cnt += (x[j] > x[k] ? 1 : 0) - (x[j] < x[k] ? 1 : 0);
      const float sy = x[j] > y ? 1.f : (x[j] < y ? -1.f : 0.f);
      d[j * plane] = keep ? coef * (a1 * sy - a2 * (float)cnt) : 0.f;
    }
  }
}

static int check_ens(const char* who, int kind, float alpha, const float* pred, const float* target, int64_t rows, int V,
                     int64_t G, int E, int64_t n_groups, const float* row_w) {
  if (int rc = column_reduce::check_operands(who, kind, 3, pred, target, row_w)) return rc;
  ANEMOI_REQUIRE(E >= 2, ANEMOI_ERR_INVALID, "%s: an ensemble score needs at least 2 members, got E = %d", who, E);
  ANEMOI_REQUIRE(E <= ENS_MAX_MEMBERS, ANEMOI_ERR_UNSUPPORTED, "%s: E = %d members, at most %d", who, E, ENS_MAX_MEMBERS);
  ANEMOI_REQUIRE(alpha >= 0.f && alpha <= 1.f, ANEMOI_ERR_INVALID, "%s: alpha must lie in [0, 1], got %g", who, (double)alpha);
  if (int rc = column_reduce::check_shape(who, rows, V, G, n_groups)) return rc;
  ANEMOI_REQUIRE(rows / (n_groups * G) < ((int64_t)1 << 31), ANEMOI_ERR_UNSUPPORTED, "%s: the batch does not fit 31 bits", who);
  return ANEMOI_OK;
}

// (a1, a2) of ens_s -- or, for the gradient of the CRPS, (1 / E, (1 - eps) / (E (E - 1))) --, rounded once from double
static void ens_coefficients(int kind, float alpha, int E, bool backward, float& a1, float& a2) {
  const double eps = (1.0 - (double)alpha) / E, pairs = (double)E * (E - 1);
  if (kind == ENS_AFCRPS && !backward) {
    a1 = (float)(2.0 / pairs);
    a2 = (float)(eps / pairs);
  } else if (kind == ENS_AFCRPS) {
    a1 = (float)(1.0 / E);
    a2 = (float)((1.0 - eps) / pairs);
  } else {
    a1 = (float)(1.0 / E);
    a2 = (float)(1.0 / (E - 1));
  }
}

#define ANEMOI_ENS_EACH(X) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)

template <int KIND>
static void launch_ens_score(int E, dim3 grid, hipStream_t st, const float* pred, const float* target, int64_t ppg,
                             int64_t chunk, int64_t G, int V, const float* row_w, const float* col_w, const float* mask,
                             const float* diff_scale, float a1, float a2, float* workspace) {
  switch (E) {
#define ANEMOI_ENS_CASE(N)                                                                                                 \
  case N:                                                                                                                  \
    hipLaunchKernelGGL((ensemble_score_kernel<KIND, N>), grid, dim3(256), 0, st, pred, target, ppg, chunk, G, V, row_w, col_w, \
                       mask, diff_scale, a1, a2, workspace);                                                               \
    break;
    ANEMOI_ENS_EACH(ANEMOI_ENS_CASE)
#undef ANEMOI_ENS_CASE
  }
}

}  // namespace anemoi

using namespace anemoi;

extern "C" {

int64_t anemoi_ensemble_score_workspace_floats(int64_t n_groups, int64_t points_per_group, int V, int E) {
  if (n_groups <= 0 || points_per_group <= 0 || V <= 0 || E < 2 || E > ENS_MAX_MEMBERS) return 0;
  return n_groups * column_reduce::blocks(points_per_group, V, ENS_MAX_BLOCKS) * V;
}

int anemoi_ensemble_score(int kind, float alpha, const float* pred, const float* target, int64_t rows, int V, int64_t G, int E,
                          int64_t n_groups, const float* row_w, const float* col_w, const float* mask,
                          const float* diff_scale, float scale, float* out, float* workspace, int64_t workspace_floats,
                          anemoi_stream_t stream) {
  if (int rc = check_ens("anemoi_ensemble_score", kind, alpha, pred, target, rows, V, G, E, n_groups, row_w)) return rc;
  hipStream_t st = as_stream(stream);
  float a1, a2;
  ens_coefficients(kind, alpha, E, false, a1, a2);
  int64_t blocks;
  int rc = column_reduce::run(
      "anemoi_ensemble_score", rows, V, n_groups, ENS_MAX_BLOCKS, scale, out, workspace, workspace_floats, st, blocks,
      [&](dim3 grid, int64_t ppg, int64_t chunk) {
#define ANEMOI_ENS_SCORE(KIND)                                                                                            \
  launch_ens_score<KIND>(E, grid, st, pred, target, ppg, chunk, G, V, row_w, col_w, mask, diff_scale, a1, a2, workspace)
        if (kind == ENS_AFCRPS) ANEMOI_ENS_SCORE(ENS_AFCRPS);
        else if (kind == ENS_MEAN_SE) ANEMOI_ENS_SCORE(ENS_MEAN_SE);
        else ANEMOI_ENS_SCORE(ENS_VARIANCE);
#undef ANEMOI_ENS_SCORE
      });
  if (blocks == 0) return rc;  // refused, or no rows: nothing was launched
  rc = trail::note(rc, "anemoi_ensemble_score", "partials", ANEMOI_F32, workspace, V, n_groups * blocks, V, st);
  return trail::note(rc, "anemoi_ensemble_score", "out", ANEMOI_F32, out, V, n_groups, V, st);
}

int anemoi_ensemble_score_backward(int kind, float alpha, const float* pred, const float* target, int64_t rows, int V,
                                   int64_t G, int E, int64_t n_groups, const float* row_w, const float* col_w,
                                   const float* mask, const float* diff_scale, float scale, const float* upstream,
                                   float* dpred, anemoi_stream_t stream) {
  if (int rc = check_ens("anemoi_ensemble_score_backward", kind, alpha, pred, target, rows, V, G, E, n_groups, row_w)) return rc;
  ANEMOI_REQUIRE(kind == ENS_AFCRPS, ANEMOI_ERR_UNSUPPORTED,
                 "anemoi_ensemble_score_backward: only ANEMOI_ENS_AFCRPS has a gradient, got kind %d", kind);
  ANEMOI_REQUIRE(upstream && dpred, ANEMOI_ERR_INVALID, "anemoi_ensemble_score_backward: null pointer (upstream / dpred)");
  const int64_t n = rows * (int64_t)V;
  if (n == 0) return ANEMOI_OK;
  hipStream_t st = as_stream(stream);
  float a1, a2;
  ens_coefficients(kind, alpha, E, true, a1, a2);
  int64_t blocks = (n + 255) / 256;
  if (blocks > 256 * 64) blocks = 256 * 64;  // grid-stride the rest
  const int64_t B = rows / (n_groups * G);
  switch (E) {
#define ANEMOI_ENS_CASE(N)                                                                                                  \
  case N:                                                                                                                   \
    hipLaunchKernelGGL(ensemble_crps_backward_kernel<N>, dim3((unsigned)blocks), dim3(256), 0, st, pred, target, n, B, G, V,   \
                       row_w, col_w, mask, diff_scale, a1, a2, scale, upstream, dpred);                                     \
    break;
    ANEMOI_ENS_EACH(ANEMOI_ENS_CASE)
#undef ANEMOI_ENS_CASE
  }
  return trail::note(check_launch("anemoi_ensemble_score_backward"), "anemoi_ensemble_score_backward", "dpred", ANEMOI_F32,
                     dpred, V, rows * E, V, st);
}

}  // extern "C"
