// The loss family ("rollout" and "8f-6").
//
// anemoi_weighted_error: one reduction [rows, V] -> [groups, V] for the node-weighted, variable-scaled, masked MSE / MAE /
// Huber / log-cosh error per variable, and its element-wise backward with a per-variable upstream gradient.
//
//   out[l, v] = scale * sum_{r in group l} keep(g, v) ? row_w[g] * col_w[v] * f(c[v] * (pred[r, v] - target[r, v])) : 0,  g = r % G
//
// It is a column reduction of csrc/column_reduce.hpp (geometry, layout, sum order and determinism contract there) over rows: a
// thread adds the terms of its column in ascending row order, WERR_UNROLL independent passes of loads in flight.
//
// anemoi_weighted_mse: the scalar node-weighted, variable-scaled, masked MSE of a rollout step with its gradient, on a flat-index
// reduction of its own (below) -- as deterministic, another sum order.
#include "column_reduce.hpp"

namespace anemoi {

constexpr int WERR_MSE = 0, WERR_MAE = 1, WERR_HUBER = 2, WERR_LOGCOSH = 3;  // ANEMOI_LOSS_* of include/anemoi_amd.h
constexpr int64_t WERR_MAX_BLOCKS = 1024;  // workgroups per group
constexpr int WERR_UNROLL = 4;

template <int KIND>
__device__ __forceinline__ float werr_f(float e, float delta) {
  if constexpr (KIND == WERR_MSE) {
    return e * e;
  } else if constexpr (KIND == WERR_MAE) {
    return fabsf(e);
  } else if constexpr (KIND == WERR_HUBER) {
    const float a = fabsf(e);
    return a <= delta ? 0.5f * (e * e) : delta * (a - 0.5f * delta);
  } else {
    const float a = fabsf(e);  // log cosh e = |e| + log1p(exp(-2 |e|)) - ln 2: no overflow
    return (a + log1pf(expf(-2.0f * a))) - 0.693147180559945309f;
  }
}

__device__ __forceinline__ float werr_sign(float e) { return e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f); }

template <int KIND>
__device__ __forceinline__ float werr_df(float e, float delta) {
  if constexpr (KIND == WERR_MSE) {
    return 2.0f * e;
  } else if constexpr (KIND == WERR_MAE) {
    return werr_sign(e);  // 0 at e = 0 (torch's convention)
  } else if constexpr (KIND == WERR_HUBER) {
    return fabsf(e) <= delta ? e : delta * werr_sign(e);
  } else {
    return tanhf(e);
  }
}

template <int KIND>
__global__ __launch_bounds__(256) void weighted_error_kernel(const float* __restrict__ pred,
                                                             const float* __restrict__ target, int64_t rows_per_group,
                                                             int64_t chunk_rows, int64_t G, int V,
                                                             const float* __restrict__ row_w,
                                                             const float* __restrict__ col_w,
                                                             const float* __restrict__ mask,
                                                             const float* __restrict__ diff_scale, float delta,
                                                             float* __restrict__ partial) {
  __shared__ float sh[256];
  const unsigned t = threadIdx.x;
  const int lanes = V <= 256 ? 256 / V : 1;
  const int64_t r_begin = (int64_t)blockIdx.x * chunk_rows;  // rows within the group blockIdx.y
  const int64_t r_end = r_begin + chunk_rows < rows_per_group ? r_begin + chunk_rows : rows_per_group;
  const int64_t group_row0 = (int64_t)blockIdx.y * rows_per_group;
  float* out = partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * V;
  const unsigned step = (unsigned)((int64_t)lanes % G);  // a pass moves every thread `lanes` rows on: g += step (mod G)
  for (int tile0 = 0; tile0 < V; tile0 += 256) {
    const unsigned width = V - tile0 < 256 ? (unsigned)(V - tile0) : 256u;  // (= V when V <= 256)
    const unsigned lane = t / width, col = tile0 + (t - lane * width);
    const bool active = lane < (unsigned)lanes;
    float acc = 0.f;
    if (active) {
      const float cw = col_w != nullptr ? col_w[col] : 1.0f;
      const float c = diff_scale != nullptr ? diff_scale[col] : 1.0f;
      int64_t r = r_begin + lane;
      unsigned g = (unsigned)(r % G);  // rows_per_group is a multiple of G: the row within the group decides
      const int64_t pass = (int64_t)lanes * V;
      const float* p = pred + (group_row0 + r) * V + col;
      const float* q = target + (group_row0 + r) * V + col;
      for (; r + (int64_t)(WERR_UNROLL - 1) * lanes < r_end; r += (int64_t)WERR_UNROLL * lanes) {
        float pv[WERR_UNROLL], qv[WERR_UNROLL], w[WERR_UNROLL];
        bool keep[WERR_UNROLL];
#pragma unroll
        for (int k = 0; k < WERR_UNROLL; ++k) {
          pv[k] = p[k * pass];
          qv[k] = q[k * pass];
          keep[k] = mask == nullptr || mask[(int64_t)g * V + col] != 0.f;  // a select: a masked NaN contributes exactly 0
          w[k] = row_w[g] * cw;
          g += step;
          if (g >= (unsigned)G) g -= (unsigned)G;
        }
#pragma unroll
        for (int k = 0; k < WERR_UNROLL; ++k) acc += keep[k] ? w[k] * werr_f<KIND>(c * (pv[k] - qv[k]), delta) : 0.f;
        p += WERR_UNROLL * pass;
        q += WERR_UNROLL * pass;
      }
      for (; r < r_end; r += lanes) {
        const bool keep = mask == nullptr || mask[(int64_t)g * V + col] != 0.f;
        const float w = row_w[g] * cw;
        acc += keep ? w * werr_f<KIND>(c * (*p - *q), delta) : 0.f;
        g += step;
        if (g >= (unsigned)G) g -= (unsigned)G;
        p += pass;
        q += pass;
      }
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

// Stage 2 of every column reduction (column_reduce::launch_finish, used by csrc/ensemble.hip as well).
__global__ __launch_bounds__(256) void column_reduce_finish_kernel(const float* __restrict__ partial, int64_t blocks,
                                                                   int64_t n_out, int V, float scale,
                                                                   float* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (l, v)
  if (idx >= n_out) return;
  const int64_t l = idx / V, v = idx - l * V;
  const float* p = partial + l * blocks * V + v;
  float s = 0.f;
#pragma unroll 8
  for (int64_t k = 0; k < blocks; ++k) s += p[k * V];
  out[idx] = s * scale;
}

void column_reduce::launch_finish(const float* partial, int64_t blocks, int64_t n_out, int V, float scale, float* out,
                                  hipStream_t st) {
  hipLaunchKernelGGL(column_reduce_finish_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, st, partial, blocks,
                     n_out, V, scale, out);
}

// dpred, four consecutive elements per thread (one 16-byte access per operand where the pointers allow), (l, g, v) kept by
// increments as in weighted_mse_kernel.
template <int KIND>
__global__ __launch_bounds__(256) void weighted_error_backward_kernel(const float* __restrict__ pred,
                                                                      const float* __restrict__ target, int64_t n,
                                                                      int64_t rows_per_group, int64_t G, int V,
                                                                      const float* __restrict__ row_w,
                                                                      const float* __restrict__ col_w,
                                                                      const float* __restrict__ mask,
                                                                      const float* __restrict__ diff_scale, float delta,
                                                                      float scale, const float* __restrict__ upstream,
                                                                      float* __restrict__ dpred, int vec_ok) {
  const bool fits32 = n < ((int64_t)1 << 31);
  for (int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; i0 < n; i0 += (int64_t)gridDim.x * 1024) {
    int64_t row, v64;
    fast_divmod(i0, V, fits32, row, v64);
    int64_t l = row / rows_per_group, rg = row - l * rows_per_group;
    unsigned g = (unsigned)(rg % G), v = (unsigned)v64;
    const int cnt = n - i0 < 4 ? (int)(n - i0) : 4;
    float p[4] = {0.f, 0.f, 0.f, 0.f}, t[4] = {0.f, 0.f, 0.f, 0.f}, r[4];
    if (cnt == 4 && vec_ok) {
      VecIO<float, 4>::load(pred + i0, p);
      VecIO<float, 4>::load(target + i0, t);
    } else {
      for (int k = 0; k < cnt; ++k) {
        p[k] = pred[i0 + k];
        t[k] = target[i0 + k];
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      r[k] = 0.f;
      if (k < cnt) {
        const bool keep = mask == nullptr || mask[(int64_t)g * V + v] != 0.f;
        const float cw = col_w != nullptr ? col_w[v] : 1.0f;
        const float c = diff_scale != nullptr ? diff_scale[v] : 1.0f;
        const float coef = (((scale * upstream[l * V + v]) * row_w[g]) * cw) * c;
        r[k] = keep ? coef * werr_df<KIND>(c * (p[k] - t[k]), delta) : 0.f;
        if (++v == (unsigned)V) {
          v = 0;
          if (++g == (unsigned)G) g = 0;
          if (++rg == rows_per_group) {
            rg = 0;
            ++l;
          }
        }
      }
    }
    if (cnt == 4 && vec_ok) {
      VecIO<float, 4>::store(dpred + i0, r);
    } else {
      for (int k = 0; k < cnt; ++k) dpred[i0 + k] = r[k];
    }
  }
}

static int check_werr(const char* who, int kind, float delta, const float* pred, const float* target, int64_t rows, int V,
                      int64_t G, int64_t n_groups, const float* row_w) {
  if (int rc = column_reduce::check_operands(who, kind, 4, pred, target, row_w)) return rc;
  ANEMOI_REQUIRE(kind != WERR_HUBER || delta > 0.f, ANEMOI_ERR_INVALID, "%s: the Huber delta must be positive, got %g", who,
                 (double)delta);
  return column_reduce::check_shape(who, rows, V, G, n_groups);
}

// ---------------------------------------------------------------------------------------------
// Weighted MSE.  Flat element i of pred / target [rows, V]: position i % (G * V) of the [G, V] weight / mask plane.
// One thread walks four consecutive elements (one 16-byte load per operand) and keeps (g, v) by increments.
// Stage 1: workgroup k reduces the contiguous chunk [k * chunk, (k + 1) * chunk) -- chunk and the workgroup count are functions
// of rows * V alone (wmse_blocks / wmse_chunk) -- each thread in ascending index order, the wave by the fixed butterfly of
// wave_sum, the four waves in wave order.  Stage 2: one workgroup sums the partials the same way and applies `scale`.
// ---------------------------------------------------------------------------------------------
constexpr int64_t WMSE_PER_BLOCK = 4096;  // elements per workgroup before the workgroup count saturates
constexpr int64_t WMSE_MAX_BLOCKS = 2048;

static inline int64_t wmse_blocks(int64_t n) {
  int64_t blocks = (n + WMSE_PER_BLOCK - 1) / WMSE_PER_BLOCK;
  if (blocks > WMSE_MAX_BLOCKS) blocks = WMSE_MAX_BLOCKS;
  return blocks < 1 ? 1 : blocks;
}

static inline int64_t wmse_chunk(int64_t n) {  // a multiple of the 1024 elements one workgroup takes per trip
  const int64_t blocks = wmse_blocks(n);
  return ((n + blocks - 1) / blocks + 1023) / 1024 * 1024;
}

__device__ __forceinline__ float block_sum_256(float v, float* sh4) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh4[0] + sh4[1]) + sh4[2]) + sh4[3];
}

// BACKWARD = false: partial[blockIdx.x] = sum of the chunk's terms.  BACKWARD = true: dpred over the same chunks.
template <bool BACKWARD>
__global__ __launch_bounds__(256) void weighted_mse_kernel(const float* __restrict__ pred,
                                                           const float* __restrict__ target, int64_t n, int64_t chunk,
                                                           int64_t G, int V, const float* __restrict__ row_w,
                                                           const float* __restrict__ col_w,
                                                           const float* __restrict__ mask, float scale,
                                                           const float* __restrict__ upstream,
                                                           float* __restrict__ out, int vec_ok) {
  __shared__ float sh4[4];
  const int64_t begin = (int64_t)blockIdx.x * chunk;
  const int64_t end = begin + chunk < n ? begin + chunk : n;
  const int64_t plane = G * (int64_t)V;  // < 2^31 (checked by the entry point)
  const bool fits32 = n < ((int64_t)1 << 31);
  float coef = 0.f;
  if constexpr (BACKWARD) coef = (*upstream * scale) * 2.0f;
  float acc = 0.f;
  for (int64_t i0 = begin + (int64_t)threadIdx.x * 4; i0 < end; i0 += 1024) {
    int64_t rep, m0;
    fast_divmod(i0, plane, fits32, rep, m0);
    unsigned g = (unsigned)m0 / (unsigned)V, v = (unsigned)m0 - g * (unsigned)V;
    const int cnt = end - i0 < 4 ? (int)(end - i0) : 4;
    float p[4] = {0.f, 0.f, 0.f, 0.f}, t[4] = {0.f, 0.f, 0.f, 0.f}, r[4];
    if (cnt == 4 && vec_ok) {
      VecIO<float, 4>::load(pred + i0, p);
      VecIO<float, 4>::load(target + i0, t);
    } else {
      for (int k = 0; k < cnt; ++k) {
        p[k] = pred[i0 + k];
        t[k] = target[i0 + k];
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      r[k] = 0.f;
      if (k < cnt) {
        const bool keep = mask == nullptr || mask[(int64_t)g * V + v] != 0.f;  // a select: a masked NaN contributes exactly 0
        const float w = row_w[g] * col_w[v];
        const float d = p[k] - t[k];
        if constexpr (BACKWARD) {
          r[k] = keep ? (coef * w) * d : 0.f;
        } else {
          acc += keep ? (w * d) * d : 0.f;
        }
        if (++v == (unsigned)V) {
          v = 0;
          if (++g == (unsigned)G) g = 0;
        }
      }
    }
    if constexpr (BACKWARD) {
      if (cnt == 4 && vec_ok) {
        VecIO<float, 4>::store(out + i0, r);
      } else {
        for (int k = 0; k < cnt; ++k) out[i0 + k] = r[k];
      }
    }
  }
  if constexpr (!BACKWARD) {
    const float s = block_sum_256(acc, sh4);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(256) void weighted_mse_finish_kernel(const float* __restrict__ partial, int n_partial,
                                                                  float scale, float* __restrict__ loss) {
  __shared__ float sh4[4];
  float acc = 0.f;
  for (int i = threadIdx.x; i < n_partial; i += 256) acc += partial[i];
  const float s = block_sum_256(acc, sh4);
  if (threadIdx.x == 0) *loss = s * scale;
}

static int check_wmse(const char* who, const float* pred, const float* target, int64_t rows, int V, int64_t G,
                      const float* row_w, const float* col_w) {
  ANEMOI_REQUIRE(pred && target && row_w && col_w, ANEMOI_ERR_INVALID, "%s: null pointer", who);
  ANEMOI_REQUIRE(rows >= 0 && V > 0 && G > 0, ANEMOI_ERR_INVALID, "%s: bad shape rows=%lld V=%d G=%lld", who,
                 (long long)rows, V, (long long)G);
  ANEMOI_REQUIRE(rows % G == 0, ANEMOI_ERR_INVALID, "%s: rows %lld is not a multiple of the grid size G = %lld", who,
                 (long long)rows, (long long)G);
  ANEMOI_REQUIRE(G * (int64_t)V < ((int64_t)1 << 31), ANEMOI_ERR_UNSUPPORTED, "%s: G * V does not fit 31 bits", who);
  return ANEMOI_OK;
}

}  // namespace anemoi

using namespace anemoi;

extern "C" {

int64_t anemoi_weighted_error_workspace_floats(int64_t n_groups, int64_t rows_per_group, int V) {
  if (n_groups <= 0 || rows_per_group <= 0 || V <= 0) return 0;
  return n_groups * column_reduce::blocks(rows_per_group, V, WERR_MAX_BLOCKS) * V;
}

int anemoi_weighted_error(int kind, float delta, const float* pred, const float* target, int64_t rows, int V, int64_t G,
                          int64_t n_groups, const float* row_w, const float* col_w, const float* mask,
                          const float* diff_scale, float scale, float* out, float* workspace, int64_t workspace_floats,
                          anemoi_stream_t stream) {
  if (int rc = check_werr("anemoi_weighted_error", kind, delta, pred, target, rows, V, G, n_groups, row_w)) return rc;
  hipStream_t st = as_stream(stream);
  int64_t blocks;
  int rc = column_reduce::run(
      "anemoi_weighted_error", rows, V, n_groups, WERR_MAX_BLOCKS, scale, out, workspace, workspace_floats, st, blocks,
      [&](dim3 grid, int64_t rows_per_group, int64_t chunk) {
#define ANEMOI_WERR(KIND)                                                                                                  \
  hipLaunchKernelGGL(weighted_error_kernel<KIND>, grid, dim3(256), 0, st, pred, target, rows_per_group, chunk, G, V, row_w,   \
                     col_w, mask, diff_scale, delta, workspace)
        if (kind == WERR_MSE) ANEMOI_WERR(WERR_MSE);
        else if (kind == WERR_MAE) ANEMOI_WERR(WERR_MAE);
        else if (kind == WERR_HUBER) ANEMOI_WERR(WERR_HUBER);
        else ANEMOI_WERR(WERR_LOGCOSH);
#undef ANEMOI_WERR
      });
  if (blocks == 0) return rc;  // refused, or no rows: nothing was launched
  rc = trail::note(rc, "anemoi_weighted_error", "partials", ANEMOI_F32, workspace, V, n_groups * blocks, V, st);
  return trail::note(rc, "anemoi_weighted_error", "out", ANEMOI_F32, out, V, n_groups, V, st);
}

int anemoi_weighted_error_backward(int kind, float delta, const float* pred, const float* target, int64_t rows, int V,
                                   int64_t G, int64_t n_groups, const float* row_w, const float* col_w, const float* mask,
                                   const float* diff_scale, float scale, const float* upstream, float* dpred,
                                   anemoi_stream_t stream) {
  if (int rc = check_werr("anemoi_weighted_error_backward", kind, delta, pred, target, rows, V, G, n_groups, row_w)) return rc;
  ANEMOI_REQUIRE(upstream && dpred, ANEMOI_ERR_INVALID, "anemoi_weighted_error_backward: null pointer (upstream / dpred)");
  const int64_t n = rows * (int64_t)V;
  if (n == 0) return ANEMOI_OK;
  hipStream_t st = as_stream(stream);
  const int vec_ok = ((((uintptr_t)pred | (uintptr_t)target | (uintptr_t)dpred) & 15) == 0);
  int64_t blocks = (n + 1023) / 1024;
  if (blocks > 256 * 16) blocks = 256 * 16;  // grid-stride the rest
#define ANEMOI_WERR(KIND)                                                                                                  \
  hipLaunchKernelGGL(weighted_error_backward_kernel<KIND>, dim3((unsigned)blocks), dim3(256), 0, st, pred, target, n,         \
                     rows / n_groups, G, V, row_w, col_w, mask, diff_scale, delta, scale, upstream, dpred, vec_ok)
  if (kind == WERR_MSE) ANEMOI_WERR(WERR_MSE);
  else if (kind == WERR_MAE) ANEMOI_WERR(WERR_MAE);
  else if (kind == WERR_HUBER) ANEMOI_WERR(WERR_HUBER);
  else ANEMOI_WERR(WERR_LOGCOSH);
#undef ANEMOI_WERR
  return trail::note(check_launch("anemoi_weighted_error_backward"), "anemoi_weighted_error_backward", "dpred", ANEMOI_F32,
                     dpred, V, rows, V, st);
}

int64_t anemoi_weighted_mse_workspace_floats(int64_t rows, int V) {
  if (rows <= 0 || V <= 0) return 0;
  return wmse_blocks(rows * (int64_t)V);
}

int anemoi_weighted_mse(const float* pred, const float* target, int64_t rows, int V, int64_t G, const float* row_w,
                        const float* col_w, const float* mask, float scale, float* loss, float* workspace,
                        int64_t workspace_floats, anemoi_stream_t stream) {
  if (int rc = check_wmse("anemoi_weighted_mse", pred, target, rows, V, G, row_w, col_w)) return rc;
  ANEMOI_REQUIRE(loss != nullptr, ANEMOI_ERR_INVALID, "anemoi_weighted_mse: null pointer (loss)");
  hipStream_t st = as_stream(stream);
  const int64_t n = rows * (int64_t)V;
  if (n == 0) {
    hipError_t e = hipMemsetAsync(loss, 0, sizeof(float), st);
    if (e != hipSuccess) return fail(ANEMOI_ERR_LAUNCH, "anemoi_weighted_mse: %s", hipGetErrorString(e));
    return ANEMOI_OK;
  }
  const int64_t blocks = wmse_blocks(n);
  ANEMOI_REQUIRE(workspace != nullptr && workspace_floats >= blocks, ANEMOI_ERR_INVALID,
                 "anemoi_weighted_mse: workspace of %lld floats, %lld needed", (long long)workspace_floats,
                 (long long)blocks);
  const int vec_ok = aligned16(pred) && aligned16(target);
  hipLaunchKernelGGL(weighted_mse_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, pred, target, n, wmse_chunk(n), G,
                     V, row_w, col_w, mask, scale, (const float*)nullptr, workspace, vec_ok);
  hipLaunchKernelGGL(weighted_mse_finish_kernel, dim3(1), dim3(256), 0, st, workspace, (int)blocks, scale, loss);
  int rc = trail::note(check_launch("anemoi_weighted_mse"), "anemoi_weighted_mse", "partials", ANEMOI_F32, workspace, blocks,
                       1, blocks, st);
  return trail::note(rc, "anemoi_weighted_mse", "loss", ANEMOI_F32, loss, 1, 1, 1, st);
}

int anemoi_weighted_mse_backward(const float* pred, const float* target, int64_t rows, int V, int64_t G,
                                 const float* row_w, const float* col_w, const float* mask, float scale,
                                 const float* upstream, float* dpred, anemoi_stream_t stream) {
  if (int rc = check_wmse("anemoi_weighted_mse_backward", pred, target, rows, V, G, row_w, col_w)) return rc;
  ANEMOI_REQUIRE(upstream && dpred, ANEMOI_ERR_INVALID, "anemoi_weighted_mse_backward: null pointer (upstream / dpred)");
  const int64_t n = rows * (int64_t)V;
  if (n == 0) return ANEMOI_OK;
  hipStream_t st = as_stream(stream);
  const int vec_ok = aligned16(pred) && aligned16(target) && aligned16(dpred);
  hipLaunchKernelGGL(weighted_mse_kernel<true>, dim3((unsigned)wmse_blocks(n)), dim3(256), 0, st, pred, target, n,
                     wmse_chunk(n), G, V, row_w, col_w, mask, scale, upstream, dpred, vec_ok);
  return trail::note(check_launch("anemoi_weighted_mse_backward"), "anemoi_weighted_mse_backward", "dpred", ANEMOI_F32, dpred,
                     V, rows, V, st);
}

}  // extern "C"
