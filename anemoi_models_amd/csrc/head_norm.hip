// qk_norm: the bias-free LayerNorm over the head dimension of queries and keys ("8f-13").
//
//   y[r, (g H + h) D + d] = (x - mean) rstd w[g, d],   mean, rstd over the D elements of head (g, h) of row r
//
// x is a [rows, groups H D] view (leading dimension ldx) of the q|k|v product of a Linear: q | k adjacent is groups = 2 with the
// weights of q_norm and k_norm stacked, a q or k on its own is groups = 1.  The kernel is a stream: one read and one write of
// the addressed columns, in place when y == x (every lane writes exactly the elements it read, after it read them).
//
// A head is owned by an aligned group of LG consecutive lanes (LG a power of two, 1 .. 64); lane l of the group holds the
// elements (i LG + l) VEC + j, i < ITEMS, j < VEC, in registers.  D sizeof(T) a whole number of 16-byte words: VEC = one word and
// ITEMS = 1 -- with x, y, ldx, ldy on 16-byte boundaries one access per lane (consecutive lanes read consecutive words, a wave
// 1 KiB per instruction when D / VEC is a power of two), otherwise (a column offset that is no multiple of 16 bytes) the same
// kernel body with element accesses: the same registers, the same arithmetic, the same bits.  Any other D: VEC = 1, LG = the
// power of two at or above D (64 for D > 64, ITEMS = 2).  Statistics in f32, mean first, the variance from the centred values;
// every sum is one balanced tree (head_sum below).
// No LDS; the flat head index r groups H + g H + h is split with one 32-bit division by groups H and one by H.
//
// Backward.  g = dy w,  xhat = x rstd + (-mean rstd),  dx = rstd (g - mean_d g - xhat mean_d(g xhat)): the same walk.
// dw[g, d] = sum_{r, h} dy xhat without atomics (the rule of csrc/column_reduce.hpp and of the conditional LayerNorm's "cols"
// kernel): one thread per column of the view and a fixed chunk of rows per workgroup (a function of `rows` alone) writes
// workspace[chunk][W]; a second kernel adds the chunks of a column in ascending order into workspace[chunks][W]; a third adds
// the H heads of (g, d) in ascending order.  Never a division by w.
#include <initializer_list>

#include "common.hpp"
#include "trail.hpp"

namespace anemoi {

constexpr int HN_MAX_D = 128;
constexpr int64_t HN_BW_MIN_CHUNK = 64, HN_BW_MAX_CHUNKS = 128;

// rows of one workgroup of the cols kernel: at least HN_BW_MIN_CHUNK, at most HN_BW_MAX_CHUNKS chunks
static inline int64_t hn_chunk_rows(int64_t rows) {
  const int64_t chunk = (rows + HN_BW_MAX_CHUNKS - 1) / HN_BW_MAX_CHUNKS;
  return chunk < HN_BW_MIN_CHUNK ? HN_BW_MIN_CHUNK : chunk;
}

static inline int64_t hn_chunks(int64_t rows) {
  const int64_t chunk = hn_chunk_rows(rows);
  const int64_t n = (rows + chunk - 1) / chunk;
  return n < 1 ? 1 : n;
}

// where head `head` (flat over rows, groups, H) starts in a matrix of leading dimension ld, and its group
struct HeadAt {
  int64_t row;
  int col0, grp;
};

__device__ __forceinline__ HeadAt hn_locate(int64_t head, int GH, int H, int D, bool fits32) {
  int64_t row, hh;
  fast_divmod(head, GH, fits32, row, hh);
  HeadAt at;
  at.row = row;
  at.col0 = (int)hh * D;
  at.grp = (int)((unsigned)hh / (unsigned)H);
  return at;
}

// Every sum over a head is ONE balanced binary tree over its elements in ascending order, zero-padded to a power of two: a
// lane adds its VEC consecutive elements pairwise, group_sum adds the lanes (lane ^ 1, lane ^ 2, then row_half_mirror and
// row_mirror, which pair each lane with one of the other quad / half: every lane of a quad or half already holds that sum and
// addition commutes, so the tree is the xor tree's), the two items of the 128-wide route are two such trees added last.  The
// depth of a sum is log2 of the padded head size.  Products enter the trees rounded (no contraction into the additions: see
// the pragma), so the order of operations is the one written here.
#pragma clang fp contract(off)

template <int N>
__device__ __forceinline__ float tree_sum(const float* a) {
  if constexpr (N == 1) return a[0];
  else return tree_sum<N / 2>(a) + tree_sum<N / 2>(a + N / 2);
}

// VEC consecutive elements of a head: one 16-byte access where the operand is aligned (AL), element accesses otherwise -- the
// registers, and everything computed from them, are the same either way
template <typename T, int VEC, bool AL>
__device__ __forceinline__ void hn_load(const T* p, float (&r)[VEC]) {
  if constexpr (AL && sizeof(T) == 4 && VEC == 8) {  // the f32 weights of a bf16 word: two 16-byte loads
    float4 t = reinterpret_cast<const float4*>(p)[0], u = reinterpret_cast<const float4*>(p)[1];
    r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w;
    r[4] = u.x; r[5] = u.y; r[6] = u.z; r[7] = u.w;
  } else if constexpr (AL) {
    VecIO<T, VEC>::load(p, r);
  } else {
#pragma unroll
    for (int j = 0; j < VEC; ++j) r[j] = Elem<T>::load(p + j);
  }
}

template <typename T, int VEC, bool AL>
__device__ __forceinline__ void hn_store(T* p, const float (&r)[VEC]) {
  if constexpr (AL) {
    VecIO<T, VEC>::store(p, r);
  } else {
#pragma unroll
    for (int j = 0; j < VEC; ++j) Elem<T>::store(p + j, r[j]);
  }
}

template <int VEC, int LG, int ITEMS>
__device__ __forceinline__ float head_sum(const float (&t)[ITEMS][VEC]) {
  float s = group_sum<LG>(tree_sum<VEC>(t[0]));
  if constexpr (ITEMS == 2) s = s + group_sum<LG>(tree_sum<VEC>(t[1]));
  return s;
}

template <typename T, int VEC, int LG, int ITEMS, bool AL>
__global__ __launch_bounds__(256) void head_norm_kernel(const T* x, int64_t ldx, const float* __restrict__ w, T* y, int64_t ldy,
                                                        float2* __restrict__ stats, int64_t heads, int GH, int H, int D,
                                                        float eps, bool fits32) {
  static_assert(ITEMS == 1 || ITEMS == 2, "one or two items per lane");
  const int sub = threadIdx.x & (LG - 1);
  const int64_t head = (int64_t)blockIdx.x * (256 / LG) + (threadIdx.x / LG);
  const bool live = head < heads;  // uniform over the lane group
  const HeadAt at = hn_locate(live ? head : 0, GH, H, D, fits32);
  float v[ITEMS][VEC], sq[ITEMS][VEC];
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const int d = (i * LG + sub) * VEC;  // (VEC divides D on the vector route: d < D covers the whole vector)
    if (live && d < D) {
      hn_load<T, VEC, AL>(x + at.row * ldx + at.col0 + d, v[i]);
    } else {
#pragma unroll
      for (int j = 0; j < VEC; ++j) v[i][j] = 0.f;
    }
  }
  const float inv_d = 1.0f / (float)D;
  const float mean = head_sum<VEC, LG, ITEMS>(v) * inv_d;
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const int d = (i * LG + sub) * VEC;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      v[i][j] = d < D ? v[i][j] - mean : 0.f;
      sq[i][j] = v[i][j] * v[i][j];
    }
  }
  const float rstd = rsqrtf(head_sum<VEC, LG, ITEMS>(sq) * inv_d + eps);
  if (!live) return;
  if (stats != nullptr && sub == 0) stats[head] = make_float2(rstd, -mean * rstd);
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const int d = (i * LG + sub) * VEC;
    if (d < D) {
      float wv[VEC];
      hn_load<float, VEC, AL>(w + at.grp * D + d, wv);
#pragma unroll
      for (int j = 0; j < VEC; ++j) v[i][j] = v[i][j] * rstd * wv[j];
      hn_store<T, VEC, AL>(y + at.row * ldy + at.col0 + d, v[i]);
    }
  }
}

template <typename T, int VEC, int LG, int ITEMS, bool AL>
__global__ __launch_bounds__(256) void head_norm_backward_kernel(const T* dy, int64_t ldd, const T* x, int64_t ldx,
                                                                 const float2* __restrict__ stats, const float* __restrict__ w,
                                                                 T* dx, int64_t ldo, int64_t heads, int GH, int H, int D,
                                                                 bool fits32) {
  const int sub = threadIdx.x & (LG - 1);
  const int64_t head = (int64_t)blockIdx.x * (256 / LG) + (threadIdx.x / LG);
  const bool live = head < heads;
  const HeadAt at = hn_locate(live ? head : 0, GH, H, D, fits32);
  const float2 st = live ? stats[head] : make_float2(0.f, 0.f);
  float g[ITEMS][VEC], xh[ITEMS][VEC], gx[ITEMS][VEC];
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const int d = (i * LG + sub) * VEC;
    if (live && d < D) {
      float wv[VEC];
      hn_load<T, VEC, AL>(dy + at.row * ldd + at.col0 + d, g[i]);
      hn_load<T, VEC, AL>(x + at.row * ldx + at.col0 + d, xh[i]);
      hn_load<float, VEC, AL>(w + at.grp * D + d, wv);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        g[i][j] = g[i][j] * wv[j];
        xh[i][j] = fmaf(xh[i][j], st.x, st.y);
      }
    } else {
#pragma unroll
      for (int j = 0; j < VEC; ++j) g[i][j] = xh[i][j] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) gx[i][j] = g[i][j] * xh[i][j];
  }
  const float inv_d = 1.0f / (float)D;
  const float sg = head_sum<VEC, LG, ITEMS>(g) * inv_d;
  const float sgx = head_sum<VEC, LG, ITEMS>(gx) * inv_d;
  if (!live) return;
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const int d = (i * LG + sub) * VEC;
    if (d < D) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) g[i][j] = st.x * (g[i][j] - sg - xh[i][j] * sgx);
      hn_store<T, VEC, AL>(dx + at.row * ldo + at.col0 + d, g[i]);
    }
  }
}

// partial[chunk][c] = sum over the chunk's rows (ascending) of dy[r, c] xhat[r, c], c a column of the [rows, W] view
template <typename T>
__global__ __launch_bounds__(256) void head_norm_backward_cols_kernel(const T* __restrict__ dy, int64_t ldd,
                                                                      const T* __restrict__ x, int64_t ldx,
                                                                      const float2* __restrict__ stats, int64_t rows, int W,
                                                                      int GH, int D, int64_t chunk_rows,
                                                                      float* __restrict__ partial) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= W) return;
  const int hh = (int)((unsigned)c / (unsigned)D);
  const int64_t r_begin = (int64_t)blockIdx.y * chunk_rows;
  const int64_t r_end = r_begin + chunk_rows < rows ? r_begin + chunk_rows : rows;
  float acc = 0.f;
#pragma unroll 4
  for (int64_t r = r_begin; r < r_end; ++r) {
    const float2 st = stats[r * GH + hh];
    acc = fmaf(Elem<T>::load(dy + r * ldd + c), fmaf(Elem<T>::load(x + r * ldx + c), st.x, st.y), acc);
  }
  partial[(int64_t)blockIdx.y * W + c] = acc;
}

// sums[c] = the chunks of column c in ascending order
__global__ __launch_bounds__(256) void head_norm_backward_chunks_kernel(const float* __restrict__ partial, int64_t chunks, int W,
                                                                        float* __restrict__ sums) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= W) return;
  float s = 0.f;
#pragma unroll 8
  for (int64_t k = 0; k < chunks; ++k) s += partial[k * W + c];
  sums[c] = s;
}

// dw[g, d] = the H heads of group g in ascending order
__global__ __launch_bounds__(256) void head_norm_backward_heads_kernel(const float* __restrict__ sums, int groups, int H, int D,
                                                                       float* __restrict__ dw) {
  const int idx = blockIdx.x * 256 + threadIdx.x;  // (g, d)
  if (idx >= groups * D) return;
  const int g = idx / D, d = idx - g * D;
  float s = 0.f;
  for (int h = 0; h < H; ++h) s += sums[(g * H + h) * D + d];
  dw[idx] = s;
}

static inline int hn_pow2_at_least(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

// 16-byte accesses: every operand's rows, and with D a whole number of 16-byte words the heads' starts, on 16-byte boundaries
template <typename T>
static bool hn_aligned(std::initializer_list<const void*> ptrs, std::initializer_list<int64_t> lds) {
  constexpr int VMAX = 16 / sizeof(T);
  bool ok = true;
  for (const void* p : ptrs) ok = ok && (uintptr_t)p % 16 == 0;
  for (int64_t ld : lds) ok = ok && ld % VMAX == 0;
  return ok;
}

// KERNEL<T, VEC, LG, ITEMS, AL>.  D a whole number of 16-byte words: a lane holds one word (VEC = VMAX), read and written as
// one access (`aligned`) or element by element -- the same kernel body, hence the same bits, either way.  Any other D: one
// element per lane (two at D > 64).
#define HN_WORDS(KERNEL, LGV, ...)                                                             \
  do {                                                                                         \
    if (aligned) hipLaunchKernelGGL((KERNEL<T, VMAX, LGV, 1, true>), grid, block, 0, st, __VA_ARGS__);  \
    else hipLaunchKernelGGL((KERNEL<T, VMAX, LGV, 1, false>), grid, block, 0, st, __VA_ARGS__);         \
  } while (0)
#define HN_DISPATCH(KERNEL, ...)                                                                                          \
  do {                                                                                                                    \
    constexpr int VMAX = 16 / sizeof(T);                                                                                  \
    const bool words = D % VMAX == 0;                                                                                     \
    const int lg = words ? hn_pow2_at_least(D / VMAX) : (D > 64 ? 64 : hn_pow2_at_least(D));                              \
    const dim3 grid((unsigned)((heads + 256 / lg - 1) / (256 / lg))), block(256);                                         \
    if (words) {                                                                                                          \
      switch (lg) {                                                                                                       \
        case 1: HN_WORDS(KERNEL, 1, __VA_ARGS__); break;                                                                  \
        case 2: HN_WORDS(KERNEL, 2, __VA_ARGS__); break;                                                                  \
        case 4: HN_WORDS(KERNEL, 4, __VA_ARGS__); break;                                                                  \
        case 8: HN_WORDS(KERNEL, 8, __VA_ARGS__); break;                                                                  \
        case 16: HN_WORDS(KERNEL, 16, __VA_ARGS__); break;                                                                \
        default: HN_WORDS(KERNEL, 32, __VA_ARGS__); break;                                                                \
      }                                                                                                                   \
    } else if (D > 64) {                                                                                                  \
      hipLaunchKernelGGL((KERNEL<T, 1, 64, 2, false>), grid, block, 0, st, __VA_ARGS__);                                  \
    } else {                                                                                                              \
      switch (lg) {                                                                                                       \
        case 1: hipLaunchKernelGGL((KERNEL<T, 1, 1, 1, false>), grid, block, 0, st, __VA_ARGS__); break;                  \
        case 2: hipLaunchKernelGGL((KERNEL<T, 1, 2, 1, false>), grid, block, 0, st, __VA_ARGS__); break;                  \
        case 4: hipLaunchKernelGGL((KERNEL<T, 1, 4, 1, false>), grid, block, 0, st, __VA_ARGS__); break;                  \
        case 8: hipLaunchKernelGGL((KERNEL<T, 1, 8, 1, false>), grid, block, 0, st, __VA_ARGS__); break;                  \
        case 16: hipLaunchKernelGGL((KERNEL<T, 1, 16, 1, false>), grid, block, 0, st, __VA_ARGS__); break;                \
        case 32: hipLaunchKernelGGL((KERNEL<T, 1, 32, 1, false>), grid, block, 0, st, __VA_ARGS__); break;                \
        default: hipLaunchKernelGGL((KERNEL<T, 1, 64, 1, false>), grid, block, 0, st, __VA_ARGS__); break;                \
      }                                                                                                                   \
    }                                                                                                                     \
  } while (0)

template <typename T>
static int head_norm_launch(const void* x, int64_t ldx, const float* w, void* y, int64_t ldy, float* stats, int64_t rows,
                            int groups, int H, int D, float eps, hipStream_t st) {
  const T* xp = static_cast<const T*>(x);
  T* yp = static_cast<T*>(y);
  float2* sp = reinterpret_cast<float2*>(stats);
  const int GH = groups * H;
  const int64_t heads = rows * GH;
  const bool fits32 = heads < ((int64_t)1 << 31);
  const bool aligned = hn_aligned<T>({x, y, w}, {ldx, ldy});
  HN_DISPATCH(head_norm_kernel, xp, ldx, w, yp, ldy, sp, heads, GH, H, D, eps, fits32);
  return check_launch("anemoi_head_norm");
}

template <typename T>
static int head_norm_backward_launch(const void* dy, int64_t ldd, const void* x, int64_t ldx, const float* stats, const float* w,
                                     void* dx, int64_t ldo, float* dw, int64_t rows, int groups, int H, int D, float* workspace,
                                     hipStream_t st) {
  const T* dp = static_cast<const T*>(dy);
  const T* xp = static_cast<const T*>(x);
  T* op = static_cast<T*>(dx);
  const float2* sp = reinterpret_cast<const float2*>(stats);
  const int GH = groups * H, W = GH * D;
  const int64_t heads = rows * GH;
  const bool fits32 = heads < ((int64_t)1 << 31);
  const bool aligned = hn_aligned<T>({dy, x, dx, w}, {ldd, ldx, ldo});
  HN_DISPATCH(head_norm_backward_kernel, dp, ldd, xp, ldx, sp, w, op, ldo, heads, GH, H, D, fits32);
  const int64_t chunk = hn_chunk_rows(rows), chunks = hn_chunks(rows);
  const dim3 block(256), cols((unsigned)((W + 255) / 256));
  hipLaunchKernelGGL((head_norm_backward_cols_kernel<T>), dim3(cols.x, (unsigned)chunks), block, 0, st, dp, ldd, xp, ldx, sp, rows,
                     W, GH, D, chunk, workspace);
  float* sums = workspace + chunks * W;
  hipLaunchKernelGGL(head_norm_backward_chunks_kernel, cols, block, 0, st, workspace, chunks, W, sums);
  hipLaunchKernelGGL(head_norm_backward_heads_kernel, dim3((unsigned)((groups * D + 255) / 256)), block, 0, st, sums, groups, H, D,
                     dw);
  return check_launch("anemoi_head_norm_backward");
}

#undef HN_DISPATCH
#undef HN_WORDS

// the shape checks of both entry points; `lds` are the leading dimensions of the [rows, groups H D] operands
static int check_head_norm_shape(const char* who, int64_t rows, int groups, int H, int D, std::initializer_list<int64_t> lds) {
  ANEMOI_REQUIRE(D >= 1 && rows >= 0 && groups >= 1 && H >= 1, ANEMOI_ERR_INVALID, "%s: bad shape rows=%lld groups=%d H=%d D=%d",
                 who, (long long)rows, groups, H, D);
  ANEMOI_REQUIRE(D <= HN_MAX_D, ANEMOI_ERR_UNSUPPORTED, "%s: head size D = %d, at most %d", who, D, HN_MAX_D);
  const int64_t width = (int64_t)groups * H * D;
  ANEMOI_REQUIRE(width < ((int64_t)1 << 24), ANEMOI_ERR_UNSUPPORTED, "%s: groups * H * D = %lld columns, fewer than 2^24", who,
                 (long long)width);
  for (int64_t ld : lds)
    ANEMOI_REQUIRE(ld >= width, ANEMOI_ERR_INVALID, "%s: leading dimension %lld < groups * H * D = %lld", who, (long long)ld,
                   (long long)width);
  // one lane group per head, at least 4 lane groups per workgroup: the grid has to fit 31 bits
  ANEMOI_REQUIRE(rows * (int64_t)groups * H < ((int64_t)1 << 32), ANEMOI_ERR_UNSUPPORTED, "%s: rows * groups * H = %lld heads, fewer than 2^32",
                 who, (long long)(rows * (int64_t)groups * H));
  return ANEMOI_OK;
}

}  // namespace anemoi

using namespace anemoi;

extern "C" {

int anemoi_head_norm(int dtype, const void* x, int64_t ldx, const float* w, void* y, int64_t ldy, float* stats, int64_t rows,
                     int groups, int H, int D, float eps, anemoi_stream_t stream) {
  ANEMOI_REQUIRE(x && w && y, ANEMOI_ERR_INVALID, "anemoi_head_norm: null pointer");
  if (int rc = check_head_norm_shape("anemoi_head_norm", rows, groups, H, D, {ldx, ldy})) return rc;
  ANEMOI_REQUIRE((uintptr_t)stats % 8 == 0, ANEMOI_ERR_INVALID, "anemoi_head_norm: stats must be 8-byte aligned");
  ANEMOI_REQUIRE(dtype == ANEMOI_F32 || dtype == ANEMOI_BF16, ANEMOI_ERR_UNSUPPORTED, "anemoi_head_norm: dtype %d", dtype);
  if (rows == 0) return ANEMOI_OK;
  hipStream_t st = as_stream(stream);
  int rc = dtype == ANEMOI_F32 ? head_norm_launch<float>(x, ldx, w, y, ldy, stats, rows, groups, H, D, eps, st)
                               : head_norm_launch<bf16_t>(x, ldx, w, y, ldy, stats, rows, groups, H, D, eps, st);
  rc = trail::note(rc, "anemoi_head_norm", "out", dtype, y, ldy, rows, (int64_t)groups * H * D, st);
  if (stats != nullptr) rc = trail::note(rc, "anemoi_head_norm", "stats", ANEMOI_F32, stats, 2, rows * groups * H, 2, st);
  return rc;
}

int64_t anemoi_head_norm_backward_workspace_floats(int64_t rows, int groups, int H, int D) {
  if (rows <= 0 || groups < 1 || H < 1 || D < 1 || D > HN_MAX_D) return 0;
  return (hn_chunks(rows) + 1) * (int64_t)groups * H * D;
}

int anemoi_head_norm_backward(int dtype, const void* dy, int64_t ldd, const void* x, int64_t ldx, const float* stats,
                              const float* w, void* dx, int64_t ldo, float* dw, int64_t rows, int groups, int H, int D,
                              float* workspace, int64_t workspace_floats, anemoi_stream_t stream) {
  const char* who = "anemoi_head_norm_backward";
  ANEMOI_REQUIRE(dy && x && stats && w, ANEMOI_ERR_INVALID, "anemoi_head_norm_backward: null pointer");
  ANEMOI_REQUIRE(dx && dw, ANEMOI_ERR_INVALID, "anemoi_head_norm_backward: null pointer (gradient outputs)");
  if (int rc = check_head_norm_shape(who, rows, groups, H, D, {ldd, ldx, ldo})) return rc;
  ANEMOI_REQUIRE(rows > 0, ANEMOI_ERR_INVALID, "anemoi_head_norm_backward: no rows");
  ANEMOI_REQUIRE((uintptr_t)stats % 8 == 0, ANEMOI_ERR_INVALID, "anemoi_head_norm_backward: stats must be 8-byte aligned");
  ANEMOI_REQUIRE(dtype == ANEMOI_F32 || dtype == ANEMOI_BF16, ANEMOI_ERR_UNSUPPORTED, "anemoi_head_norm_backward: dtype %d", dtype);
  const int64_t need = anemoi_head_norm_backward_workspace_floats(rows, groups, H, D);
  ANEMOI_REQUIRE(workspace != nullptr && workspace_floats >= need, ANEMOI_ERR_INVALID,
                 "anemoi_head_norm_backward: workspace of %lld floats, %lld needed", (long long)workspace_floats, (long long)need);
  hipStream_t st = as_stream(stream);
  int rc = dtype == ANEMOI_F32
               ? head_norm_backward_launch<float>(dy, ldd, x, ldx, stats, w, dx, ldo, dw, rows, groups, H, D, workspace, st)
               : head_norm_backward_launch<bf16_t>(dy, ldd, x, ldx, stats, w, dx, ldo, dw, rows, groups, H, D, workspace, st);
  rc = trail::note(rc, who, "dx", dtype, dx, ldo, rows, (int64_t)groups * H * D, st);
  return trail::note(rc, who, "dw", ANEMOI_F32, dw, D, groups, D, st);
}

}  // extern "C"
