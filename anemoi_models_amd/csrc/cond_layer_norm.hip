// Conditional LayerNorm and the device noise it is conditioned on ("8f-8").
//
//   y[r, c] = xhat[r, c] (1 + s[r, c]) + t[r, c],   s = cond Ws^T + bs,   t = cond Wb^T + bb,   cond [rows, K] f32, K <= 32
//
// xhat = (x - mean) rstd from the two-pass f32 statistics of layer_norm_kernel (csrc/elementwise.hip): one wave64 per row, the
// same lane -> column map (16-byte vectors when the row is aligned and at most 8 vectors per lane long, lane-strided scalars
// otherwise) and the same order of every sum, so the statistics are the bits of anemoi_row_stats and, with zero weights, y is
// the bits of anemoi_layer_norm with gamma = 1, beta = 0.  s and t never exist in memory.
//
// The 2 K C weights are what the kernel is built around.  A wave that read them once per row would move 8 K bytes of weights
// per element against 2 sizeof(T) bytes of activations, so a wave owns R = 8 consecutive rows (a workgroup 32): it takes the
// statistics of its rows one after the other, then walks the columns once, holds the 2 KP weights of a lane's column in
// registers and applies them to all R rows (re-read from L2, where the statistics pass left them).  Weight traffic per element
// falls to 8 K / R bytes of L2 hits.  The row is therefore not kept in registers between the statistics and the apply pass --
// registers hold weights and the R values of the lane's column instead; the arithmetic per element is that of layer_norm_kernel
// all the same.  cond is wave-uniform: it is read through the scalar cache into SGPRs and enters the FMAs as a scalar operand
// (no VGPR, no LDS anywhere in this file).  K is padded to KP = 4, 8, 16 or 32 by the caller (zero weight columns; leading
// dimensions ldc, ldw): one code path per KP, 16-byte weight loads, wide scalar loads.
//
// Backward, deterministic and without atomics (the rule of anemoi_layer_norm_backward):
//   g = dy (1 + s),  ds = dy xhat,  dx = rstd (g - mean_c g - xhat mean_c(g xhat)),  dcond[r, k] = sum_c ds Ws[c, k] + dy Wb[c, k]
//   dWs[c, k] = sum_r ds cond[r, k],  dbs = sum_r ds,  dWb[c, k] = sum_r dy cond[r, k],  dbb = sum_r dy
// "rows" kernel: the forward's wave-owns-R-rows shape (R = 4 at KP >= 16: R KP accumulators of dcond per lane), two walks over
// the columns (the row sums, then dx).  "cols" kernel: one thread per column and a fixed chunk of rows per workgroup, 2 KP + 2
// accumulators in registers, cond and the statistics of a row as scalar loads (the row is uniform over the workgroup);
// workgroup (tile, chunk) writes its partials to workspace[chunk][2 K + 2][C], a second stage adds the chunks in ascending
// order.  The chunking is a function of `rows` alone (anemoi_cond_layer_norm_backward_workspace_floats).
//
// anemoi_gaussian_noise: counter-based normals.  Philox4x32-10 (Salmon et al., SC'11) with counter (q, q >> 32, 0, 0), q = i / 4,
// and key (seed + device word, 0x6E6F6973) gives four words w0..w3 for the elements 4 q .. 4 q + 3; from a pair (wa, wb):
//   a = wa >> 8, b = wb >> 8,  u1 = (a + 1) / 2^24,  u2 = b / 2^24,  r = sqrt(-2 ln u1),  (z, z') = r (cos 2 pi u2, sin 2 pi u2)
// elements 4 q, 4 q + 1 from (w0, w1), 4 q + 2, 4 q + 3 from (w2, w3).  Nothing depends on the launch geometry or on `rows`.
// logf / sqrtf / sincospif are the accurate ones (tests/_cond_ln_ref.py restates the integers exactly, the normals in f64).
#include "common.hpp"
#include "trail.hpp"

namespace anemoi {

constexpr int CLN_MAX_K = 32;
constexpr int CLN_ROWS = 8;         // rows of one wave in the forward
constexpr int64_t CLN_BW_MIN_CHUNK = 64, CLN_BW_MAX_CHUNKS = 128;

static inline int cln_kp(int K) { return K <= 4 ? 4 : (K <= 8 ? 8 : (K <= 16 ? 16 : 32)); }

// rows of one workgroup of the cols kernel: at least CLN_BW_MIN_CHUNK, a multiple of 8, at most CLN_BW_MAX_CHUNKS chunks
static inline int64_t cln_chunk_rows(int64_t rows) {
  int64_t chunk = (rows + CLN_BW_MAX_CHUNKS - 1) / CLN_BW_MAX_CHUNKS;
  if (chunk < CLN_BW_MIN_CHUNK) chunk = CLN_BW_MIN_CHUNK;
  return (chunk + CLN_ROWS - 1) / CLN_ROWS * CLN_ROWS;
}

static inline int64_t cln_chunks(int64_t rows) {
  const int64_t chunk = cln_chunk_rows(rows);
  const int64_t n = (rows + chunk - 1) / chunk;
  return n < 1 ? 1 : n;
}

// The entry points take cond and the weights with K padded to KP columns (leading dimensions ldc, ldw >= KP, 16-byte aligned
// rows, zeros in the weights' padding): one code path, vector loads of the weights, wide scalar loads of cond.
template <int KP>
__device__ __forceinline__ void cln_load_w(const float* __restrict__ W, int64_t ldw, int c, float (&w)[KP]) {
  const float4* p = reinterpret_cast<const float4*>(W + (int64_t)c * ldw);
#pragma unroll
  for (int k = 0; k < KP / 4; ++k) {
    const float4 t = p[k];
    w[4 * k] = t.x; w[4 * k + 1] = t.y; w[4 * k + 2] = t.z; w[4 * k + 3] = t.w;
  }
}

// cond is wave-uniform (a wave works on whole rows): its KP values are read through the scalar cache into SGPRs (merged into
// wide scalar loads) and enter the FMAs as scalar operands -- no VGPR, no LDS.
template <int KP>
__device__ __forceinline__ void cln_cond_row(const float* __restrict__ cond_row, float (&cv)[KP]) {
#pragma unroll
  for (int k = 0; k < KP; ++k) cv[k] = cond_row[k];
}

// cond[row, :] does not change along the columns, and the compiler, left alone, lifts the loads of all R rows out of the column
// loop: R KP SGPRs, more than there are, spilled to VGPR lanes and read back with one v_readlane per FMA.  A row offset it cannot
// see through, tied to the result of the row before the previous one, keeps the loads (one or two wide scalar loads per row)
// in the loop and at most two rows of cond in flight.
__device__ __forceinline__ int64_t cln_opaque(int64_t row_offset, float after) {
  asm volatile("" : "+s"(row_offset) : "v"(after));
  return row_offset;
}

template <int KP>
__device__ __forceinline__ float cln_dot(const float (&cv)[KP], const float (&w)[KP], float base) {  // k ascending
#pragma unroll
  for (int k = 0; k < KP; ++k) base = fmaf(cv[k], w[k], base);
  return base;
}

template <typename T, int VEC, int KP>
__global__ __launch_bounds__(256) void cond_layer_norm_kernel(const T* __restrict__ x, int64_t ldx,
                                                              const float* __restrict__ cond, int64_t ldc, int K,
                                                              const float* __restrict__ Ws, int64_t ldw,
                                                              const float* __restrict__ bs,
                                                              const float* __restrict__ Wb, const float* __restrict__ bb,
                                                              T* __restrict__ y, int64_t ldy,
                                                              float2* __restrict__ stats, int64_t rows, int C, float eps) {
  constexpr int R = CLN_ROWS;
  constexpr int PV = VEC >= 2 ? 2 : 1;  // columns of a lane per step of the apply pass
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row0 = ((int64_t)blockIdx.x * 4 + wid) * R;
  if (row0 >= rows) return;

  // statistics, row by row: lane r keeps those of row r
  float my_mean = 0.f, my_rstd = 0.f;
  const int items = (C + 64 * VEC - 1) / (64 * VEC);
#pragma unroll 1
  for (int r = 0; r < R; ++r) {
    const int64_t row = row0 + r;
    if (row >= rows) break;
    const T* xr = x + row * ldx;
    float s = 0.f;
#pragma unroll 2
    for (int i = 0; i < items; ++i) {
      const int c = (i * 64 + lane) * VEC;
      if (c < C) {
        float v[VEC];
        VecIO<T, VEC>::load(xr + c, v);
#pragma unroll
        for (int j = 0; j < VEC; ++j) s += v[j];
      }
    }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll 2
    for (int i = 0; i < items; ++i) {
      const int c = (i * 64 + lane) * VEC;
      if (c < C) {
        float v[VEC];
        VecIO<T, VEC>::load(xr + c, v);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const float d = v[j] - mean;
          q += d * d;
        }
      }
    }
    const float rstd = rsqrtf(wave_sum(q) / (float)C + eps);
    if (stats != nullptr && lane == 0) stats[row] = make_float2(rstd, -mean * rstd);  // as row_stats_kernel leaves them
    if (lane == r) {
      my_mean = mean;
      my_rstd = rstd;
    }
  }
  float mean_r[R], rstd_r[R];
  int64_t cond_r[R];  // offset of the row's cond (rows past the end: the last row's, computed and not stored)
#pragma unroll
  for (int r = 0; r < R; ++r) {
    mean_r[r] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_mean), r));
    rstd_r[r] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_rstd), r));
    cond_r[r] = (row0 + r < rows ? row0 + r : rows - 1) * ldc;
  }

  // apply: the weights of a column are loaded once for the R rows
  const int steps = (C + 64 * PV - 1) / (64 * PV);
#pragma unroll 1
  for (int i = 0; i < steps; ++i) {
    const int c = (i * 64 + lane) * PV;
    if (c >= C) continue;
    float v[R][PV];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (row0 + r < rows) {
        VecIO<T, PV>::load(x + (row0 + r) * ldx + c, v[r]);
      } else {
#pragma unroll
        for (int j = 0; j < PV; ++j) v[r][j] = 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < PV; ++j) {
      float ws[KP], wb[KP];
      cln_load_w<KP>(Ws, ldw, c + j, ws);
      cln_load_w<KP>(Wb, ldw, c + j, wb);
      const float s0 = bs[c + j], t0 = bb[c + j];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float cv[KP];
        cln_cond_row<KP>(cond + cln_opaque(cond_r[r], r >= 2 ? v[r - 2][j] : (j > 0 ? v[R - 2 + r][j - 1] : 0.f)), cv);
        const float sc = cln_dot<KP>(cv, ws, s0), sh = cln_dot<KP>(cv, wb, t0);
        v[r][j] = (v[r][j] - mean_r[r]) * rstd_r[r] * (1.0f + sc) + sh;
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (row0 + r < rows) VecIO<T, PV>::store(y + (row0 + r) * ldy + c, v[r]);
  }
}

template <typename T, int PV, int KP>
__global__ __launch_bounds__(256) void cond_layer_norm_backward_rows_kernel(
    const T* __restrict__ dy, int64_t ldd, const T* __restrict__ x, int64_t ldx, const float2* __restrict__ stats,
    const float* __restrict__ cond, int64_t ldc, int K, const float* __restrict__ Ws, int64_t ldw, const float* __restrict__ bs,
    const float* __restrict__ Wb, T* __restrict__ dx, int64_t ldo, float* __restrict__ dcond, int64_t rows, int C) {
  constexpr int R = KP >= 16 ? 4 : 8;
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t row0 = ((int64_t)blockIdx.x * 4 + wid) * R;
  if (row0 >= rows) return;
  float2 st[R];
  int64_t cond_r[R];
  float sg[R], sgx[R], dc[R][KP];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t rc = row0 + r < rows ? row0 + r : rows - 1;
    st[r] = stats[rc];
    cond_r[r] = rc * ldc;
    sg[r] = sgx[r] = 0.f;
#pragma unroll
    for (int k = 0; k < KP; ++k) dc[r][k] = 0.f;
  }
  const int steps = (C + 64 * PV - 1) / (64 * PV);
#pragma unroll 1
  for (int i = 0; i < steps; ++i) {
    const int c = (i * 64 + lane) * PV;
    if (c >= C) continue;
    float xv[R][PV], dv[R][PV];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (row0 + r < rows) {
        VecIO<T, PV>::load(x + (row0 + r) * ldx + c, xv[r]);
        VecIO<T, PV>::load(dy + (row0 + r) * ldd + c, dv[r]);
      } else {  // dy = 0: nothing reaches a sum
#pragma unroll
        for (int j = 0; j < PV; ++j) xv[r][j] = dv[r][j] = 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < PV; ++j) {
      float ws[KP], wb[KP];
      cln_load_w<KP>(Ws, ldw, c + j, ws);
      cln_load_w<KP>(Wb, ldw, c + j, wb);
      const float s0 = bs[c + j];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float cv[KP];
        cln_cond_row<KP>(cond + cln_opaque(cond_r[r], r >= 2 ? sgx[r - 2] : (j > 0 ? sgx[R - 2 + r] : 0.f)), cv);
        const float sc = cln_dot<KP>(cv, ws, s0);
        const float xh = fmaf(xv[r][j], st[r].x, st[r].y);
        const float d = dv[r][j];
        const float g = d * (1.0f + sc), ds = d * xh;
        sg[r] += g;
        sgx[r] = fmaf(g, xh, sgx[r]);
#pragma unroll
        for (int k = 0; k < KP; ++k) dc[r][k] = fmaf(ds, ws[k], fmaf(d, wb[k], dc[r][k]));
      }
    }
  }
  const float inv_c = 1.0f / (float)C;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    sg[r] = wave_sum(sg[r]) * inv_c;
    sgx[r] = wave_sum(sgx[r]) * inv_c;
    float mine = 0.f;  // lane k keeps dcond[row, k]
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      const float t = group_sum<64>(dc[r][k]);
      if (lane == k) mine = t;
    }
    if (lane < K && row0 + r < rows) dcond[(row0 + r) * K + lane] = mine;
  }
#pragma unroll 1
  for (int i = 0; i < steps; ++i) {
    const int c = (i * 64 + lane) * PV;
    if (c >= C) continue;
    float xv[R][PV], dv[R][PV];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (row0 + r < rows) {
        VecIO<T, PV>::load(x + (row0 + r) * ldx + c, xv[r]);
        VecIO<T, PV>::load(dy + (row0 + r) * ldd + c, dv[r]);
      } else {
#pragma unroll
        for (int j = 0; j < PV; ++j) xv[r][j] = dv[r][j] = 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < PV; ++j) {
      float ws[KP];
      cln_load_w<KP>(Ws, ldw, c + j, ws);
      const float s0 = bs[c + j];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float cv[KP];
        cln_cond_row<KP>(cond + cln_opaque(cond_r[r], r >= 2 ? xv[r - 2][j] : (j > 0 ? xv[R - 2 + r][j - 1] : 0.f)), cv);
        const float sc = cln_dot<KP>(cv, ws, s0);
        const float xh = fmaf(xv[r][j], st[r].x, st[r].y);
        const float g = dv[r][j] * (1.0f + sc);
        xv[r][j] = st[r].x * (g - sg[r] - xh * sgx[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (row0 + r < rows) VecIO<T, PV>::store(dx + (row0 + r) * ldo + c, xv[r]);
  }
}

template <typename T, int KP>
__global__ __launch_bounds__(256) void cond_layer_norm_backward_cols_kernel(
    const T* __restrict__ dy, int64_t ldd, const T* __restrict__ x, int64_t ldx, const float2* __restrict__ stats,
    const float* __restrict__ cond, int64_t ldc, int K, int64_t rows, int C, int64_t chunk_rows,
    float* __restrict__ partial) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const int64_t r_begin = (int64_t)blockIdx.y * chunk_rows;
  const int64_t r_end = r_begin + chunk_rows < rows ? r_begin + chunk_rows : rows;
  float as[KP], ab[KP], sbs = 0.f, sbb = 0.f;
#pragma unroll
  for (int k = 0; k < KP; ++k) as[k] = ab[k] = 0.f;
#pragma unroll 4
  for (int64_t r = r_begin; r < r_end; ++r) {  // r, and with it cond[r, :] and stats[r], are uniform over the workgroup
    const float2 st = stats[r];
    float cv[KP];
    cln_cond_row<KP>(cond + r * ldc, cv);
    const float d = Elem<T>::load(dy + r * ldd + c);
    const float ds = d * fmaf(Elem<T>::load(x + r * ldx + c), st.x, st.y);
    sbs += ds;
    sbb += d;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
      as[k] = fmaf(ds, cv[k], as[k]);
      ab[k] = fmaf(d, cv[k], ab[k]);
    }
  }
  // [2 K + 2][C]: dWs columns, dbs, dWb columns, dbb
  float* out = partial + (int64_t)blockIdx.y * (2 * K + 2) * C + c;
#pragma unroll
  for (int k = 0; k < KP; ++k)
    if (k < K) {
      out[(int64_t)k * C] = as[k];
      out[(int64_t)(K + 1 + k) * C] = ab[k];
    }
  out[(int64_t)K * C] = sbs;
  out[(int64_t)(2 * K + 1) * C] = sbb;
}

__global__ __launch_bounds__(256) void cond_layer_norm_backward_finish_kernel(const float* __restrict__ partial, int64_t chunks,
                                                                              int K, int C, float* __restrict__ dWs,
                                                                              float* __restrict__ dbs, float* __restrict__ dWb,
                                                                              float* __restrict__ dbb) {
  const int64_t n = (int64_t)(2 * K + 2) * C;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (q, c)
  if (idx >= n) return;
  float s = 0.f;
#pragma unroll 8
  for (int64_t k = 0; k < chunks; ++k) s += partial[k * n + idx];
  const int q = (int)(idx / C), c = (int)(idx - (int64_t)q * C);
  if (q < K) dWs[(int64_t)c * K + q] = s;
  else if (q == K) dbs[c] = s;
  else if (q <= 2 * K) dWb[(int64_t)c * K + (q - K - 1)] = s;
  else dbb[c] = s;
}

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&w)[4]) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

constexpr uint32_t NOISE_KEY1 = 0x6E6F6973u;

__global__ __launch_bounds__(256) void gaussian_noise_kernel(float* __restrict__ out, int64_t n, float std, uint32_t seed,
                                                             const uint32_t* __restrict__ seed_dev) {
  if (seed_dev != nullptr) seed += __builtin_nontemporal_load(seed_dev);  // as edge_dropout_seed
  const int64_t quads = (n + 3) / 4;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += (int64_t)gridDim.x * 256) {
    uint32_t w[4];
    philox4x32_10((uint32_t)q, (uint32_t)((uint64_t)q >> 32), 0u, 0u, seed, NOISE_KEY1, w);
    float z[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float u1 = (float)((w[2 * h] >> 8) + 1u) * 0x1p-24f;  // (0, 1], exact
      const float t2 = (float)(w[2 * h + 1] >> 8) * 0x1p-23f;     // 2 u2 in [0, 2), exact
      const float r = sqrtf(-2.0f * logf(u1));
      float sn, cs;
      sincospif(t2, &sn, &cs);
      z[2 * h] = std * (r * cs);
      z[2 * h + 1] = std * (r * sn);
    }
    const int64_t i0 = q * 4;
    if (i0 + 3 < n && (uintptr_t)out % 16 == 0) {
      *reinterpret_cast<float4*>(out + i0) = make_float4(z[0], z[1], z[2], z[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (i0 + e < n) out[i0 + e] = z[e];
    }
  }
}

template <typename T>
static int cond_layer_norm_launch(const void* x, int64_t ldx, const float* cond, int64_t ldc, int K, const float* Ws,
                                  int64_t ldw, const float* bs,
                                  const float* Wb, const float* bb, void* y, int64_t ldy, float* stats, int64_t rows, int C,
                                  float eps, hipStream_t st) {
  constexpr int VMAX = 16 / sizeof(T);
  const T* xp = static_cast<const T*>(x);
  T* yp = static_cast<T*>(y);
  float2* sp = reinterpret_cast<float2*>(stats);
  // the route of anemoi_layer_norm: vectors for aligned rows of at most 8 vectors per lane, lane-strided scalars otherwise
  const bool aligned = (C % VMAX == 0) && (ldx % VMAX == 0) && (ldy % VMAX == 0) && ((uintptr_t)x % 16 == 0) &&
                       ((uintptr_t)y % 16 == 0);
  const bool vec = aligned && (C + 64 * VMAX - 1) / (64 * VMAX) <= 8;
  const dim3 grid((unsigned)((rows + 4 * CLN_ROWS - 1) / (4 * CLN_ROWS))), block(256);
#define CLN_LAUNCH(V, KPV)                                                                                                 \
  hipLaunchKernelGGL((cond_layer_norm_kernel<T, V, KPV>), grid, block, 0, st, xp, ldx, cond, ldc, K, Ws, ldw, bs, Wb, bb, yp, ldy, \
                     sp, rows, C, eps)
#define CLN_CASE(KPV)                  \
  case KPV:                            \
    if (vec) CLN_LAUNCH(VMAX, KPV);    \
    else CLN_LAUNCH(1, KPV);           \
    break;
  switch (cln_kp(K)) { CLN_CASE(4) CLN_CASE(8) CLN_CASE(16) CLN_CASE(32) }
#undef CLN_CASE
#undef CLN_LAUNCH
  return check_launch("anemoi_cond_layer_norm");
}

template <typename T>
static int cond_layer_norm_backward_launch(const void* dy, int64_t ldd, const void* x, int64_t ldx, const float* stats,
                                           const float* cond, int64_t ldc, int K, const float* Ws, int64_t ldw, const float* bs,
                                           const float* Wb, void* dx, int64_t ldo, float* dcond, float* dWs, float* dbs,
                                           float* dWb, float* dbb, int64_t rows, int C, float* workspace, hipStream_t st) {
  const T* dp = static_cast<const T*>(dy);
  const T* xp = static_cast<const T*>(x);
  T* op = static_cast<T*>(dx);
  const float2* sp = reinterpret_cast<const float2*>(stats);
  constexpr uintptr_t PB = 2 * sizeof(T);  // a lane's pair of columns
  const bool pair = C % 2 == 0 && ldd % 2 == 0 && ldx % 2 == 0 && ldo % 2 == 0 && (uintptr_t)dy % PB == 0 &&
                    (uintptr_t)x % PB == 0 && (uintptr_t)dx % PB == 0;
  const int KP = cln_kp(K);
  const int R = KP >= 16 ? 4 : 8;
  const dim3 rgrid((unsigned)((rows + 4 * R - 1) / (4 * R))), block(256);
  const int64_t chunk = cln_chunk_rows(rows), chunks = cln_chunks(rows);
  const dim3 cgrid((unsigned)((C + 255) / 256), (unsigned)chunks);
#define CLN_ROWS_LAUNCH(V, KPV)                                                                                              \
  hipLaunchKernelGGL((cond_layer_norm_backward_rows_kernel<T, V, KPV>), rgrid, block, 0, st, dp, ldd, xp, ldx, sp, cond, ldc, \
                     K, Ws, ldw, bs, Wb, op, ldo, dcond, rows, C)
#define CLN_CASE(KPV)                                                                                                        \
  case KPV:                                                                                                                  \
    if (pair) CLN_ROWS_LAUNCH(2, KPV);                                                                                       \
    else CLN_ROWS_LAUNCH(1, KPV);                                                                                            \
    hipLaunchKernelGGL((cond_layer_norm_backward_cols_kernel<T, KPV>), cgrid, block, 0, st, dp, ldd, xp, ldx, sp, cond, ldc, \
                       K, rows, C, chunk, workspace);                                                                        \
    break;
  switch (KP) { CLN_CASE(4) CLN_CASE(8) CLN_CASE(16) CLN_CASE(32) }
#undef CLN_CASE
#undef CLN_ROWS_LAUNCH
  const int64_t n = (int64_t)(2 * K + 2) * C;
  hipLaunchKernelGGL(cond_layer_norm_backward_finish_kernel, dim3((unsigned)((n + 255) / 256)), block, 0, st, workspace, chunks,
                     K, C, dWs, dbs, dWb, dbb);
  return check_launch("anemoi_cond_layer_norm_backward");
}

}  // namespace anemoi

using namespace anemoi;

extern "C" {

// cond [rows, ldc] and Ws / Wb [C, ldw] hold K columns padded to KP = 4, 8, 16 or 32
static int check_cln_padding(const char* who, const float* cond, int64_t ldc, int K, const float* Ws, const float* Wb,
                             int64_t ldw) {
  const int KP = cln_kp(K);
  ANEMOI_REQUIRE(ldc >= KP && ldw >= KP && ldc % 4 == 0 && ldw % 4 == 0, ANEMOI_ERR_INVALID,
                 "%s: K = %d is padded to %d columns: ldc = %lld and ldw = %lld must be multiples of 4 of at least that", who, K,
                 KP, (long long)ldc, (long long)ldw);
  ANEMOI_REQUIRE((uintptr_t)cond % 16 == 0 && (uintptr_t)Ws % 16 == 0 && (uintptr_t)Wb % 16 == 0, ANEMOI_ERR_INVALID,
                 "%s: cond, Ws and Wb must be 16-byte aligned", who);
  return ANEMOI_OK;
}

int anemoi_cond_layer_norm(int dtype, const void* x, int64_t ldx, const float* cond, int64_t ldc, int K, const float* Ws,
                           int64_t ldw, const float* bs, const float* Wb, const float* bb, void* y, int64_t ldy, float* stats,
                           int64_t rows, int C, float eps, anemoi_stream_t stream) {
  ANEMOI_REQUIRE(x && cond && Ws && bs && Wb && bb && y, ANEMOI_ERR_INVALID, "anemoi_cond_layer_norm: null pointer");
  ANEMOI_REQUIRE(K >= 1, ANEMOI_ERR_INVALID, "anemoi_cond_layer_norm: the condition needs at least one column, got K = %d", K);
  ANEMOI_REQUIRE(K <= CLN_MAX_K, ANEMOI_ERR_UNSUPPORTED, "anemoi_cond_layer_norm: K = %d condition columns, at most %d", K,
                 CLN_MAX_K);
  ANEMOI_REQUIRE(C > 0 && rows >= 0 && ldx >= C && ldy >= C, ANEMOI_ERR_INVALID,
                 "anemoi_cond_layer_norm: bad shape rows=%lld C=%d ldx=%lld ldy=%lld", (long long)rows, C, (long long)ldx,
                 (long long)ldy);
  ANEMOI_REQUIRE((uintptr_t)stats % 8 == 0, ANEMOI_ERR_INVALID, "anemoi_cond_layer_norm: stats must be 8-byte aligned");
  if (int rc = check_cln_padding("anemoi_cond_layer_norm", cond, ldc, K, Ws, Wb, ldw)) return rc;
  if (rows == 0) return ANEMOI_OK;
  hipStream_t st = as_stream(stream);
  int rc;
  if (dtype == ANEMOI_F32)
    rc = cond_layer_norm_launch<float>(x, ldx, cond, ldc, K, Ws, ldw, bs, Wb, bb, y, ldy, stats, rows, C, eps, st);
  else if (dtype == ANEMOI_BF16)
    rc = cond_layer_norm_launch<bf16_t>(x, ldx, cond, ldc, K, Ws, ldw, bs, Wb, bb, y, ldy, stats, rows, C, eps, st);
  else
    return fail(ANEMOI_ERR_UNSUPPORTED, "anemoi_cond_layer_norm: dtype %d", dtype);
  rc = trail::note(rc, "anemoi_cond_layer_norm", "out", dtype, y, ldy, rows, C, st);
  if (stats != nullptr) rc = trail::note(rc, "anemoi_cond_layer_norm", "stats", ANEMOI_F32, stats, 2, rows, 2, st);
  return rc;
}

int64_t anemoi_cond_layer_norm_backward_workspace_floats(int64_t rows, int C, int K) {
  if (rows <= 0 || C <= 0 || K < 1 || K > CLN_MAX_K) return 0;
  return cln_chunks(rows) * (int64_t)(2 * K + 2) * C;
}

int anemoi_cond_layer_norm_backward(int dtype, const void* dy, int64_t ldd, const void* x, int64_t ldx, const float* stats,
                                    const float* cond, int64_t ldc, int K, const float* Ws, int64_t ldw, const float* bs,
                                    const float* Wb, void* dx, int64_t ldo, float* dcond, float* dWs, float* dbs, float* dWb,
                                    float* dbb, int64_t rows, int C, float* workspace, int64_t workspace_floats,
                                    anemoi_stream_t stream) {
  ANEMOI_REQUIRE(dy && x && stats && cond && Ws && bs && Wb, ANEMOI_ERR_INVALID,
                 "anemoi_cond_layer_norm_backward: null pointer");
  ANEMOI_REQUIRE(dx && dcond && dWs && dbs && dWb && dbb, ANEMOI_ERR_INVALID,
                 "anemoi_cond_layer_norm_backward: null pointer (gradient outputs)");
  ANEMOI_REQUIRE(K >= 1, ANEMOI_ERR_INVALID,
                 "anemoi_cond_layer_norm_backward: the condition needs at least one column, got K = %d", K);
  ANEMOI_REQUIRE(K <= CLN_MAX_K, ANEMOI_ERR_UNSUPPORTED, "anemoi_cond_layer_norm_backward: K = %d condition columns, at most %d",
                 K, CLN_MAX_K);
  ANEMOI_REQUIRE(C > 0 && rows > 0 && ldd >= C && ldx >= C && ldo >= C, ANEMOI_ERR_INVALID,
                 "anemoi_cond_layer_norm_backward: bad shape rows=%lld C=%d ldd=%lld ldx=%lld ldo=%lld", (long long)rows, C,
                 (long long)ldd, (long long)ldx, (long long)ldo);
  ANEMOI_REQUIRE((uintptr_t)stats % 8 == 0, ANEMOI_ERR_INVALID, "anemoi_cond_layer_norm_backward: stats must be 8-byte aligned");
  if (int rc = check_cln_padding("anemoi_cond_layer_norm_backward", cond, ldc, K, Ws, Wb, ldw)) return rc;
  const int64_t need = anemoi_cond_layer_norm_backward_workspace_floats(rows, C, K);
  ANEMOI_REQUIRE(workspace != nullptr && workspace_floats >= need, ANEMOI_ERR_INVALID,
                 "anemoi_cond_layer_norm_backward: workspace of %lld floats, %lld needed", (long long)workspace_floats,
                 (long long)need);
  hipStream_t st = as_stream(stream);
  int rc;
  if (dtype == ANEMOI_F32)
    rc = cond_layer_norm_backward_launch<float>(dy, ldd, x, ldx, stats, cond, ldc, K, Ws, ldw, bs, Wb, dx, ldo, dcond, dWs, dbs,
                                                dWb, dbb, rows, C, workspace, st);
  else if (dtype == ANEMOI_BF16)
    rc = cond_layer_norm_backward_launch<bf16_t>(dy, ldd, x, ldx, stats, cond, ldc, K, Ws, ldw, bs, Wb, dx, ldo, dcond, dWs, dbs,
                                                 dWb, dbb, rows, C, workspace, st);
  else
    return fail(ANEMOI_ERR_UNSUPPORTED, "anemoi_cond_layer_norm_backward: dtype %d", dtype);
  const char* who = "anemoi_cond_layer_norm_backward";
  rc = trail::note(rc, who, "dx", dtype, dx, ldo, rows, C, st);
  rc = trail::note(rc, who, "dcond", ANEMOI_F32, dcond, K, rows, K, st);
  rc = trail::note(rc, who, "dWs", ANEMOI_F32, dWs, K, C, K, st);
  rc = trail::note(rc, who, "dbs", ANEMOI_F32, dbs, C, 1, C, st);
  rc = trail::note(rc, who, "dWb", ANEMOI_F32, dWb, K, C, K, st);
  return trail::note(rc, who, "dbb", ANEMOI_F32, dbb, C, 1, C, st);
}

int anemoi_gaussian_noise(float* out, int64_t rows, int K, float std, uint32_t seed, const void* seed_dev,
                          anemoi_stream_t stream) {
  ANEMOI_REQUIRE(out != nullptr, ANEMOI_ERR_INVALID, "anemoi_gaussian_noise: null pointer");
  ANEMOI_REQUIRE(rows >= 0 && K >= 1, ANEMOI_ERR_INVALID, "anemoi_gaussian_noise: bad shape rows=%lld K=%d", (long long)rows, K);
  ANEMOI_REQUIRE(std >= 0.f, ANEMOI_ERR_INVALID, "anemoi_gaussian_noise: std must be >= 0, got %g", (double)std);
  ANEMOI_REQUIRE(seed_dev == nullptr || (uintptr_t)seed_dev % 4 == 0, ANEMOI_ERR_INVALID,
                 "anemoi_gaussian_noise: seed_dev must be 4-byte aligned");
  const int64_t n = rows * (int64_t)K;
  if (n == 0) return ANEMOI_OK;
  hipStream_t st = as_stream(stream);
  int64_t blocks = ((n + 3) / 4 + 255) / 256;
  if (blocks > 256 * 16) blocks = 256 * 16;  // grid-stride the rest
  hipLaunchKernelGGL(gaussian_noise_kernel, dim3((unsigned)blocks), dim3(256), 0, st, out, n, std, seed,
                     static_cast<const uint32_t*>(seed_dev));
  return trail::note(check_launch("anemoi_gaussian_noise"), "anemoi_gaussian_noise", "out", ANEMOI_F32, out, K, rows, K, st);
}

}  // extern "C"
