// Thin Linear: y[M, N] = epilogue(x[M, K] W^T + b) for bf16 operands whose WEIGHT is small enough to stay in the four waves'
// registers for the whole launch (include/anemoi_amd.h, anemoi_linear_thin).
//
// The products this serves -- the decoder's extraction Linear (K = 1024, N = 80), the per-head products on either side of
// the raw-row edge phase (64 <-> 256 per head) and the embedding-variance operator (256 x 256, only its row statistics are
// wanted) -- move one long activation matrix once and multiply it with a few kilobytes of weight.  On the tiled kernels of
// gemm.hip they pay an LDS round trip per operand byte, re-stage W for every tile and, on the 128 x 128 kernel, leave most
// of an N = 80 tile empty.  Here W is loaded ONCE per wave into VGPRs in the MFMA operand layout; the rows of x go global ->
// VGPR directly in the same layout (lane l: row l & 15, the eight consecutive k at (l >> 4) * 8 of every 32-k step, one
// 16-byte load each), several 16-row blocks in flight per wave; v_mfma_f32_16x16x32_bf16 through the compiler builtin.
// No LDS-DMA, and LDS only where a row's result is spread over the waves (KSPLIT partial sums, NSPLIT row statistics), added
// in wave order -- no atomics, so two launches give the same bits.
//
// This is a separate file with its own entry point on purpose: the fused Linear family's dispatch (gemm.hip::linear_plan) is
// pinned argument set by argument set by tests/test_linear_ref_cpu.py, and nothing here changes what that family routes where.
// The caller asks for this kernel by shape (ops.linear_thin) and keeps the family's route when it is refused.

#include <type_traits>

#include "common.hpp"
#include "gemm_thin_plan.hpp"
#include "trail.hpp"

namespace anemoi {
namespace thin {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;

struct Params {
  const bf16_t* x;
  const bf16_t* w;
  const float* bias;
  const float* colsum;
  const float2* stats;
  const bf16_t* res;
  void* y;
  float2* stats_out;
  int64_t ldx, ldr, ldy, M, row_blocks;
  int64_t sx, sw, sy, sr;  // element offsets between the problems of a batched launch
  int N;                   // all columns of one problem (a wave may hold a part)
  int out_f32, pair;
  float eps;
};

template <bool STREAM>
__device__ __forceinline__ bf16x8_t load_frag(const bf16_t* p) {
  const u32x4_t* q = reinterpret_cast<const u32x4_t*>(p);
  if constexpr (STREAM) return __builtin_bit_cast(bf16x8_t, __builtin_nontemporal_load(q));  // the one-pass x stream
  return __builtin_bit_cast(bf16x8_t, *q);
}

// First of the four consecutive output columns that lane quarter `q` holds of MFMA tile `j` (relative to the wave's first
// column).  Plain: tile j = columns 16 j .. 16 j + 15.  Paired: tiles 2 i and 2 i + 1 interleave so that a lane's eight values
// are CONSECUTIVE columns (one 16-byte bf16 store): the weight rows are simply loaded in that order.
__device__ __forceinline__ int col_of(int j, int q, int pair) {
  return pair ? (j >> 1) * 32 + q * 8 + (j & 1) * 4 : j * 16 + q * 4;
}

enum { OUT_BF16 = 0, OUT_F32 = 1, OUT_STATS = 2 };

// The per-column epilogue operands of one problem, { colsum | bias } (zeros where absent), copied to LDS once per workgroup:
// the epilogue then reads them with ds_read, which the vector-memory counter does not see.  Every global load inside the row
// loop -- the x blocks in flight, the row statistics, the residual -- is issued unconditionally and in a fixed order, so that
// the wait in front of a block's MFMAs leaves exactly the younger loads outstanding; a load under a branch, or an epilogue
// load issued behind the prefetch, makes the compiler wait for everything (vmcnt(0)) and the blocks in flight are lost.
template <int N>
__device__ __forceinline__ void fill_table(float (&tab)[2][N], const Params& p, int bias_off) {
  for (int n = threadIdx.x; n < N; n += 256) {
    tab[0][n] = p.colsum != nullptr ? p.colsum[n] : 0.f;
    tab[1][n] = p.bias != nullptr ? p.bias[bias_off + n] : 0.f;
  }
  __syncthreads();
}

// LayerNorm fold, bias and the bf16 rounding of four consecutive columns (cs, b: their table entries).
__device__ __forceinline__ void finish4(float (&v)[4], bool fold, float2 st, float4 cs, float4 b, bool round) {
  if (fold) {
    v[0] = fmaf(v[0], st.x, st.y * cs.x);
    v[1] = fmaf(v[1], st.x, st.y * cs.y);
    v[2] = fmaf(v[2], st.x, st.y * cs.z);
    v[3] = fmaf(v[3], st.x, st.y * cs.w);
  }
  v[0] += b.x;
  v[1] += b.y;
  v[2] += b.z;
  v[3] += b.w;
  if (round) {  // the value as a bf16 store leaves it: what the statistics are taken of, and what the residual is added to
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = bf16_to_f32(f32_to_bf16(v[i]));
  }
}

__device__ __forceinline__ void add4(float (&v)[4], uint2 r) {
  v[0] += __uint_as_float(r.x << 16);
  v[1] += __uint_as_float(r.x & 0xffff0000u);
  v[2] += __uint_as_float(r.y << 16);
  v[3] += __uint_as_float(r.y & 0xffff0000u);
}

// ------------------------------------------------------------------------------------------------ ROWS / NSPLIT
// K: the whole reduction, NT: 16-column tiles a wave holds.  ROWS: NT 16 = N, wave w of workgroup b takes the row blocks
// 4 b + w, + 4 gridDim.x, ...  NSPLIT: 4 NT 16 = N, the workgroup takes the row blocks b, b + gridDim.x, ... and wave w the
// columns from w NT 16 on.  PF: row blocks in flight per wave.  OUT: what leaves (OUT_*), RES: with a residual.
template <int K, int NT, bool NSPLIT, int PF, int OUT, bool RES>
__global__ __launch_bounds__(256) void thin_rows_kernel(Params p) {
  constexpr int KF = K / 32, N = NT * 16 * (NSPLIT ? 4 : 1);
  __shared__ __attribute__((aligned(16))) float tab[2][N];
  __shared__ float red[2][4][16];  // NSPLIT statistics: the waves' partial row sums
  const int lane = threadIdx.x & 63, fr = lane & 15, fq = lane >> 4;
  const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t h = blockIdx.y;
  const bf16_t* X = p.x + h * p.sx;
  const bf16_t* W = p.w + h * p.sw;
  const int col0 = NSPLIT ? wid * NT * 16 : 0;
  const int pair = OUT == OUT_BF16 ? p.pair : 0;
  const bool fold = p.stats != nullptr, round = !p.out_f32;
  fill_table<N>(tab, p, (int)h * N);

  // (32-bit block indices: the launcher refuses more than 2^30 row blocks; scalar compares keep the row loop's branches scalar)
  const int nrb = (int)p.row_blocks;
  const int first = NSPLIT ? (int)blockIdx.x : (int)blockIdx.x * 4 + wid;
  const int step = NSPLIT ? (int)gridDim.x : (int)gridDim.x * 4;
  if (first >= nrb) return;  // (ROWS only, a wave without a row block: the launcher gives every workgroup one; no barrier follows in ROWS)

  bf16x8_t wf[NT][KF];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int n = col0 + col_of(j, fr >> 2, pair) + (fr & 3);  // (< N: col_of permutes the wave's NT 16 columns)
#pragma unroll
    for (int ks = 0; ks < KF; ++ks) wf[j][ks] = load_frag<false>(W + (int64_t)n * K + ks * 32 + fq * 8);
  }

  // A row block in flight: its x fragments AND the epilogue's per-row global operands.  Loads return in order, so an epilogue
  // operand fetched when its block is computed would make the wave wait for every older load -- all the blocks in flight.
  struct Block {
    bf16x8_t x[KF];
    float2 st;               // LayerNorm-fold statistics of the lane's row (absent: a valid address is read and not used)
    uint2 rv[RES ? NT : 1];  // the residual's four columns of every tile
  };
  Block xb[PF];
  auto load_block = [&](int rb, Block& dst) {
    int64_t m = (int64_t)rb * 16 + fr;
    if (m > p.M - 1) m = p.M - 1;  // ragged last block: the rows behind M - 1 re-read row M - 1 and are never stored
    const bf16_t* xr = X + m * p.ldx + fq * 8;
#pragma unroll
    for (int ks = 0; ks < KF; ++ks) dst.x[ks] = load_frag<!NSPLIT>(xr + ks * 32);
    dst.st = *(fold ? p.stats + m : reinterpret_cast<const float2*>(p.w));
    if constexpr (RES) {
      const bf16_t* rr = p.res + h * p.sr + m * p.ldr + col0;
#pragma unroll
      for (int j = 0; j < NT; ++j) dst.rv[j] = *reinterpret_cast<const uint2*>(rr + col_of(j, fq, pair));
    }
  };
#pragma unroll
  for (int s = 0; s < PF; ++s) {
    const int rb = first + s * step;
    __builtin_amdgcn_sched_barrier(0);  // block s whole before block s + 1: the waits of the row loop count the younger loads
    load_block(rb < nrb ? rb : first, xb[s]);  // (a block behind the end: any valid one, never used)
  }
  __builtin_amdgcn_sched_barrier(0);

  // One row block: MFMAs on its fragments, the epilogue in registers, the next block into the same slot (PREFETCH), the
  // stores.  Every branch around it is uniform (per wave in ROWS, per workgroup in NSPLIT: the barriers inside are safe).
  auto process = [&](int rb, Block& xs, auto prefetch) {
      f32x4_t acc[NT];
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KF; ++ks)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j][ks], xs.x[ks], acc[j], 0, 0, 0);

      // lane holds row m = 16 rb + fr, columns col0 + col_of(j, fq) + 0..3 of every tile j
      const int64_t m = (int64_t)rb * 16 + fr;
      const bool valid = m < p.M;
      const float2 st = xs.st;
      float v[NT][4];
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int n = col0 + col_of(j, fq, pair);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[j][i] = acc[j][i];
        finish4(v[j], fold, st, *reinterpret_cast<const float4*>(&tab[0][n]), *reinterpret_cast<const float4*>(&tab[1][n]), round);
        if constexpr (RES) add4(v[j], xs.rv[j]);
      }
      __builtin_amdgcn_sched_barrier(0);  // the slot's operands are consumed: refill it before the stores
      if constexpr (decltype(prefetch)::value) {
        const int nx = rb + PF * step;
        load_block(nx < nrb ? nx : rb, xs);
      }
      __builtin_amdgcn_sched_barrier(0);

      if constexpr (OUT == OUT_STATS) {  // the two-pass formula of row_stats_kernel on the row in registers
        // (NSPLIT: red[0] is written again only behind the second barrier of this block, red[1] behind the first of the next)
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
          for (int i = 0; i < 4; ++i) sum += v[j][i];
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        if constexpr (NSPLIT) {
          if (fq == 0) red[0][wid][fr] = sum;
          __syncthreads();
          sum = ((red[0][0][fr] + red[0][1][fr]) + red[0][2][fr]) + red[0][3][fr];
        }
        const float mean = sum / (float)N;
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float d = v[j][i] - mean;
            q += d * d;
          }
        q += __shfl_xor(q, 16, 64);
        q += __shfl_xor(q, 32, 64);
        if constexpr (NSPLIT) {
          if (fq == 0) red[1][wid][fr] = q;
          __syncthreads();
          q = ((red[1][0][fr] + red[1][1][fr]) + red[1][2][fr]) + red[1][3][fr];
        }
        const float rstd = rsqrtf(q / (float)N + p.eps);
        if (valid && fq == 0 && (!NSPLIT || wid == 0)) p.stats_out[m] = make_float2(rstd, -mean * rstd);
      } else {
        if (valid) {
          if constexpr (OUT == OUT_F32) {
            float* yr = static_cast<float*>(p.y) + h * p.sy + m * p.ldy + col0;
#pragma unroll
            for (int j = 0; j < NT; ++j) VecIO<float, 4>::store(yr + col_of(j, fq, 0), v[j]);
          } else {
            bf16_t* yr = static_cast<bf16_t*>(p.y) + h * p.sy + m * p.ldy + col0;
            if constexpr (NT % 2 == 0) {  // (the launcher pairs exactly these kernels' bf16 stores)
#pragma unroll
              for (int j = 0; j < NT; j += 2) {
                const float o[8] = {v[j][0], v[j][1], v[j][2], v[j][3], v[j + 1][0], v[j + 1][1], v[j + 1][2], v[j + 1][3]};
                VecIO<bf16_t, 8>::store(yr + col_of(j, fq, 1), o);
              }
            } else {
#pragma unroll
              for (int j = 0; j < NT; ++j) VecIO<bf16_t, 4>::store(yr + col_of(j, fq, 0), v[j]);
            }
          }
        }
      }
  };

  // Whole rounds of PF blocks, with no way out in between: every path to a block's MFMAs then carries the same number of
  // younger loads, and the wait in front of them leaves the other blocks in flight.  (An exit inside the round joins the
  // loop's latch in the compiler's CFG; the never-taken path exit -> latch -> block 0 then forces vmcnt(0) on block 0.)
  int rb0 = first;
  for (; rb0 + (PF - 1) * step < nrb; rb0 += PF * step) {
#pragma unroll
    for (int s = 0; s < PF; ++s) process(rb0 + s * step, xb[s], std::true_type{});
  }
  // the last, partial round: its blocks are in xb already
#pragma unroll
  for (int s = 0; s < PF - 1; ++s)
    if (rb0 + s * step < nrb) process(rb0 + s * step, xb[s], std::false_type{});
}

// ------------------------------------------------------------------------------------------------ KSPLIT
// KW = K / 4: the k range of one wave, NT 16 = N.  The workgroup takes the row blocks b, b + gridDim.x, ...; every wave
// multiplies its quarter of k, the four f32 partial tiles meet in LDS (two buffers: one barrier per block) and thread t adds
// them in wave order for row t >> 4, columns 4 (t & 15) + 64 i, then runs the epilogue.
template <int KW, int NT, int PF, int OUT, bool RES>
__global__ __launch_bounds__(256) void thin_ksplit_kernel(Params p) {
  constexpr int KF = KW / 32, K = 4 * KW, N = NT * 16, LDP = N + 4, CI = (N + 63) / 64;
  __shared__ __attribute__((aligned(16))) float part[2][4][16][LDP];
  __shared__ __attribute__((aligned(16))) float tab[2][N];
  const int lane = threadIdx.x & 63, fr = lane & 15, fq = lane >> 4;
  const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const bf16_t* X = p.x + wid * KW;
  const bf16_t* W = p.w + wid * KW;
  const bool fold = p.stats != nullptr, round = !p.out_f32;
  fill_table<N>(tab, p, 0);
  const int er = threadIdx.x >> 4, ec = (threadIdx.x & 15) * 4;  // this thread's row and first column in the epilogue

  bf16x8_t wf[NT][KF];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int ks = 0; ks < KF; ++ks) wf[j][ks] = load_frag<false>(W + (int64_t)(j * 16 + fr) * K + ks * 32 + fq * 8);

  const int nrb = (int)p.row_blocks, first = (int)blockIdx.x, step = (int)gridDim.x;  // (first < nrb: the launcher's grid)
  struct Block {  // (see thin_rows_kernel; st and rv belong to the thread's EPILOGUE row 16 rb + er)
    bf16x8_t x[KF];
    float2 st;
    uint2 rv[RES ? CI : 1];
  };
  Block xb[PF];
  auto load_block = [&](int rb, Block& dst) {
    int64_t m = (int64_t)rb * 16 + fr;
    if (m > p.M - 1) m = p.M - 1;
    const bf16_t* xr = X + m * p.ldx + fq * 8;
#pragma unroll
    for (int ks = 0; ks < KF; ++ks) dst.x[ks] = load_frag<true>(xr + ks * 32);
    int64_t me = (int64_t)rb * 16 + er;
    if (me > p.M - 1) me = p.M - 1;
    dst.st = *(fold ? p.stats + me : reinterpret_cast<const float2*>(p.w));
    if constexpr (RES) {
#pragma unroll
      for (int i = 0; i < CI; ++i) dst.rv[i] = *reinterpret_cast<const uint2*>(p.res + me * p.ldr + (ec + i * 64 < N ? ec + i * 64 : 0));
    }
  };
#pragma unroll
  for (int s = 0; s < PF; ++s) {
    const int rb = first + s * step;
    __builtin_amdgcn_sched_barrier(0);
    load_block(rb < nrb ? rb : first, xb[s]);
  }
  __builtin_amdgcn_sched_barrier(0);

  int buf = 0;
  auto process = [&](int rb, Block& xs, auto prefetch) {  // (uniform over the workgroup; see thin_rows_kernel)
      f32x4_t acc[NT];
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KF; ++ks)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j][ks], xs.x[ks], acc[j], 0, 0, 0);

      const int64_t m = (int64_t)rb * 16 + er;
      const bool valid = m < p.M;
      const float2 st = xs.st;  // (copies: the slot is refilled before the epilogue runs)
      uint2 rv[RES ? CI : 1];
      if constexpr (RES) {
#pragma unroll
        for (int i = 0; i < CI; ++i) rv[i] = xs.rv[i];
      }
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (decltype(prefetch)::value) {
        const int nx = rb + PF * step;
        load_block(nx < nrb ? nx : rb, xs);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < NT; ++j)
        *reinterpret_cast<float4*>(&part[buf][wid][fr][j * 16 + fq * 4]) = make_float4(acc[j][0], acc[j][1], acc[j][2], acc[j][3]);
      __syncthreads();

      float v[CI][4];
#pragma unroll
      for (int i = 0; i < CI; ++i) {
        const int c = ec + i * 64;
        if (c < N) {
          const float4 a0 = *reinterpret_cast<const float4*>(&part[buf][0][er][c]);
          const float4 a1 = *reinterpret_cast<const float4*>(&part[buf][1][er][c]);
          const float4 a2 = *reinterpret_cast<const float4*>(&part[buf][2][er][c]);
          const float4 a3 = *reinterpret_cast<const float4*>(&part[buf][3][er][c]);
          v[i][0] = ((a0.x + a1.x) + a2.x) + a3.x;
          v[i][1] = ((a0.y + a1.y) + a2.y) + a3.y;
          v[i][2] = ((a0.z + a1.z) + a2.z) + a3.z;
          v[i][3] = ((a0.w + a1.w) + a2.w) + a3.w;
          finish4(v[i], fold, st, *reinterpret_cast<const float4*>(&tab[0][c]), *reinterpret_cast<const float4*>(&tab[1][c]), round);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[i][e] = 0.f;
        }
      }
      buf ^= 1;

      if constexpr (OUT == OUT_STATS) {  // a row lives in the 16 lanes t & 15 of one wave
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < CI; ++i)
          if (ec + i * 64 < N) sum += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
        const float mean = group_sum<16>(sum) / (float)N;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < CI; ++i)
          if (ec + i * 64 < N) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float d = v[i][e] - mean;
              q += d * d;
            }
          }
        const float rstd = rsqrtf(group_sum<16>(q) / (float)N + p.eps);
        if (valid && (threadIdx.x & 15) == 0) p.stats_out[m] = make_float2(rstd, -mean * rstd);
      } else {
#pragma unroll
        for (int i = 0; i < CI; ++i) {
          const int c = ec + i * 64;
          if (valid && c < N) {
            if constexpr (RES) add4(v[i], rv[i]);
            if constexpr (OUT == OUT_F32)
              VecIO<float, 4>::store(static_cast<float*>(p.y) + m * p.ldy + c, v[i]);
            else
              VecIO<bf16_t, 4>::store(static_cast<bf16_t*>(p.y) + m * p.ldy + c, v[i]);
          }
        }
      }
  };

  int rb0 = first;
  for (; rb0 + (PF - 1) * step < nrb; rb0 += PF * step) {
#pragma unroll
    for (int s = 0; s < PF; ++s) process(rb0 + s * step, xb[s], std::true_type{});
  }
#pragma unroll
  for (int s = 0; s < PF - 1; ++s)
    if (rb0 + s * step < nrb) process(rb0 + s * step, xb[s], std::false_type{});
}

typedef void (*Kernel)(Params);
// { OUT_BF16, OUT_F32, OUT_STATS } without, then with a residual (PFR blocks in flight: the residual's columns travel with them)
#define ANEMOI_THIN_ROWS(K, NT, NS, PF, PFR)                                                                     \
  {                                                                                                              \
    thin_rows_kernel<K, NT, NS, PF, OUT_BF16, false>, thin_rows_kernel<K, NT, NS, PF, OUT_F32, false>,           \
        thin_rows_kernel<K, NT, NS, PF, OUT_STATS, false>, thin_rows_kernel<K, NT, NS, PFR, OUT_BF16, true>,     \
        thin_rows_kernel<K, NT, NS, PFR, OUT_F32, true>, nullptr                                                 \
  }
#define ANEMOI_THIN_KSPLIT(KW, NT, PF)                                                                           \
  {                                                                                                              \
    thin_ksplit_kernel<KW, NT, PF, OUT_BF16, false>, thin_ksplit_kernel<KW, NT, PF, OUT_F32, false>,             \
        thin_ksplit_kernel<KW, NT, PF, OUT_STATS, false>, thin_ksplit_kernel<KW, NT, PF, OUT_BF16, true>,        \
        thin_ksplit_kernel<KW, NT, PF, OUT_F32, true>, nullptr                                                   \
  }
// in the order of thin::SHAPES.  Launched one workgroup per CU (thin::SHAPES): the wide kernels need that (256 VGPRs + 72 - 192
// AGPRs per lane); the N = 16 and K = 128 ones (186 - 272 registers) would fit two and are small enough not to matter.  No spills.
static const Kernel KERNELS[N_SHAPES][6] = {
    ANEMOI_THIN_ROWS(64, 16, false, 4, 2),  // N = 256, K = 64: W 128 VGPRs, accumulators 64, blocks of 8 (x) + 32 (residual)
    ANEMOI_THIN_ROWS(256, 4, false, 4, 4),  // N = 64, K = 256: W 128, accumulators 16, blocks of 32 + 8
    ANEMOI_THIN_ROWS(256, 4, true, 6, 6),   // N = 256, K = 256: a quarter of the columns per wave, blocks of 32 + 8
    ANEMOI_THIN_KSPLIT(256, 5, 3),          // N = 80, K = 1024: W 160, accumulators 20, blocks of 32
    ANEMOI_THIN_KSPLIT(256, 1, 3),          // N = 16, K = 1024
    ANEMOI_THIN_ROWS(256, 1, false, 4, 4),  // N = 16, K = 256
    ANEMOI_THIN_ROWS(128, 4, true, 8, 8),   // N = 256, K = 128 (the variance operator of a 128-wide raw row)
};

// compute units of the current device, asked of the runtime once per device ordinal (0: no device)
static int device_cus() {
  static std::atomic<int> cached[256] = {};
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  std::atomic<int>& slot = cached[dev & 255];
  cus = slot.load(std::memory_order_relaxed);
  if (cus > 0) return cus;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
  slot.store(cus, std::memory_order_relaxed);
  return cus;
}

}  // namespace thin
}  // namespace anemoi

using namespace anemoi;

extern "C" int anemoi_linear_thin(const anemoi_linear_thin_args* args, anemoi_stream_t stream) {
  thin::Plan pl;
  // (the plan judges the argument block before it looks at the CU count: a refused or invalid block needs no device)
  int rc = thin::plan(args, thin::device_cus(), pl);
  if (rc != ANEMOI_OK) return rc;
  thin::Params p;
  p.x = static_cast<const bf16_t*>(args->x);
  p.w = static_cast<const bf16_t*>(args->w);
  p.bias = args->bias;
  p.colsum = args->colsum;
  p.stats = reinterpret_cast<const float2*>(args->stats);
  p.res = static_cast<const bf16_t*>(args->residual);
  p.y = args->y;
  p.stats_out = reinterpret_cast<float2*>(args->stats_out);
  p.ldx = args->ldx;
  p.ldr = args->ldr;
  p.ldy = args->ldy;
  p.M = args->M;
  p.row_blocks = pl.row_blocks;
  const bool batched = args->batch > 1;
  p.sx = batched ? args->stride_x : 0;
  p.sw = batched ? args->stride_w : 0;
  p.sy = batched ? args->stride_y : 0;
  p.sr = batched ? args->stride_r : 0;
  p.N = args->N;
  p.out_f32 = args->out_dtype == ANEMOI_F32;
  p.pair = pl.pair;
  p.eps = args->eps;
  const int out = args->stats_out != nullptr ? thin::OUT_STATS : (p.out_f32 ? thin::OUT_F32 : thin::OUT_BF16);
  hipLaunchKernelGGL(thin::KERNELS[pl.shape][out + (args->residual != nullptr ? 3 : 0)], dim3(pl.grid_x, pl.grid_y), dim3(256), 0, as_stream(stream), p);
  rc = check_launch("anemoi_linear_thin");
  if (args->stats_out != nullptr)
    return trail::note(rc, "anemoi_linear_thin", "stats", ANEMOI_F32, args->stats_out, 2, args->M, 2, as_stream(stream));
  if (!batched) return trail::note(rc, "anemoi_linear_thin", "out", args->out_dtype, args->y, args->ldy, args->M, args->N, as_stream(stream));
  if (trail::armed_state() == nullptr) return rc;
  const int esz = args->out_dtype == ANEMOI_BF16 ? 2 : 4;
  for (int b = 0; b < args->batch; ++b)
    rc = trail::note(rc, "anemoi_linear_thin", "out", args->out_dtype, static_cast<const char*>(args->y) + b * args->stride_y * esz,
                     args->ldy, args->M, args->N, as_stream(stream));
  return rc;
}
