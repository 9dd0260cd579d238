// Split-bf16 ("bf16x3") Linear  y = act(x @ W^T + bias) + residual  for f32 storage on the bf16 matrix cores.
//
// Every f32 operand v is written as hi + lo with hi = bf16(v), lo = bf16(v - hi) (round to nearest even both times:
// 16 significand bits together) and the product is formed as
//     x W^T  ~=  x_hi W_hi^T + x_hi W_lo^T + x_lo W_hi^T        (x_lo W_lo^T, ~2^-18 relative, is dropped)
// on three v_mfma_f32_16x16x32_bf16 per (W fragment, x fragment) pair with ONE f32 accumulator.  The error against the exact
// product is ~4e-6 rms relative (the f32 kernel: 3e-7, bf16 operands: 2e-3) at 3x the bf16 MFMA work, i.e. a ceiling of
// 2.5 PFLOP/s / 3 = 833 TFLOP/s of f32-equivalent work against the 157 TFLOP/s of v_mfma_f32_32x32x2_f32.
//
// Domain: finite inputs with |v| < 2^126.  bf16(v) of a value next to the f32 maximum rounds to infinity and v - hi is then
// NaN; +-infinity in x or W gives NaN where the exact kernel gives +-infinity.  NaN in -> NaN out holds (hi = NaN).
//
// Weights are split ONCE (anemoi_split_weight: two bf16 planes [N, K]); x is split INSIDE the GEMM, at the fragment read:
// the f32 slab of x is staged by LDS-DMA exactly as gemm.hip::linear_kernel stages it (no VGPR round trip, no extra HBM
// pass, no second LDS image to write), and each lane converts the 8 f32 values of its fragment into a hi and a lo bf16x8.
// The price of that placement: an x fragment is read by the two waves of a wave row, so the conversion is done twice.
//
// Tile: 128 (M) x 128 (N) per 256-thread workgroup, 4 waves as 2 (M) x 2 (N), 4 x 4 tiles of 16x16x32 per wave, K-slab of
// 32 elements = one MFMA k-step: 128 B per x row (f32), 64 B per row of each W plane (bf16).  Two stages of
// 16 KiB (x) + 8 KiB (W_hi) + 8 KiB (W_lo) = 64 KiB of LDS, one barrier per slab, 8 LDS-DMAs per wave and slab.
// As in gemm.hip the MFMA "A" operand is the W fragment and "B" the x fragment, so a lane ends up with 4 consecutive output
// columns of one row and the epilogue works on 16-byte vectors.
//
// Budget per K-slab and wave (cycles of one SIMD; MFMA 16x16x32 bf16 = 16 cycles back to back, a wave64 VALU op = 4):
//   MFMA   4 x 4 pairs x 3 products = 48 MFMAs                                   = 768 cycles
//   VALU   4 x fragments x (4 v_cvt_pk_bf16_f32 [hi] + 8 shift/and [hi back to f32] + 8 v_sub_f32 + 4 v_cvt_pk_bf16_f32 [lo])
//          = 96 ops                                                               = 384 cycles   (VALU : MFMA = 0.50)
//   LDS    8 ds_read_b128 (x: 2 per fragment) + 8 ds_read_b128 (W: hi and lo of 4 fragments)
// (The compiler packs the 32 subtractions into 16 v_pk_add_f32: 80 ops in the listing.)  Measured: 0.34 - 0.37 of the
// 833 TFLOP/s ceiling at M = 40 962, K >= 1024, 2.4 - 2.8 x the exact f32 kernel.
// Staging moves 256 B per K-element pair of rows (128 B x + 2 x 64 B W) for 3 MFMAs where the bf16 kernel moves 128 B for
// one, so the MFMA work per staged byte is 1.5x that of gemm.hip's 128 x 128 bf16 kernel.
//
// MFMAs are the compiler builtins: the compiler owns their wait states (tools/isa_hazard_audit.py checks the listing).
#include "common.hpp"
#include "trail.hpp"

namespace anemoi {
namespace split {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;

constexpr int BM = 128, BN = 128, BK = 32;
constexpr int X_ROW = BK * 4, W_ROW = BK * 2;          // bytes per LDS row
constexpr int X_TILE = BM * X_ROW, W_TILE = BN * W_ROW;  // 16 KiB, 8 KiB
constexpr int STAGE = X_TILE + 2 * W_TILE;              // 32 KiB

__device__ __forceinline__ void glds16(const void* gptr, void* lptr) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gptr,
                                   (__attribute__((address_space(3))) void*)lptr, 16, 0, 0);
}

// Bank swizzles of the lane-linear LDS images (applied to the DMA's source chunk, undone at the fragment read).
//   x   128-B rows, 8 chunks: the 16 rows of a fragment read (stride 128 B) cover 8 masks x 2 halves of the 256-B bank row
//   W   64-B rows, 4 chunks: rows r .. r+3 fill one bank row, each next group of 4 rows takes the next chunk position
__device__ __forceinline__ int swz_x(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }
__device__ __forceinline__ int swz_w(int row, int chunk) { return chunk ^ ((row >> 2) & 3); }

// hi / lo bf16 pairs of two f32 values (one v_cvt_pk_bf16_f32 each; the hi values go back to f32 by shift / mask)
__device__ __forceinline__ void split2(float a, float b, uint32_t& hi, uint32_t& lo) {
  hi = pack_bf16x2(a, b);
  lo = pack_bf16x2(a - __uint_as_float(hi << 16), b - __uint_as_float(hi & 0xffff0000u));
}

__device__ __forceinline__ void epilogue4(const f32x4_t& acc, int64_t m, int n, int64_t M, int N,
                                          const float* __restrict__ bias, const float* __restrict__ R, int64_t ldr,
                                          float* __restrict__ Y, int64_t ldy, int act, bool vec_ok) {
  if (m >= M || n >= N) return;
  if (vec_ok && n + 4 <= N) {
    float o[4] = {acc[0], acc[1], acc[2], acc[3]};
    if (bias != nullptr) {
      float b[4];
      VecIO<float, 4>::load(bias + n, b);
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] += b[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = act_apply(o[i], act);
    if (R != nullptr) {
      float r[4];
      VecIO<float, 4>::load(R + m * ldr + n, r);
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] += r[i];
    }
    VecIO<float, 4>::store(Y + m * ldy + n, o);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (n + i < N) {
        float t = acc[i] + (bias != nullptr ? bias[n + i] : 0.f);
        t = act_apply(t, act);
        if (R != nullptr) t += R[m * ldr + n + i];
        Y[m * ldy + n + i] = t;
      }
    }
  }
}

__global__ __launch_bounds__(256) void linear_split_kernel(const float* __restrict__ X, int64_t ldx,
                                                           const bf16_t* __restrict__ Whi,
                                                           const bf16_t* __restrict__ Wlo,
                                                           const float* __restrict__ bias, const float* __restrict__ R,
                                                           int64_t ldr, float* __restrict__ Y, int64_t ldy, int64_t M, int N,
                                                           int K, int act, int vec_ok) {
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];  // 64 KiB
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int nt_count = (N + BN - 1) / BN;
  const int nt = blockIdx.x % nt_count;
  const int64_t m0 = (int64_t)(blockIdx.x / nt_count) * BM;
  const int n0 = nt * BN;
  const int nk = K / BK;

  // ---- staging.  x: wave `wid` moves row groups wid*4 .. wid*4+3 (8 rows x 128 B per DMA); each W plane: row groups
  // wid*2, wid*2+1 (16 rows x 64 B per DMA).  Rows behind M / N are clamped to the last valid row (never stored).
  const char* xg[4];
  const char* whg[2];
  const char* wlg[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = (wid * 4 + i) * 8 + (lane >> 3);
    int64_t gm = m0 + r;
    if (gm > M - 1) gm = M - 1;
    xg[i] = reinterpret_cast<const char*>(X + gm * ldx) + swz_x(r, lane & 7) * 16;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = (wid * 2 + i) * 16 + (lane >> 2);
    int gn = n0 + r;
    if (gn > N - 1) gn = N - 1;
    const int64_t off = (int64_t)gn * K * 2 + swz_w(r, lane & 3) * 16;
    whg[i] = reinterpret_cast<const char*>(Whi) + off;
    wlg[i] = reinterpret_cast<const char*>(Wlo) + off;
  }
  auto stage = [&](int kt, int buf) {
    char* xs = smem + buf * STAGE + wid * 4096;
    char* hs = smem + buf * STAGE + X_TILE + wid * 2048;
    char* ls = hs + W_TILE;
#pragma unroll
    for (int i = 0; i < 4; ++i) glds16(xg[i] + (int64_t)kt * X_ROW, xs + i * 1024);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      glds16(whg[i] + (int64_t)kt * W_ROW, hs + i * 1024);
      glds16(wlg[i] + (int64_t)kt * W_ROW, ls + i * 1024);
    }
  };

  const int wr = wid >> 1, wc = wid & 1;
  const int fr = lane & 15, fq = lane >> 4;  // lane holds k = 8 fq .. 8 fq + 7 of row fr of a fragment
  f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  stage(0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's LDS-DMA of slab kt has landed (explicit: the compiler
    __syncthreads();                                    // does not always count it at the barrier)
    if (kt + 1 < nk) stage(kt + 1, (kt + 1) & 1);
    const char* xs = smem + (kt & 1) * STAGE;
    const char* hs = xs + X_TILE;
    const char* ls = hs + W_TILE;
    bf16x8_t ah[4], al[4], bh[4], bl[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = wc * 64 + i * 16 + fr;
      const int off = row * W_ROW + (swz_w(row, fq) << 4);
      ah[i] = *reinterpret_cast<const bf16x8_t*>(hs + off);
      al[i] = *reinterpret_cast<const bf16x8_t*>(ls + off);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = wr * 64 + j * 16 + fr;
      const f32x4_t v0 = *reinterpret_cast<const f32x4_t*>(xs + row * X_ROW + (swz_x(row, 2 * fq) << 4));
      const f32x4_t v1 = *reinterpret_cast<const f32x4_t*>(xs + row * X_ROW + (swz_x(row, 2 * fq + 1) << 4));
      uint32_t h[4], l[4];
      split2(v0[0], v0[1], h[0], l[0]);
      split2(v0[2], v0[3], h[1], l[1]);
      split2(v1[0], v1[1], h[2], l[2]);
      split2(v1[2], v1[3], h[3], l[3]);
      bh[j] = __builtin_bit_cast(bf16x8_t, u32x4_t{h[0], h[1], h[2], h[3]});
      bl[j] = __builtin_bit_cast(bf16x8_t, u32x4_t{l[0], l[1], l[2], l[3]});
    }
    // the two correction products first, the leading one last; each pass touches all 16 accumulators before any is reused
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
  }
  // epilogue: lane holds C[m = .. + fr][n = .. + fq*4 + 0..3]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      epilogue4(acc[i][j], m0 + wr * 64 + j * 16 + fr, n0 + wc * 64 + i * 16 + fq * 4, M, N, bias, R, ldr, Y, ldy, act,
                vec_ok != 0);
}

// One thread per 8 consecutive K-elements of a row: two float4 in, one 16-byte chunk of each plane out.
__global__ __launch_bounds__(256) void split_weight_kernel(const float* __restrict__ W, int64_t ldw,
                                                           bf16_t* __restrict__ Whi, bf16_t* __restrict__ Wlo, int64_t N,
                                                           int K) {
  const int kc = K / 8;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= N * kc) return;
  const int64_t n = idx / kc;
  const int c = (int)(idx - n * kc);
  const float4 a = *reinterpret_cast<const float4*>(W + n * ldw + c * 8);
  const float4 b = *reinterpret_cast<const float4*>(W + n * ldw + c * 8 + 4);
  uint4 h, l;
  split2(a.x, a.y, h.x, l.x);
  split2(a.z, a.w, h.y, l.y);
  split2(b.x, b.y, h.z, l.z);
  split2(b.z, b.w, h.w, l.w);
  *reinterpret_cast<uint4*>(Whi + n * K + c * 8) = h;
  *reinterpret_cast<uint4*>(Wlo + n * K + c * 8) = l;
}

}  // namespace split
}  // namespace anemoi

using namespace anemoi;

extern "C" int anemoi_split_weight(const float* w, int64_t ldw, void* w_hi, void* w_lo, int64_t N, int K,
                                   anemoi_stream_t stream) {
  ANEMOI_REQUIRE(w && w_hi && w_lo, ANEMOI_ERR_INVALID, "anemoi_split_weight: null pointer");
  ANEMOI_REQUIRE(N >= 0 && K > 0 && ldw >= K, ANEMOI_ERR_INVALID, "anemoi_split_weight: bad shape N=%lld K=%d ldw=%lld",
                 (long long)N, K, (long long)ldw);
  ANEMOI_REQUIRE(K % split::BK == 0, ANEMOI_ERR_INVALID, "anemoi_split_weight: K=%d must be a multiple of %d (pad with zeros)",
                 K, split::BK);
  ANEMOI_REQUIRE((uintptr_t)w % 16 == 0 && ldw % 4 == 0 && (uintptr_t)w_hi % 16 == 0 && (uintptr_t)w_lo % 16 == 0,
                 ANEMOI_ERR_INVALID, "anemoi_split_weight: w and the planes must be 16-byte aligned, ldw a multiple of 4");
  if (N == 0) return ANEMOI_OK;
  const int64_t blocks = (N * (K / 8) + 255) / 256;
  ANEMOI_REQUIRE(blocks < (int64_t)1 << 31, ANEMOI_ERR_UNSUPPORTED, "anemoi_split_weight: grid too large");
  hipLaunchKernelGGL(split::split_weight_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), w, ldw,
                     static_cast<bf16_t*>(w_hi), static_cast<bf16_t*>(w_lo), N, K);
  int rc = trail::note(check_launch("anemoi_split_weight"), "anemoi_split_weight", "w_hi", ANEMOI_BF16, w_hi, K, N, K, as_stream(stream));
  return trail::note(rc, "anemoi_split_weight", "w_lo", ANEMOI_BF16, w_lo, K, N, K, as_stream(stream));
}

extern "C" int anemoi_linear_split(const float* x, int64_t ldx, const void* w_hi, const void* w_lo, const float* bias,
                                   const float* residual, int64_t ldr, float* y, int64_t ldy, int64_t M, int N, int K,
                                   int act, anemoi_stream_t stream) {
  ANEMOI_REQUIRE(x && w_hi && w_lo && y, ANEMOI_ERR_INVALID, "anemoi_linear_split: null pointer");
  ANEMOI_REQUIRE(M >= 0 && N > 0 && K > 0, ANEMOI_ERR_INVALID, "anemoi_linear_split: bad shape M=%lld N=%d K=%d",
                 (long long)M, N, K);
  ANEMOI_REQUIRE(ldx >= K && ldy >= N && (residual == nullptr || ldr >= N), ANEMOI_ERR_INVALID,
                 "anemoi_linear_split: leading dimension too small");
  ANEMOI_REQUIRE(act >= ANEMOI_ACT_NONE && act <= ANEMOI_ACT_RELU, ANEMOI_ERR_INVALID, "anemoi_linear_split: act %d", act);
  ANEMOI_REQUIRE(K % split::BK == 0, ANEMOI_ERR_INVALID,
                 "anemoi_linear_split: K=%d must be a multiple of %d (pad with zeros)", K, split::BK);
  ANEMOI_REQUIRE((uintptr_t)x % 16 == 0 && ldx % 4 == 0 && (uintptr_t)w_hi % 16 == 0 && (uintptr_t)w_lo % 16 == 0,
                 ANEMOI_ERR_INVALID,
                 "anemoi_linear_split: x and the weight planes must be 16-byte aligned, ldx a multiple of 4");
  if (M == 0) return ANEMOI_OK;
  const int64_t mt = (M + split::BM - 1) / split::BM;
  const int64_t nt = (N + split::BN - 1) / split::BN;
  ANEMOI_REQUIRE(mt * nt < (int64_t)1 << 31, ANEMOI_ERR_UNSUPPORTED, "anemoi_linear_split: grid too large");
  const bool vec_ok = (N % 4 == 0) && (ldy % 4 == 0) && ((uintptr_t)y % 16 == 0) &&
                      (bias == nullptr || (uintptr_t)bias % 16 == 0) &&
                      (residual == nullptr || (ldr % 4 == 0 && (uintptr_t)residual % 16 == 0));
  hipLaunchKernelGGL(split::linear_split_kernel, dim3((unsigned)(mt * nt)), dim3(256), 0, as_stream(stream), x, ldx,
                     static_cast<const bf16_t*>(w_hi), static_cast<const bf16_t*>(w_lo), bias, residual, ldr, y, ldy, M, N,
                     K, act, vec_ok ? 1 : 0);
  return trail::note(check_launch("anemoi_linear_split"), "anemoi_linear_split", "out", ANEMOI_F32, y, ldy, M, N, as_stream(stream));
}
