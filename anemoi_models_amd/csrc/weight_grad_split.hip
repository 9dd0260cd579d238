// Split-bf16 ("bf16x3") weight gradient  dW[n, k] = sum_m dY[m, n] * x[m, k]  for f32 operands on the bf16 matrix cores.
//
// The training counterpart of gemm_split.hip.  BOTH operands are f32 activations here, both are
// row-major with the reduction index m as the slow dimension ("TN", as weight_grad.hip), and both are read as they lie: no
// transposed copies and no hi / lo planes in HBM.  Every value v is split as hi = bf16(v), lo = bf16(v - hi) (round to
// nearest even both times) and each product is formed as
//     dY^T x  ~=  dY_hi^T x_hi + (dY_hi^T x_lo + dY_lo^T x_hi)       (dY_lo^T x_lo, ~2^-18 relative, is dropped)
// on three v_mfma_f32_16x16x32_bf16 per fragment pair with ONE f32 accumulator (the two correction products first).
// Domain as gemm_split.hip: finite values below 2^126; NaN in -> NaN out (hi = NaN).
//
// Path of a value: global -> VGPR (float4, coalesced 512-byte rows, predicated: a row at or behind the end of the chunk
// / of M, or a column group at or behind N / K, is never read and enters as zeros) -> split in registers, ONCE per value
// (the forward kernel splits an x fragment in both waves of a wave row) -> four bf16 LDS planes per slab (dY_hi, dY_lo,
// x_hi, x_lo; [32 m][128 columns], 256-byte rows) -> fragments by gfx950's transposing read ds_read_b64_tr_b16, exactly as
// the validated bf16 TN kernel takes them: a 16-lane group reads a [4 m][16 columns] block and lane c receives the 4 m of
// column c; two reads make the 8-deep fragment of a lane.
//
// LDS image of a plane: row m keeps its columns, but the 32-byte slot p (16 columns) holds source slot p ^ g(m),
// g(m) = (m & 3) | ((m >> 3) & 1) << 2 -- the swizzle weight_grad.hip documents, on a 256-byte row (8 slots, so the XOR
// permutes the whole row): the eight rows a half-wave reads in one transposing read lie in eight different slots = all 64
// banks once.  A write is 8 bytes per lane, 32 lanes per row: one full row, conflict free.
//
// Tile: 128 dY columns x 128 x columns per 256-thread workgroup, four waves as 2 x 2 of 64 x 64 (4 x 4 accumulators of
// 16 x 16), reduction slabs of 32 rows = ONE MFMA k-step.  Two stages of 4 planes x 8 KiB = 64 KiB of LDS (the suggested
// 64-row slab would take 2 x 64 KiB = 128 KiB of the CU's 160 KiB: one workgroup per CU, i.e. one wave per SIMD, with
// nothing to cover the split's VALU work; 32-row slabs keep two workgroups per CU).  One barrier per slab: the global
// loads of slab t + 1 are issued before the barrier, the MFMAs of slab t run, then slab t + 1 is split and written to the
// other stage (its last readers passed this slab's barrier).
//
// Budget per slab and wave (cycles of one SIMD; MFMA 16x16x32 bf16 = 16, a wave64 VALU op = 4):
//   MFMA   4 x 4 pairs x 3 products = 48 MFMAs                                             = 768 cycles
//   VALU   8 float4 per lane (4 of dY, 4 of x) = 16 value pairs x (1 v_cvt_pk_bf16_f32 [hi] + 2 shift / and [hi back to
//          f32] + 2 v_sub_f32 [or 1 v_pk_add_f32] + 1 v_cvt_pk_bf16_f32 [lo]) = 96 ops    = 384 cycles  (VALU : MFMA = 0.50)
//          plus ~24 ops of predicates and addresses
//   LDS    16 ds_write_b64, 32 ds_read_b64_tr_b16 (2 per fragment, 16 fragments: hi and lo of 4 + 4)
//   HBM    2 x 16 KiB per workgroup and slab for 2 x 128 x 128 x 32 x 3 MFMA-flops
// The same ratio as the forward kernel with both operands converted, because no value is converted twice.
//
// The reduction over M is cut into chunks; workgroup (chunk, tile) writes its f32 partial tile and the caller sums the
// chunks with anemoi_col_sum (ops.weight_grad_split), as ops.weight_grad does for the bf16 TN kernel: no atomics, the
// result is the same bits on every run.  The bias gradient is NOT computed here: it is an exact f32 sum, which
// anemoi_col_sum over dY gives in one pass of N * M * 4 bytes; riding on the dY panel would mean a fourth, f32, use of
// the staged registers in a kernel whose VALU is already half of its MFMA time.
//
// MFMAs and LDS reads are compiler builtins: the compiler owns their wait states and counters (tools/isa_hazard_audit.py
// checks the listing).
#include "common.hpp"
#include "trail.hpp"

namespace anemoi {
namespace wgs {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) short s16x4_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;

constexpr int TILE = 128;                 // output tile: 128 dY columns x 128 x columns
constexpr int ROWS = 32;                  // reduction rows per slab = one MFMA k-step
constexpr int ROW_BYTES = TILE * 2;       // 256: one bf16 plane row
constexpr int PLANE = ROWS * ROW_BYTES;   // 8 KiB
constexpr int STAGE = 4 * PLANE;          // dY_hi, dY_lo, x_hi, x_lo
constexpr int CHUNK_MULTIPLE = ROWS;

__device__ __forceinline__ void split2(float a, float b, uint32_t& hi, uint32_t& lo) {
  hi = pack_bf16x2(a, b);
  lo = pack_bf16x2(a - __uint_as_float(hi << 16), b - __uint_as_float(hi & 0xffff0000u));
}

// OUT [chunks][out_stride] f32, chunk c holds the [N][K] partial of rows c * chunk_rows ... min(M, (c + 1) * chunk_rows)
__global__ __launch_bounds__(256) void weight_grad_split_kernel(const float* __restrict__ DY, int64_t ldy,
                                                                const float* __restrict__ X, int64_t ldx,
                                                                float* __restrict__ OUT, int64_t out_stride, int64_t M,
                                                                int N, int K, int chunk_rows, int kt_count,
                                                                int tiles_per_chunk) {
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];  // 64 KiB
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = blockIdx.x / tiles_per_chunk;
  const int t = blockIdx.x - c * tiles_per_chunk;
  const int n0 = (t / kt_count) * TILE, k0 = (t % kt_count) * TILE;
  const int64_t row0 = (int64_t)c * chunk_rows;
  const int64_t row_end = row0 + chunk_rows < M ? row0 + chunk_rows : M;
  const int nk = (int)((row_end - row0 + ROWS - 1) / ROWS);

  // ---- staging side: thread (lr = tid >> 5, c4 = tid & 31) moves columns 4 c4 .. 4 c4 + 3 of slab rows lr + 8 i
  const int c4 = tid & 31, lr = tid >> 5;
  const bool y_in = n0 + 4 * c4 < N, x_in = k0 + 4 * c4 < K;  // N % 4 == K % 4 == 0 (launcher): 4 columns in or out together
  const float* yp = DY + (row0 + lr) * ldy + n0 + 4 * c4;
  const float* xp = X + (row0 + lr) * ldx + k0 + 4 * c4;
  float4 yv[4], xv[4];
  auto fetch = [&](int kt) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = kt * ROWS + 8 * i;  // (+ lr: in yp / xp)
      const bool row_in = row0 + r + lr < row_end;
      yv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      xv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row_in && y_in) yv[i] = *reinterpret_cast<const float4*>(yp + (int64_t)r * ldy);
      if (row_in && x_in) xv[i] = *reinterpret_cast<const float4*>(xp + (int64_t)r * ldx);
    }
  };
  // byte offset of (row lr + 8 i, float4 c4) inside a plane: g(row) = (lr & 3) | (i & 1) << 2
  int woff[2];
#pragma unroll
  for (int v = 0; v < 2; ++v) woff[v] = lr * ROW_BYTES + ((((c4 >> 2) ^ ((lr & 3) | (v << 2))) << 5) | ((c4 & 3) << 3));
  auto put = [&](int buf) {
    char* base = smem + buf * STAGE;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int off = woff[i & 1] + 8 * i * ROW_BYTES;
      uint2 h, l;
      split2(yv[i].x, yv[i].y, h.x, l.x);
      split2(yv[i].z, yv[i].w, h.y, l.y);
      *reinterpret_cast<uint2*>(base + off) = h;
      *reinterpret_cast<uint2*>(base + PLANE + off) = l;
      split2(xv[i].x, xv[i].y, h.x, l.x);
      split2(xv[i].z, xv[i].w, h.y, l.y);
      *reinterpret_cast<uint2*>(base + 2 * PLANE + off) = h;
      *reinterpret_cast<uint2*>(base + 3 * PLANE + off) = l;
    }
  };

  // ---- compute side.  Fragment f (16 columns) of a plane: the 16-lane group fq reads rows 8 fq + 4 h + mr
  //      (mr = (lane & 15) >> 2), 4 columns at 4 cq (cq = lane & 3), h = 0, 1; lane (fr, fq) then holds m = 8 fq .. 8 fq + 7
  //      of column 16 f + fr.
  const int wm = wid >> 1, wn = wid & 1;  // wm: dY column half (MFMA "B" side), wn: x column half ("A" side)
  const int fr = lane & 15, fq = lane >> 4;
  const int mr = fr >> 2, cq = fr & 3;
  const int gl = mr | ((fq & 1) << 2);
  const int rbase = (8 * fq + mr) * ROW_BYTES + cq * 8;
  int ra[4], rb[4];
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    ra[f] = 2 * PLANE + rbase + (((4 * wn + f) ^ gl) << 5);
    rb[f] = rbase + (((4 * wm + f) ^ gl) << 5);
  }
  auto ld_frag = [&](int off) {
    const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(smem + off));
    const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) s16x4_t*)(smem + off + 4 * ROW_BYTES));
    return __builtin_bit_cast(bf16x8_t, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
  };

  f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  fetch(0);
  put(0);
  for (int kt = 0; kt < nk; ++kt) {
    const bool more = kt + 1 < nk;
    if (more) fetch(kt + 1);
    __syncthreads();  // stage kt & 1 is complete; every wave has finished reading the other one (slab kt - 1)
    const int sb = (kt & 1) * STAGE;
    bf16x8_t xh[4], xl[4], yh[4], yl[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      yh[f] = ld_frag(sb + rb[f]);
      yl[f] = ld_frag(sb + PLANE + rb[f]);
      xh[f] = ld_frag(sb + ra[f]);
      xl[f] = ld_frag(sb + PLANE + ra[f]);
    }
    // the two correction products first, the leading one last; each pass touches all 16 accumulators before any is reused
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xl[i], yh[j], acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh[i], yl[j], acc[i][j], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh[i], yh[j], acc[i][j], 0, 0, 0);
    if (more) put((kt + 1) & 1);
  }

  // ---- epilogue: lane (fr, fq) holds, for dY column n = n0 + 64 wm + 16 j + fr, the x columns k0 + 64 wn + 16 i + 4 fq + 0..3
  float* out = OUT + (int64_t)c * out_stride;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = n0 + 64 * wm + 16 * j + fr;
    if (n >= N) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = k0 + 64 * wn + 16 * i + 4 * fq;
      if (k < K)
        *reinterpret_cast<float4*>(out + (int64_t)n * K + k) = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
    }
  }
}

}  // namespace wgs
}  // namespace anemoi

using namespace anemoi;

extern "C" int anemoi_weight_grad_split(const float* dy, int64_t ldy, const float* x, int64_t ldx, float* partial,
                                        int64_t partial_stride, int64_t M, int N, int K, int chunk_rows,
                                        anemoi_stream_t stream) {
  ANEMOI_REQUIRE(partial != nullptr && (M == 0 || (dy != nullptr && x != nullptr)), ANEMOI_ERR_INVALID,
                 "anemoi_weight_grad_split: null pointer");
  ANEMOI_REQUIRE(M >= 0 && N > 0 && K > 0, ANEMOI_ERR_INVALID, "anemoi_weight_grad_split: bad shape M=%lld N=%d K=%d",
                 (long long)M, N, K);
  ANEMOI_REQUIRE(ldy >= N && ldx >= K, ANEMOI_ERR_INVALID, "anemoi_weight_grad_split: leading dimension below the width");
  ANEMOI_REQUIRE(N % 4 == 0 && K % 4 == 0, ANEMOI_ERR_INVALID,
                 "anemoi_weight_grad_split: N=%d and K=%d must be multiples of 4 (16-byte column groups)", N, K);
  ANEMOI_REQUIRE(ldy % 4 == 0 && ldx % 4 == 0 && (uintptr_t)dy % 16 == 0 && (uintptr_t)x % 16 == 0 &&
                     (uintptr_t)partial % 16 == 0,
                 ANEMOI_ERR_INVALID, "anemoi_weight_grad_split: operands 16-byte aligned, row pitches multiples of 4");
  ANEMOI_REQUIRE(chunk_rows > 0 && chunk_rows % wgs::CHUNK_MULTIPLE == 0, ANEMOI_ERR_INVALID,
                 "anemoi_weight_grad_split: chunk_rows=%d must be a positive multiple of %d", chunk_rows, wgs::CHUNK_MULTIPLE);
  ANEMOI_REQUIRE(partial_stride >= (int64_t)N * K && partial_stride % 4 == 0, ANEMOI_ERR_INVALID,
                 "anemoi_weight_grad_split: partial_stride must cover N * K floats and be a multiple of 4");
  if (M == 0) {  // an empty reduction: zeros, no launch
    if (hipMemsetAsync(partial, 0, (size_t)N * K * 4, as_stream(stream)) != hipSuccess)
      return fail(ANEMOI_ERR_LAUNCH, "anemoi_weight_grad_split: hipMemsetAsync failed");
    return ANEMOI_OK;
  }
  const int64_t chunks = (M + chunk_rows - 1) / chunk_rows;
  const int64_t nt = (N + wgs::TILE - 1) / wgs::TILE, kt = (K + wgs::TILE - 1) / wgs::TILE;
  ANEMOI_REQUIRE(nt * kt < ((int64_t)1 << 31) && chunks * nt * kt < ((int64_t)1 << 31), ANEMOI_ERR_UNSUPPORTED,
                 "anemoi_weight_grad_split: grid too large");
  hipLaunchKernelGGL(wgs::weight_grad_split_kernel, dim3((unsigned)(chunks * nt * kt)), dim3(256), 0, as_stream(stream), dy,
                     ldy, x, ldx, partial, partial_stride, M, N, K, chunk_rows, (int)kt, (int)(nt * kt));
  return trail::note(check_launch("anemoi_weight_grad_split"), "anemoi_weight_grad_split", "partial", ANEMOI_F32, partial,
                     partial_stride, chunks, (int64_t)N * K, as_stream(stream));
}
