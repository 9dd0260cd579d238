// MXFP8 inference route: the quantiser (optionally behind a LayerNorm) and the Linear on the
// block-scaled MFMA v_mfma_scale_f32_16x16x128_f8f6f4.  Number format and layout: include/anemoi_amd.h ("MXFP8").
#include "common.hpp"
#include "trail.hpp"

namespace anemoi {
namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;

// Block exponent e = floor(log2(amax)) - 8 clamped to [-127, 127]; amax = 0 or an f32 subnormal gives -127 (scale byte 0).
__device__ __forceinline__ int mx_block_exp(float amax) {
  const int eb = (int)((__float_as_uint(amax) >> 23) & 0xffu);
  return max(eb - 127 - 8, -127);
}

// 2^-e as an f32 (exact for e in [-127, 126], which covers every finite amax).
__device__ __forceinline__ float mx_inv_scale(int e) { return __uint_as_float((uint32_t)(127 - e) << 23); }

// f32 -> e4m3fn, round to nearest-even, |f| > 448 saturates to 448 (the scaled block never carries a NaN or an overflow).
__device__ __forceinline__ uint32_t f32_to_e4m3(float f) {
  const uint32_t sign = (__float_as_uint(f) >> 24) & 0x80u;
  const float a = fminf(fabsf(f), 448.0f);
  uint32_t code;
  if (a < 0.015625f) {  // below 2^-6: subnormal codes m 2^-9, m = 0..8 (8 is the smallest normal, code 0x08)
    code = (uint32_t)__builtin_rintf(a * 512.0f);
  } else {  // keep 3 mantissa bits, round to nearest-even at bit 20; a carry moves into the exponent as it should
    uint32_t b = __float_as_uint(a);
    b += 0x7ffffu + ((b >> 20) & 1u);
    code = (((b >> 23) - 120u) << 3) | ((b >> 20) & 7u);
  }
  return sign | code;
}

__device__ __forceinline__ uint32_t pack_e4m3x4(const float* v, float inv) {
  return f32_to_e4m3(v[0] * inv) | f32_to_e4m3(v[1] * inv) << 8 | f32_to_e4m3(v[2] * inv) << 16 |
         f32_to_e4m3(v[3] * inv) << 24;
}

// ------------------------------------------------------------------------------------------------ quantiser
// One wave per row, four rows per block.  Lane l holds elements [512 c + 8 l, +8) of chunk c, so a 32-element block is the
// aligned quad of lanes 4b .. 4b+3 and its amax is two DPP steps.  The row stays in registers between the LayerNorm
// statistics and the quantisation: it is read once.
template <typename T, int NCH>
__global__ __launch_bounds__(256) void mx_quantize_kernel(const T* __restrict__ x, int64_t ldx,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float eps,
                                                          uint8_t* __restrict__ q, int64_t ldq, uint8_t* __restrict__ s,
                                                          int64_t lds, int64_t rows, int K, int Kp, bool vec) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;  // wave-uniform: the DPP reductions below see all 64 lanes
  const T* xr = x + row * ldx;
  float v[NCH][8];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col0 = c * 512 + lane * 8;
    if (vec && col0 + 8 <= K) {
      VecIO<T, 8>::load(xr + col0, v[c]);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[c][i] = col0 + i < K ? Elem<T>::load(xr + col0 + i) : 0.f;
    }
  }
  if (gamma != nullptr) {
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int i = 0; i < 8; ++i) sum += v[c][i];
    const float mean = wave_sum(sum) / (float)K;
    float sq = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float d = c * 512 + lane * 8 + i < K ? v[c][i] - mean : 0.f;
        sq = fmaf(d, d, sq);
      }
    const float rstd = rsqrtf(wave_sum(sq) / (float)K + eps);
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int col = c * 512 + lane * 8 + i;
        v[c][i] = col < K ? fmaf((v[c][i] - mean) * rstd, gamma[col], beta[col]) : 0.f;
      }
  }
  uint8_t* qr = q + row * ldq;
  uint8_t* sr = s + row * lds;
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int col0 = c * 512 + lane * 8;
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(v[c][i]));
    amax = fmaxf(amax, dpp_f32<0xB1>(amax));  // lane ^ 1
    amax = fmaxf(amax, dpp_f32<0x4E>(amax));  // lane ^ 2
    const int e = mx_block_exp(amax);
    const float inv = mx_inv_scale(e);
    if (col0 < Kp) {  // Kp is a multiple of 128: a quad is either wholly inside or wholly outside
      *reinterpret_cast<uint2*>(qr + col0) = make_uint2(pack_e4m3x4(v[c], inv), pack_e4m3x4(v[c] + 4, inv));
      if ((lane & 3) == 0) sr[col0 >> 5] = (uint8_t)(e + 127);
    }
  }
}

// ------------------------------------------------------------------------------------------------ Linear
// Four waves in 2 x 2, each owning (16 WM) x (16 WN) outputs as WM x WN scaled MFMAs of 16 x 16 x 128: the block tile is
// (32 WM) x (32 WN).  Per 128-byte K-slab the block stages the A and B rows (rows padded to 144 B in LDS) and one u32 of
// four scale bytes per row; the next slab's global loads are in flight while the current one is multiplied.
constexpr int MX_PITCH = 144;  // LDS bytes per staged row (128 + 16: spreads 16 rows over the banks)

template <int WM, int WN>
constexpr int mx_lds_bytes() {  // two staging buffers of (BM + BN) rows and their scale words
  return 2 * (32 * WM + 32 * WN) * (MX_PITCH + 4);
}

__device__ __forceinline__ uint4 ldg16(const uint8_t* p) { return *reinterpret_cast<const uint4*>(p); }

template <int WM, int WN>
__global__ __launch_bounds__(256) void linear_mx_kernel(const uint8_t* __restrict__ xq, int64_t ldxq,
                                                        const uint8_t* __restrict__ xs, int64_t ldxs,
                                                        const uint8_t* __restrict__ wq, const uint8_t* __restrict__ ws,
                                                        const float* __restrict__ bias,
                                                        const bf16_t* __restrict__ residual, int64_t ldr, int out_mx,
                                                        uint8_t* __restrict__ y, int64_t ldy, uint8_t* __restrict__ ys,
                                                        int64_t ldys, int64_t M, int N, int K, int act) {
  constexpr int BM = 32 * WM, BN = 32 * WN;
  constexpr int EPI_ROWS = 8192 / BN;   // epilogue chunk: 256 threads x one 32-column block each
  constexpr int EPI_PITCH = BN + 4;     // f32 per epilogue row
  static_assert(EPI_ROWS * EPI_PITCH * 4 <= (BM + BN) * MX_PITCH, "epilogue chunk must fit the staging buffer");
  extern __shared__ __attribute__((aligned(16))) uint8_t smem_all[];
  constexpr int STAGE = (BM + BN) * (MX_PITCH + 4);  // bytes of one staging buffer: rows, then [BM + BN] scale words
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int64_t m0 = (int64_t)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const int nk = K / 128;
  const int64_t ldws = K / 32;

  uint4 ra[WM], rb[WN];
  uint32_t rs[(BM + BN + 255) / 256];
  auto load = [&](int ks) {
#pragma unroll
    for (int i = 0; i < WM; ++i) {
      const int c = tid + 256 * i, r = c >> 3, o = (c & 7) * 16;
      ra[i] = m0 + r < M ? ldg16(xq + (m0 + r) * ldxq + ks * 128 + o) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < WN; ++i) {
      const int c = tid + 256 * i, r = c >> 3, o = (c & 7) * 16;
      rb[i] = n0 + r < N ? ldg16(wq + (int64_t)(n0 + r) * K + ks * 128 + o) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < (BM + BN + 255) / 256; ++i) {
      const int r = tid + 256 * i;
      if (r < BM) {
        rs[i] = m0 + r < M ? *reinterpret_cast<const uint32_t*>(xs + (m0 + r) * ldxs + ks * 4) : 0u;
      } else if (r < BM + BN) {
        rs[i] = n0 + r - BM < N ? *reinterpret_cast<const uint32_t*>(ws + (int64_t)(n0 + r - BM) * ldws + ks * 4) : 0u;
      }
    }
  };

  f32x4_t acc[WM][WN];
#pragma unroll
  for (int i = 0; i < WM; ++i)
#pragma unroll
    for (int j = 0; j < WN; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // lane l of a 16-row operand: row l & 15, bytes [16 g, +16) and [64 + 16 g, +16) of the slab, scale byte g (g = l >> 4)
  const int g = lane >> 4, lr = lane & 15;
  load(0);
  for (int ks = 0; ks < nk; ++ks) {
    // slab ks goes to buffer ks & 1: the last reads of that buffer (slab ks - 2) are behind the barrier of slab ks - 1
    uint8_t* smem = smem_all + (ks & 1) * STAGE;
    uint32_t* s_sc = reinterpret_cast<uint32_t*>(smem + (BM + BN) * MX_PITCH);
#pragma unroll
    for (int i = 0; i < WM; ++i) {
      const int c = tid + 256 * i;
      *reinterpret_cast<uint4*>(smem + (c >> 3) * MX_PITCH + (c & 7) * 16) = ra[i];
    }
#pragma unroll
    for (int i = 0; i < WN; ++i) {
      const int c = tid + 256 * i;
      *reinterpret_cast<uint4*>(smem + (BM + (c >> 3)) * MX_PITCH + (c & 7) * 16) = rb[i];
    }
#pragma unroll
    for (int i = 0; i < (BM + BN + 255) / 256; ++i)
      if (tid + 256 * i < BM + BN) s_sc[tid + 256 * i] = rs[i];
    __syncthreads();
    if (ks + 1 < nk) load(ks + 1);
    i32x8_t bf[WN];
    int sbj[WN];
#pragma unroll
    for (int j = 0; j < WN; ++j) {
      const int r = BM + wn * 16 * WN + j * 16 + lr;
      const uint4 lo = *reinterpret_cast<const uint4*>(smem + r * MX_PITCH + 16 * g);
      const uint4 hi = *reinterpret_cast<const uint4*>(smem + r * MX_PITCH + 64 + 16 * g);
      bf[j] = i32x8_t{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
      sbj[j] = (int)(s_sc[r] >> (8 * g));
    }
#pragma unroll
    for (int i = 0; i < WM; ++i) {
      const int r = wm * 16 * WM + i * 16 + lr;
      const uint4 lo = *reinterpret_cast<const uint4*>(smem + r * MX_PITCH + 16 * g);
      const uint4 hi = *reinterpret_cast<const uint4*>(smem + r * MX_PITCH + 64 + 16 * g);
      const i32x8_t af = {(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
      const int sai = (int)(s_sc[r] >> (8 * g));
#pragma unroll
      for (int j = 0; j < WN; ++j)  // op_sel 0: the low byte of each scale operand
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af, bf[j], acc[i][j], 0, 0, 0, sai, 0, sbj[j]);
    }
  }
  __syncthreads();  // every wave is done with both buffers before the epilogue reuses them

  // Epilogue in chunks of EPI_ROWS rows through LDS: thread t owns row t / (BN / 32) of the chunk and the 32-column block
  // t % (BN / 32), which is one MXFP8 scale block of the output.
  float* cs = reinterpret_cast<float*>(smem_all);
  const int er = tid / (BN / 32), eb = tid % (BN / 32);
  const int Np = (N + 127) / 128 * 128;
  for (int chunk = 0; chunk < BM / EPI_ROWS; ++chunk) {
#pragma unroll
    for (int i = 0; i < WM; ++i) {
      const int row = wm * 16 * WM + i * 16;  // first row of this wave's tile i
      if (row >= chunk * EPI_ROWS && row < (chunk + 1) * EPI_ROWS) {
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r)  // C/D: column lane & 15, row 4 (lane >> 4) + r
            cs[(row - chunk * EPI_ROWS + g * 4 + r) * EPI_PITCH + wn * 16 * WN + j * 16 + lr] = acc[i][j][r];
      }
    }
    __syncthreads();
    const int64_t m = m0 + chunk * EPI_ROWS + er;
    const int c0 = n0 + eb * 32;
    if (m < M && c0 < (out_mx ? Np : N)) {
      float v[32];
#pragma unroll
      for (int q8 = 0; q8 < 4; ++q8) {
        const int cq = c0 + q8 * 8;
        float res[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (residual != nullptr && cq < N) VecIO<bf16_t, 8>::load(residual + m * ldr + cq, res);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int col = cq + e;
          float t = cs[er * EPI_PITCH + eb * 32 + q8 * 8 + e];
          if (col < N) {
            if (bias != nullptr) t += bias[col];
            t = act_apply(t, act) + res[e];
          } else {
            t = 0.f;
          }
          v[q8 * 8 + e] = t;
        }
      }
      if (out_mx) {
        float amax = 0.f;
#pragma unroll
        for (int e = 0; e < 32; ++e) amax = fmaxf(amax, fabsf(v[e]));
        const int ex = mx_block_exp(amax);
        const float inv = mx_inv_scale(ex);
        uint8_t* yr = y + m * ldy + c0;
        *reinterpret_cast<uint4*>(yr) = make_uint4(pack_e4m3x4(v, inv), pack_e4m3x4(v + 4, inv),
                                                   pack_e4m3x4(v + 8, inv), pack_e4m3x4(v + 12, inv));
        *reinterpret_cast<uint4*>(yr + 16) = make_uint4(pack_e4m3x4(v + 16, inv), pack_e4m3x4(v + 20, inv),
                                                        pack_e4m3x4(v + 24, inv), pack_e4m3x4(v + 28, inv));
        ys[m * ldys + (c0 >> 5)] = (uint8_t)(ex + 127);
      } else {
        bf16_t* yr = reinterpret_cast<bf16_t*>(y) + m * ldy + c0;
#pragma unroll
        for (int q8 = 0; q8 < 4; ++q8) {
          if (c0 + q8 * 8 < N) {
            float t8[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) t8[e] = v[q8 * 8 + e];
            VecIO<bf16_t, 8>::store(yr + q8 * 8, t8);
          }
        }
      }
    }
    __syncthreads();
  }
}

template <int WM, int WN>
int launch_linear_mx(const uint8_t* xq, int64_t ldxq, const uint8_t* xs, int64_t ldxs, const uint8_t* wq,
                     const uint8_t* ws, const float* bias, const void* residual, int64_t ldr, int out_mx, void* y,
                     int64_t ldy, uint8_t* ys, int64_t ldys, int64_t M, int N, int K, int act, hipStream_t st) {
  static PerDeviceOnce raised;
  const int dev = raised.pending();
  if (dev >= 0) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(linear_mx_kernel<WM, WN>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, mx_lds_bytes<WM, WN>()) != hipSuccess)
      return fail(ANEMOI_ERR_LAUNCH, "anemoi_linear_mx: cannot raise the dynamic LDS limit to %d", mx_lds_bytes<WM, WN>());
    raised.done(dev);
  }
  constexpr int BM = 32 * WM, BN = 32 * WN, LDS = mx_lds_bytes<WM, WN>();
  const dim3 grid((unsigned)((M + BM - 1) / BM), (unsigned)((N + BN - 1) / BN)), block(256);
  hipLaunchKernelGGL((linear_mx_kernel<WM, WN>), grid, block, LDS, st, xq, ldxq, xs, ldxs, wq, ws,
                     bias, static_cast<const bf16_t*>(residual), ldr, out_mx, static_cast<uint8_t*>(y), ldy, ys, ldys, M,
                     N, K, act);
  return check_launch("anemoi_linear_mx");
}

}  // namespace
}  // namespace anemoi

using namespace anemoi;

extern "C" {

int anemoi_mx_quantize(int dtype, const void* x, int64_t ldx, const float* gamma, const float* beta, float eps,
                       uint8_t* q, int64_t ldq, uint8_t* s, int64_t lds, int64_t rows, int K, int Kp,
                       anemoi_stream_t stream) {
  ANEMOI_REQUIRE(x && q && s, ANEMOI_ERR_INVALID, "anemoi_mx_quantize: null pointer");
  ANEMOI_REQUIRE((gamma == nullptr) == (beta == nullptr), ANEMOI_ERR_INVALID,
                 "anemoi_mx_quantize: gamma and beta go together");
  ANEMOI_REQUIRE(dtype == ANEMOI_F32 || dtype == ANEMOI_BF16, ANEMOI_ERR_INVALID, "anemoi_mx_quantize: dtype %d", dtype);
  ANEMOI_REQUIRE(rows >= 0 && K > 0 && Kp >= K && ldx >= K, ANEMOI_ERR_INVALID,
                 "anemoi_mx_quantize: bad shape rows=%lld K=%d Kp=%d ldx=%lld", (long long)rows, K, Kp, (long long)ldx);
  ANEMOI_REQUIRE(Kp % 128 == 0, ANEMOI_ERR_UNSUPPORTED, "anemoi_mx_quantize: Kp=%d is not a multiple of 128", Kp);
  ANEMOI_REQUIRE(Kp <= 4096, ANEMOI_ERR_UNSUPPORTED, "anemoi_mx_quantize: Kp=%d > 4096", Kp);
  ANEMOI_REQUIRE(ldq >= Kp && ldq % 16 == 0 && (uintptr_t)q % 16 == 0 && lds >= Kp / 32, ANEMOI_ERR_INVALID,
                 "anemoi_mx_quantize: ldq=%lld must be a multiple of 16 and >= Kp, q 16-byte aligned, lds=%lld >= Kp/32",
                 (long long)ldq, (long long)lds);
  if (rows == 0) return ANEMOI_OK;
  const int esz = dtype == ANEMOI_F32 ? 4 : 2;
  const bool vec = (uintptr_t)x % 16 == 0 && (ldx * esz) % 16 == 0;
  const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  hipStream_t st = as_stream(stream);
#define MXQ_LAUNCH(T, NCH)                                                                                               \
  hipLaunchKernelGGL((mx_quantize_kernel<T, NCH>), grid, block, 0, st, static_cast<const T*>(x), ldx, gamma, beta, eps, \
                     q, ldq, s, lds, rows, K, Kp, vec)
#define MXQ_DISPATCH(T)               \
  if (Kp <= 512) MXQ_LAUNCH(T, 1);    \
  else if (Kp <= 1024) MXQ_LAUNCH(T, 2); \
  else if (Kp <= 2048) MXQ_LAUNCH(T, 4); \
  else MXQ_LAUNCH(T, 8)
  if (dtype == ANEMOI_F32) {
    MXQ_DISPATCH(float);
  } else {
    MXQ_DISPATCH(bf16_t);
  }
#undef MXQ_DISPATCH
#undef MXQ_LAUNCH
  int rc = trail::note(check_launch("anemoi_mx_quantize"), "anemoi_mx_quantize", "q", ANEMOI_U8, q, ldq, rows, Kp, st);
  return trail::note(rc, "anemoi_mx_quantize", "scales", ANEMOI_U8, s, lds, rows, Kp / 32, st);
}

int anemoi_linear_mx(const uint8_t* xq, int64_t ldxq, const uint8_t* xs, int64_t ldxs, const uint8_t* wq,
                     const uint8_t* ws, const float* bias, const void* residual, int64_t ldr, int out_mx, void* y,
                     int64_t ldy, uint8_t* ys, int64_t ldys, int64_t M, int N, int K, int act, anemoi_stream_t stream) {
  ANEMOI_REQUIRE(xq && xs && wq && ws && y && (!out_mx || ys), ANEMOI_ERR_INVALID, "anemoi_linear_mx: null pointer");
  ANEMOI_REQUIRE(M >= 0 && N > 0 && K > 0, ANEMOI_ERR_INVALID, "anemoi_linear_mx: bad shape M=%lld N=%d K=%d",
                 (long long)M, N, K);
  ANEMOI_REQUIRE(act >= ANEMOI_ACT_NONE && act <= ANEMOI_ACT_RELU, ANEMOI_ERR_INVALID, "anemoi_linear_mx: act %d", act);
  ANEMOI_REQUIRE(K % 128 == 0, ANEMOI_ERR_UNSUPPORTED, "anemoi_linear_mx: K=%d is not a multiple of 128", K);
  ANEMOI_REQUIRE(N % (out_mx ? 32 : 16) == 0, ANEMOI_ERR_UNSUPPORTED, "anemoi_linear_mx: N=%d is not a multiple of %d", N,
                 out_mx ? 32 : 16);
  const int Np = (N + 127) / 128 * 128;
  ANEMOI_REQUIRE(ldxq >= K && ldxq % 16 == 0 && ldxs >= K / 32 && ldxs % 4 == 0, ANEMOI_ERR_INVALID,
                 "anemoi_linear_mx: ldxq=%lld must be a multiple of 16 >= K, ldxs=%lld a multiple of 4 >= K/32",
                 (long long)ldxq, (long long)ldxs);
  ANEMOI_REQUIRE((uintptr_t)xq % 16 == 0 && (uintptr_t)wq % 16 == 0 && (uintptr_t)xs % 4 == 0 && (uintptr_t)ws % 4 == 0 &&
                     (uintptr_t)y % 16 == 0,
                 ANEMOI_ERR_INVALID, "anemoi_linear_mx: operands must be 16-byte (scales 4-byte) aligned");
  if (out_mx) {
    ANEMOI_REQUIRE(ldy >= Np && ldy % 16 == 0 && ldys >= Np / 32, ANEMOI_ERR_INVALID,
                   "anemoi_linear_mx: MXFP8 output needs ldy=%lld a multiple of 16 >= %d and ldys=%lld >= %d",
                   (long long)ldy, Np, (long long)ldys, Np / 32);
  } else {
    ANEMOI_REQUIRE(ldy >= N && ldy % 8 == 0, ANEMOI_ERR_INVALID,
                   "anemoi_linear_mx: ldy=%lld must be a multiple of 8 and >= N", (long long)ldy);
  }
  ANEMOI_REQUIRE(residual == nullptr || (ldr >= N && ldr % 8 == 0 && (uintptr_t)residual % 16 == 0), ANEMOI_ERR_INVALID,
                 "anemoi_linear_mx: residual needs ldr=%lld a multiple of 8 >= N and 16-byte alignment", (long long)ldr);
  if (M == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE((M + 127) / 128 < ((int64_t)1 << 31), ANEMOI_ERR_UNSUPPORTED, "anemoi_linear_mx: M too large");
  // 128 x 128 block tiles (four waves of 64 x 64); the larger wave tiles measured slower (profiles/r07_mxfp8.md)
  int rc = launch_linear_mx<4, 4>(xq, ldxq, xs, ldxs, wq, ws, bias, residual, ldr, out_mx, y, ldy, ys, ldys, M, N, K, act,
                                  as_stream(stream));
  if (!out_mx) return trail::note(rc, "anemoi_linear_mx", "out", ANEMOI_BF16, y, ldy, M, N, as_stream(stream));
  rc = trail::note(rc, "anemoi_linear_mx", "out", ANEMOI_U8, y, ldy, M, Np, as_stream(stream));
  return trail::note(rc, "anemoi_linear_mx", "scales", ANEMOI_U8, ys, ldys, M, Np / 32, as_stream(stream));
}

}  // extern "C"
