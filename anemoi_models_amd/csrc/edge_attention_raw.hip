// Folded GraphTransformer edge phase whose SOURCES ARE RAW ROWS (bf16, 16 heads, gfx950).
//
// The encoder's sources enter their mapper block as the K_s raw feature columns x_j they are embedded from; k_j and v_j
// are linear in them (embedding and layer_norm1 folded into the k|v weights, runtime.fold_embedded_layer_norm):
//     k_j,h = rstd_j A_k,h x_j + b_k,h          v_j,h = rstd_j A_v,h x_j + b_v,h          (A_h: D x K_s)
// so both products move to the destination side, where there are 13 x fewer rows:
//     q_i,h . k_j,h          = rstd_j (qt_i,h . x_j) + q_i,h . b_k,h          qt_i,h = A_k,h^T q_i,h   (K_s values)
//     sum_j alpha_ij v_j,h   = A_v,h g_i,h + b_v,h sum_j alpha_ij             g_i,h  = sum_j alpha_ij rstd_j x_j
// q . b_k is the same for every in-edge of (i, h): the segment softmax subtracts the segment maximum, so it drops out
// of alpha exactly and is never formed.  The kernel gathers 2 K_s-byte raw rows instead of 4 C-byte k|v rows, reads qt
// [n_dst, 16 K_s] and writes g (same shape; column `sum_col` of every head, a zero column of x, carries sum_j alpha_ij
// so that b_v rides in the following product as one more weight column) and t~ (the lin_edge fold, as the other folded
// kernels).  The lin_edge terms u . a and sum alpha a are those of gt_edge_attention_folded_kernel.
//
// One wave per destination, 16 in-edges per step, heads on the MFMA column:
//     S^T [16 edges x 16 heads]  = X [16 x K_s] Qt^T [K_s x 16]          K_s / 32  v_mfma_f32_16x16x32_bf16
//         lane l: A = 16 bytes of the row of edge l & 15 (the gather itself), B = 16 bytes of qt of head l & 15;
//         result: edges 4 (l >> 4) .. + 3 of head l & 15 -- the segment softmax of a head is lane-local but for two
//         cross-lane maxima per step and two sums per destination;
//     G^T [K_s x 16 heads]      += X^T [K_s x 16 edges] P^T [16 x 16]     K_s / 16  v_mfma_f32_16x16x16_bf16
//         B = the lane's own four alpha rstd (bf16), A = X^T out of the wave's LDS image of the gathered rows through
//         ds_read_b64_tr_b16; result: 4 consecutive channels of head l & 15, so the online rescale and the final
//         normalisation use the lane's own max / sum.
// No atomics, fixed summation order: run-to-run bit-identical.  Tail edges of a step repeat the segment's last edge with
// weight 0 (every lane keeps a valid address: the transposing read needs EXEC all ones).
#include <cmath>

#include "common.hpp"
#include "trail.hpp"

namespace anemoi {

typedef __attribute__((ext_vector_type(8))) __bf16 rbf16x8_t;
typedef __attribute__((ext_vector_type(4))) short rs16x4_t;
typedef __attribute__((ext_vector_type(4))) float rf32x4_t;
typedef uint32_t ru32x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t ru32x2_t __attribute__((ext_vector_type(2)));

struct EdgeRawParams {
  const bf16_t* qt;
  const bf16_t* x;
  const float* stats;  // [n_src, 2]: {rstd, -mean rstd} of LayerNorm(emb(x)); only rstd is used (the mean is folded out)
  const bf16_t* u;
  bf16_t* g;
  bf16_t* t;
  int64_t ldqt, ldx, ldu, ldg, ldt;
  int64_t n_dst;
  int sum_col;  // column of every head's g that receives sum_j alpha_ij, or -1
  float scale;
};

template <int KS, int UP>
__global__ __launch_bounds__(256, (KS == 256 || UP > 8) ? 2 : 3) void gt_edge_attention_raw_kernel(const EdgeRawParams p,
                                                                    const float* __restrict__ attr_,
                                                                    const int32_t* __restrict__ rowptr_,
                                                                    const int32_t* __restrict__ col_) {
  constexpr int T = KS / 32;            // reduction steps of the score product
  constexpr int NT = KS / 16;           // 16-channel tiles of the aggregate
  constexpr int PITCH = KS * 2 + 16;    // bytes per row of the LDS image (16 rows per wave)
  __shared__ __attribute__((aligned(16))) unsigned char image[4][16 * PITCH];

  const int lane = threadIdx.x & 63;
  const int wib = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int r16 = lane & 15, g4 = lane >> 4;
  // block b runs on XCD b % 8: XCD x walks the contiguous destination range [x N / 8, (x + 1) N / 8), as the other edge
  // kernels do (shared source rows are re-used from that XCD's L2)
  const int xcd = blockIdx.x & 7;
  const int64_t n0 = p.n_dst * xcd / 8, n1 = p.n_dst * (xcd + 1) / 8;
  const int64_t node = n0 + (int64_t)(blockIdx.x >> 3) * 4 + wib;
  if (node >= n1) return;  // (wave-uniform)
  unsigned char* tile = image[wib];

  const int e_begin = __builtin_amdgcn_readfirstlane(rowptr_[node]);
  const int e_end = __builtin_amdgcn_readfirstlane(rowptr_[node + 1]);

  rbf16x8_t qb[T];
  {
    const bf16_t* qrow = p.qt + node * p.ldqt + r16 * KS + g4 * 8;
#pragma unroll
    for (int t = 0; t < T; ++t) qb[t] = __builtin_bit_cast(rbf16x8_t, *reinterpret_cast<const ru32x4_t*>(qrow + t * 32));
  }
  float u[UP];
  {
    const uint32_t* uw = reinterpret_cast<const uint32_t*>(p.u + node * p.ldu + r16 * UP);
#pragma unroll
    for (int a = 0; a < UP / 2; ++a) {
      const uint32_t w = uw[a];
      u[2 * a] = __uint_as_float(w << 16);
      u[2 * a + 1] = __uint_as_float(w & 0xffff0000u);
    }
  }

  float m = -INFINITY, lsum = 0.f;
  float tacc[UP];
  rf32x4_t acc[NT];
#pragma unroll
  for (int a = 0; a < UP; ++a) tacc[a] = 0.f;
#pragma unroll
  for (int n = 0; n < NT; ++n) acc[n] = rf32x4_t{0.f, 0.f, 0.f, 0.f};

  for (int e0 = e_begin; e0 < e_end; e0 += 16) {
    // the gather: lane l takes 16 bytes of the row of edge e0 + (l & 15) per reduction step
    ru32x4_t xa[T];
    {
      const int ea = min(e0 + r16, e_end - 1);
      const bf16_t* xrow = p.x + (int64_t)col_[ea] * p.ldx + g4 * 8;
#pragma unroll
      for (int t = 0; t < T; ++t) xa[t] = *reinterpret_cast<const ru32x4_t*>(xrow + t * 32);
    }
    // the four edges whose scores land in this lane: rstd of their sources, their attribute rows
    float rs[4], at[4][UP];
    bool valid[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int eq = e0 + g4 * 4 + q;
      valid[q] = eq < e_end;
      const int ec = valid[q] ? eq : e_end - 1;
      rs[q] = p.stats[2 * (int64_t)col_[ec]];
      const float4* ap = reinterpret_cast<const float4*>(attr_ + (int64_t)ec * UP);
#pragma unroll
      for (int a = 0; a < UP / 4; ++a) {
        const float4 v = ap[a];
        at[q][4 * a] = v.x; at[q][4 * a + 1] = v.y; at[q][4 * a + 2] = v.z; at[q][4 * a + 3] = v.w;
      }
    }

    rf32x4_t s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < T; ++t)
      s4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(rbf16x8_t, xa[t]), qb[t], s4, 0, 0, 0);
    // the rows go to the wave's LDS image as they are (row = edge): the aggregate reads them back transposed
#pragma unroll
    for (int t = 0; t < T; ++t) *reinterpret_cast<ru32x4_t*>(tile + r16 * PITCH + t * 64 + g4 * 16) = xa[t];

    float s[4], cmax = -INFINITY;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float ua = 0.f;
#pragma unroll
      for (int a = 0; a < UP; ++a) ua = fmaf(u[a], at[q][a], ua);
      s[q] = valid[q] ? fmaf(rs[q], s4[q], ua) * p.scale : -INFINITY;
      cmax = fmaxf(cmax, s[q]);
    }
    cmax = fmaxf(cmax, __shfl_xor(cmax, 16, 64));
    cmax = fmaxf(cmax, __shfl_xor(cmax, 32, 64));
    const float mb = fmaxf(m, cmax);  // finite: the step holds at least one edge
    const float corr = __expf(m - mb);
    float pe[4], psum = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      pe[q] = valid[q] ? __expf(s[q] - mb) : 0.f;
      psum += pe[q];
    }
    lsum = fmaf(lsum, corr, psum);
#pragma unroll
    for (int a = 0; a < UP; ++a) {
      float ta = tacc[a] * corr;
#pragma unroll
      for (int q = 0; q < 4; ++q) ta = fmaf(pe[q], at[q][a], ta);
      tacc[a] = ta;
    }
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] *= corr;
    m = mb;
    const rs16x4_t pb = __builtin_bit_cast(
        rs16x4_t, ru32x2_t{pack_bf16x2(pe[0] * rs[0], pe[1] * rs[1]), pack_bf16x2(pe[2] * rs[2], pe[3] * rs[3])});

    // (LDS instructions of one wave execute in order: the image written above is complete when the reads below run)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // lane 4 q + c of the 16-lane group g4 names row 4 g4 + q, columns 4 c .. 4 c + 3 of the tile; lane i receives
    // column i of the group's four rows: X^T [channel 16 n + i][edges 4 g4 .. + 3], the A operand of the lane
    const int tr_off = (g4 * 4 + (r16 >> 2)) * PITCH + (r16 & 3) * 8;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const rs16x4_t xt = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (__attribute__((address_space(3))) rs16x4_t*)(tile + tr_off + n * 32));
      acc[n] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(xt, pb, acc[n], 0, 0, 0);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }

  // the four lane groups hold partial sums over their edges
  lsum += __shfl_xor(lsum, 16, 64);
  lsum += __shfl_xor(lsum, 32, 64);
  const float inv = 1.0f / (lsum + 1e-16f);
  const float asum = lsum * inv;  // sum_j alpha_ij: 1, or 0 for a destination without in-edges
#pragma unroll
  for (int a = 0; a < UP; ++a) {
    float ta = tacc[a];
    ta += __shfl_xor(ta, 16, 64);
    ta += __shfl_xor(ta, 32, 64);
    tacc[a] = ta * inv;
  }
  if (g4 == 0) {
    uint32_t* tw = reinterpret_cast<uint32_t*>(p.t + node * p.ldt + r16 * UP);
#pragma unroll
    for (int a = 0; a < UP / 2; ++a) tw[a] = pack_bf16x2(tacc[2 * a], tacc[2 * a + 1]);
  }
  bf16_t* grow = p.g + node * p.ldg + r16 * KS + g4 * 4;
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (n * 16 + g4 * 4 + j == p.sum_col) ? asum : acc[n][j] * inv;
    *reinterpret_cast<ru32x2_t*>(grow + n * 16) = ru32x2_t{pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3])};
  }
}

template <int KS, int UP>
static void launch_raw(const EdgeRawParams& p, const float* attr, const int32_t* rowptr, const int32_t* col,
                       hipStream_t st) {
  const int64_t per_xcd = (p.n_dst + 7) / 8;  // (the longest of the eight destination ranges)
  const int64_t bpx = (per_xcd + 3) / 4;
  hipLaunchKernelGGL((gt_edge_attention_raw_kernel<KS, UP>), dim3((unsigned)(8 * bpx)), dim3(256), 0, st, p, attr, rowptr,
                     col);
}

template <int KS>
static bool dispatch_raw(const EdgeRawParams& p, int up, const float* attr, const int32_t* rowptr, const int32_t* col,
                         hipStream_t st) {
  switch (up) {
    case 4: launch_raw<KS, 4>(p, attr, rowptr, col, st); return true;
    case 8: launch_raw<KS, 8>(p, attr, rowptr, col, st); return true;
    case 12: launch_raw<KS, 12>(p, attr, rowptr, col, st); return true;
    case 16: launch_raw<KS, 16>(p, attr, rowptr, col, st); return true;
    default: return false;
  }
}

}  // namespace anemoi

extern "C" int anemoi_gt_edge_attention_raw(const void* qt, int64_t ldqt, const void* x, int64_t ldx,
                                            const float* src_stats, const void* u, int64_t ldu,
                                            const float* edge_attr, int up, const int32_t* rowptr, const int32_t* col,
                                            void* g, int64_t ldg, void* t, int64_t ldt, int64_t n_dst, int H, int Ks,
                                            int D, int sum_col, anemoi_stream_t stream) {
  using namespace anemoi;
  ANEMOI_REQUIRE(qt && x && src_stats && u && g && t && rowptr, ANEMOI_ERR_INVALID,
                 "anemoi_gt_edge_attention_raw: null pointer");
  ANEMOI_REQUIRE(n_dst >= 0 && D > 0 && sum_col >= -1 && sum_col < Ks, ANEMOI_ERR_INVALID,
                 "anemoi_gt_edge_attention_raw: bad argument");
  ANEMOI_REQUIRE(H == 16 && (Ks == 64 || Ks == 128 || Ks == 256) && up >= 4 && up <= 16 && up % 4 == 0, ANEMOI_ERR_UNSUPPORTED,
                 "anemoi_gt_edge_attention_raw: needs 16 heads, 64, 128 or 256 raw columns, up in {4, 8, 12, 16} (H=%d, Ks=%d, up=%d)",
                 H, Ks, up);
  ANEMOI_REQUIRE(ldqt >= (int64_t)H * Ks && ldg >= (int64_t)H * Ks && ldx >= Ks && ldu >= (int64_t)H * up &&
                     ldt >= (int64_t)H * up,
                 ANEMOI_ERR_INVALID, "anemoi_gt_edge_attention_raw: leading dimension too small");
  if (n_dst == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(col != nullptr && edge_attr != nullptr, ANEMOI_ERR_INVALID,
                 "anemoi_gt_edge_attention_raw: null edge arrays");
  const bool aligned = (uintptr_t)qt % 16 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)g % 16 == 0 &&
                       (uintptr_t)u % 8 == 0 && (uintptr_t)t % 8 == 0 && (uintptr_t)edge_attr % 16 == 0 &&
                       ldqt % 8 == 0 && ldx % 8 == 0 && ldg % 8 == 0 && ldu % 4 == 0 && ldt % 4 == 0;
  ANEMOI_REQUIRE(aligned, ANEMOI_ERR_UNSUPPORTED, "anemoi_gt_edge_attention_raw: operands must be 16-byte aligned");
  EdgeRawParams p;
  p.qt = static_cast<const bf16_t*>(qt); p.x = static_cast<const bf16_t*>(x); p.stats = src_stats;
  p.u = static_cast<const bf16_t*>(u); p.g = static_cast<bf16_t*>(g); p.t = static_cast<bf16_t*>(t);
  p.ldqt = ldqt; p.ldx = ldx; p.ldu = ldu; p.ldg = ldg; p.ldt = ldt;
  p.n_dst = n_dst; p.sum_col = sum_col;
  p.scale = 1.0f / sqrtf((float)D);
  const bool ok = Ks == 256   ? dispatch_raw<256>(p, up, edge_attr, rowptr, col, as_stream(stream))
                  : Ks == 128 ? dispatch_raw<128>(p, up, edge_attr, rowptr, col, as_stream(stream))
                              : dispatch_raw<64>(p, up, edge_attr, rowptr, col, as_stream(stream));
  ANEMOI_REQUIRE(ok, ANEMOI_ERR_UNSUPPORTED, "anemoi_gt_edge_attention_raw: up=%d", up);
  int rc = trail::note(check_launch("anemoi_gt_edge_attention_raw"), "anemoi_gt_edge_attention_raw", "out", ANEMOI_BF16, g, ldg,
                       n_dst, (int64_t)H * Ks, as_stream(stream));
  return trail::note(rc, "anemoi_gt_edge_attention_raw", "t_out", ANEMOI_BF16, t, ldt, n_dst, (int64_t)H * up, as_stream(stream));
}
