// Remappers (preprocessing/monomapper.py, multimapper.py) folded into predict_step's first and last steps: the input assembly
// reads a raw state of V_raw columns and writes the V_int internal columns the model sees, the prognostic residual adds the
// remapped last state, and one pass maps the internal output back to the raw output layout (include/anemoi_amd.h "Remappers
// folded into predict_step's I/O kernels").  One thread owns every output element; no atomics; the same bits on every run.
//
// Separate code from assemble_nodes8_kernel (csrc/elementwise.hip) on purpose: that template reads and writes with ONE V and
// loads (v, v + 1) pairs; a table lookup per element in its loop would make the plain and imputed instantiations pay for a
// caller they never have.
#include <cstdlib>
#include <type_traits>

#include "common.hpp"
#include "trail.hpp"

namespace anemoi {

// per-column tables of one direction, device arrays; a NULL pair is the identity
struct RemapTable {
  const int32_t* op;
  const float* pre_mul;
  const float* pre_add;
  const float* post_mul;
  const float* post_add;
};

constexpr float kDegToRad = 0.017453292519943295f;
constexpr float kRadToDeg = 57.29577951308232f;

// THE device function of the three kernels: op code -> value.  u1 is read by ATAN2DEG alone.
__device__ __forceinline__ float remap_op(int op, float u, float u1) {
  switch (op) {
    case ANEMOI_REMAP_LOG1P: return log1pf(u);
    case ANEMOI_REMAP_SQRT: return sqrtf(u);
    case ANEMOI_REMAP_BOXCOX: return (sqrtf(u) - 1.f) / 0.5f;
    case ANEMOI_REMAP_COS: return cosf(u * kDegToRad);
    case ANEMOI_REMAP_SIN: return sinf(u * kDegToRad);
    case ANEMOI_REMAP_EXPM1: return expm1f(u);
    case ANEMOI_REMAP_SQUARE: return u * u;
    case ANEMOI_REMAP_INV_BOXCOX: {
      const float h = u * 0.5f + 1.f;
      return h * h;
    }
    case ANEMOI_REMAP_ATAN2DEG: {
      float d = fmodf(atan2f(u1, u) * kRadToDeg, 360.f);  // torch.remainder: the sign of the divisor
      if (d < 0.f) d += 360.f;
      return d;
    }
    default: return u;
  }
}

// f_j(x) = post_mul[j] * op_j(pre_mul[j] * x + pre_add[j]) + post_add[j]
__device__ __forceinline__ float remap_forward(const RemapTable& t, int j, float x) {
  if (t.pre_mul != nullptr) x = x * t.pre_mul[j] + t.pre_add[j];
  x = remap_op(t.op[j], x, 0.f);
  if (t.post_mul != nullptr) x = x * t.post_mul[j] + t.post_add[j];
  return x;
}

template <typename T>
__global__ __launch_bounds__(256) void assemble_remapped_kernel(const float* __restrict__ x, int B, int T_, int Ens, int64_t G,
                                                                int V_raw, int V_int, const float* __restrict__ latlons,
                                                                int n_ll, const float* __restrict__ trainable, int n_tr,
                                                                T* __restrict__ out, int64_t ldo,
                                                                const int32_t* __restrict__ src, const RemapTable tab) {
  const int64_t total = (int64_t)B * Ens * G * ldo;
  const int tv = T_ * V_int;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = idx / ldo;
    const int c = (int)(idx - row * ldo);
    const int64_t g = row % G;
    float val = 0.f;
    if (c < tv) {
      const int64_t be = row / G;
      const int e = (int)(be % Ens);
      const int64_t b = be / Ens;
      const int t = c / V_int, j = c - t * V_int;
      val = remap_forward(tab, j, x[((((b * T_ + t) * Ens + e) * G) + g) * V_raw + src[j]]);
    } else if (c < tv + n_ll) {
      val = latlons[g * n_ll + (c - tv)];
    } else if (c < tv + n_ll + n_tr) {
      val = trainable[g * n_tr + (c - tv - n_ll)];
    }
    Elem<T>::store(out + idx, val);
  }
}

// EIGHT consecutive output columns per thread (ldo % 8 == 0), one 16-byte (bf16) / two 16-byte (f32) stores, one row / column
// division per eight elements; IDX32: every flat index fits 31 bits (see assemble_nodes8_kernel)
template <typename T, bool IDX32>
__global__ __launch_bounds__(256) void assemble_remapped8_kernel(const float* __restrict__ x, int B, int T_, int Ens, int64_t G,
                                                                 int V_raw, int V_int, const float* __restrict__ latlons,
                                                                 int n_ll, const float* __restrict__ trainable, int n_tr,
                                                                 T* __restrict__ out, int ldo8,
                                                                 const int32_t* __restrict__ src, const RemapTable tab) {
  const int64_t total = (int64_t)B * Ens * G * ldo8;
  const int tv = T_ * V_int;
  using I = typename std::conditional<IDX32, unsigned, int64_t>::type;
  const bool one_be = B * Ens == 1;
  for (I idx = (I)blockIdx.x * blockDim.x + threadIdx.x; idx < (I)total; idx += (I)gridDim.x * blockDim.x) {
    const I row = idx / (I)ldo8;
    const int c0 = (int)(idx - row * (I)ldo8) * 8;
    int64_t g, b = 0;
    int e = 0;
    if (one_be) g = (int64_t)row;
    else {
      const I be = row / (I)G;
      g = (int64_t)(row - be * (I)G);
      e = (int)(be % (I)Ens);
      b = (int64_t)(be / (I)Ens);
    }
    float val[8];
    int t = c0 / V_int, j = c0 - t * V_int;  // (time, internal column) of column c0; advanced without further divisions
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int c = c0 + i;
      float r = 0.f;
      if (c < tv) {
        r = remap_forward(tab, j, x[((((b * T_ + t) * Ens + e) * G) + g) * V_raw + src[j]]);
        if (++j == V_int) {
          j = 0;
          ++t;
        }
      } else if (c < tv + n_ll) {
        r = latlons[g * n_ll + (c - tv)];
      } else if (c < tv + n_ll + n_tr) {
        r = trainable[g * n_tr + (c - tv - n_ll)];
      }
      val[i] = r;
    }
    VecIO<T, 8>::store(out + ((int64_t)row * ldo8 + (c0 >> 3)) * 8, val);
  }
}

// y[row, c] += f_j(x[b, T-1, e, g, src[j]]), j = res[c] >= 0; one thread per element of y
template <bool IDX32>
__global__ __launch_bounds__(256) void residual_remapped_kernel(float* __restrict__ y, int V_out, const float* __restrict__ x,
                                                                int T_, int Ens, int64_t G, int V_raw, int64_t total,
                                                                const int32_t* __restrict__ res,
                                                                const int32_t* __restrict__ src, const RemapTable tab) {
  using I = typename std::conditional<IDX32, unsigned, int64_t>::type;
  for (I idx = (I)blockIdx.x * blockDim.x + threadIdx.x; idx < (I)total; idx += (I)gridDim.x * blockDim.x) {
    const I row = idx / (I)V_out;
    const int c = (int)(idx - row * (I)V_out);
    const int j = res[c];
    if (j < 0) continue;
    const I be = row / (I)G;
    const int64_t g = (int64_t)(row - be * (I)G);
    const int e = (int)(be % (I)Ens);
    const int64_t b = (int64_t)(be / (I)Ens);
    y[idx] += remap_forward(tab, j, x[((((b * T_ + (T_ - 1)) * Ens + e) * G) + g) * V_raw + src[j]]);
  }
}

// out[row, c] = (op_c((y[row, s0[c]] - post_add) / post_mul, the same of s1[c]) - pre_add[c]) / pre_mul[c]
template <bool IDX32>
__global__ __launch_bounds__(256) void unmap_output_kernel(const float* __restrict__ y, int V_int, float* __restrict__ out,
                                                           int V_out, int64_t total, const int32_t* __restrict__ s0,
                                                           const int32_t* __restrict__ s1, const RemapTable tab) {
  using I = typename std::conditional<IDX32, unsigned, int64_t>::type;
  for (I idx = (I)blockIdx.x * blockDim.x + threadIdx.x; idx < (I)total; idx += (I)gridDim.x * blockDim.x) {
    const I row = idx / (I)V_out;
    const int c = (int)(idx - row * (I)V_out);
    const float* yr = y + (int64_t)row * V_int;
    const int op = tab.op[c];
    const int a = s0[c];
    float u = yr[a], u1 = 0.f;
    if (tab.post_mul != nullptr) u = (u - tab.post_add[a]) / tab.post_mul[a];
    if (op == ANEMOI_REMAP_ATAN2DEG) {
      const int a1 = s1[c];
      u1 = yr[a1];
      if (tab.post_mul != nullptr) u1 = (u1 - tab.post_add[a1]) / tab.post_mul[a1];
    }
    float z = remap_op(op, u, u1);
    if (tab.pre_mul != nullptr) z = (z - tab.pre_add[c]) / tab.pre_mul[c];
    out[idx] = z;
  }
}

// ANEMOI_AMD_IDX64=1 forces the 64-bit index instantiations (tests: no tensor of 2^31 elements needed)
static bool force_idx64() {
  static const bool v = [] {
    const char* e = getenv("ANEMOI_AMD_IDX64");
    return e != nullptr && atoi(e) != 0;
  }();
  return v;
}

static inline unsigned flat_grid(int64_t total) {
  int64_t blocks = (total + 255) / 256;
  if (blocks > 256 * 16) blocks = 256 * 16;  // grid-stride the rest
  if (blocks < 1) blocks = 1;
  return (unsigned)blocks;
}

static inline bool fits_idx32(int64_t total) {  // (+ one grid stride stays below 2^31)
  return !force_idx64() && total < ((int64_t)1 << 31) - ((int64_t)1 << 24);
}

// the forward tables of an entry point: device pointers all given or, for a pair, both NULL; host copies inside their range
static int check_forward(const char* who, int V_raw, int V_int, const int32_t* src, const RemapTable& tab, const int32_t* h_src,
                         const int32_t* h_op) {
  ANEMOI_REQUIRE(V_raw > 0 && V_int > 0, ANEMOI_ERR_INVALID, "%s: V_raw %d / V_int %d", who, V_raw, V_int);
  ANEMOI_REQUIRE(src && tab.op && h_src && h_op, ANEMOI_ERR_INVALID, "%s: null src / op table", who);
  ANEMOI_REQUIRE((tab.pre_mul == nullptr) == (tab.pre_add == nullptr) && (tab.post_mul == nullptr) == (tab.post_add == nullptr),
                 ANEMOI_ERR_INVALID, "%s: the mul and add table of a pair come together", who);
  for (int j = 0; j < V_int; ++j) {
    ANEMOI_REQUIRE(h_src[j] >= 0 && h_src[j] < V_raw, ANEMOI_ERR_INVALID, "%s: src[%d] = %d outside [0, %d)", who, j, h_src[j],
                   V_raw);
    ANEMOI_REQUIRE(h_op[j] >= ANEMOI_REMAP_COPY && h_op[j] <= ANEMOI_REMAP_SIN, ANEMOI_ERR_INVALID,
                   "%s: op[%d] = %d is no forward op code", who, j, h_op[j]);
  }
  return ANEMOI_OK;
}

}  // namespace anemoi

using namespace anemoi;

extern "C" {

int anemoi_assemble_nodes_remapped(int dtype, const float* x, int B, int T, int Ens, int64_t G, int V_raw, int V_int,
                                   const float* latlons, int n_ll, const float* trainable, int n_tr, void* out, int64_t ldo,
                                   const int32_t* src, const int32_t* op, const float* pre_mul, const float* pre_add,
                                   const float* post_mul, const float* post_add, const int32_t* h_src, const int32_t* h_op,
                                   anemoi_stream_t stream) {
  const char* who = "anemoi_assemble_nodes_remapped";
  const RemapTable tab{op, pre_mul, pre_add, post_mul, post_add};
  const int rc = check_forward(who, V_raw, V_int, src, tab, h_src, h_op);
  if (rc != ANEMOI_OK) return rc;
  ANEMOI_REQUIRE(x && out && B > 0 && Ens > 0 && G >= 0 && T > 0 && n_ll >= 0 && n_tr >= 0, ANEMOI_ERR_INVALID,
                 "%s: bad argument", who);
  ANEMOI_REQUIRE((latlons != nullptr) || n_ll == 0, ANEMOI_ERR_INVALID, "%s: latlons is null", who);
  ANEMOI_REQUIRE((trainable != nullptr) || n_tr == 0, ANEMOI_ERR_INVALID, "%s: trainable is null", who);
  ANEMOI_REQUIRE(ldo >= (int64_t)T * V_int + n_ll + n_tr, ANEMOI_ERR_INVALID, "%s: ldo too small", who);
  ANEMOI_REQUIRE(dtype == ANEMOI_F32 || dtype == ANEMOI_BF16, ANEMOI_ERR_UNSUPPORTED, "%s: dtype %d", who, dtype);
  const int64_t total = (int64_t)B * Ens * G * ldo;
  if (total == 0) return ANEMOI_OK;
  hipStream_t st = as_stream(stream);
  if (ldo % 8 == 0 && ldo < ((int64_t)1 << 31) && (uintptr_t)out % 16 == 0) {
    const int ldo8 = (int)(ldo / 8);
#define ANEMOI_RMP8(TT, I32)                                                                                                  \
  hipLaunchKernelGGL((assemble_remapped8_kernel<TT, I32>), dim3(flat_grid(total / 8)), dim3(256), 0, st, x, B, T, Ens, G, V_raw, \
                     V_int, latlons, n_ll, trainable, n_tr, static_cast<TT*>(out), ldo8, src, tab)
    const bool idx32 = fits_idx32(total / 8);
    if (dtype == ANEMOI_F32) {
      if (idx32) ANEMOI_RMP8(float, true);
      else ANEMOI_RMP8(float, false);
    } else {
      if (idx32) ANEMOI_RMP8(bf16_t, true);
      else ANEMOI_RMP8(bf16_t, false);
    }
#undef ANEMOI_RMP8
    return trail::note(check_launch(who), who, "out", dtype, out, ldo, total / ldo, ldo, st);
  }
#define ANEMOI_RMP1(TT)                                                                                                        \
  hipLaunchKernelGGL((assemble_remapped_kernel<TT>), dim3(flat_grid(total)), dim3(256), 0, st, x, B, T, Ens, G, V_raw, V_int, \
                     latlons, n_ll, trainable, n_tr, static_cast<TT*>(out), ldo, src, tab)
  if (dtype == ANEMOI_F32) ANEMOI_RMP1(float);
  else ANEMOI_RMP1(bf16_t);
#undef ANEMOI_RMP1
  return trail::note(check_launch(who), who, "out", dtype, out, ldo, total / ldo, ldo, st);
}

int anemoi_residual_remapped(float* y, int V_int_out, const float* x, int B, int T, int Ens, int64_t G, int V_raw, int V_int,
                             const int32_t* res, const int32_t* src, const int32_t* op, const float* pre_mul,
                             const float* pre_add, const float* post_mul, const float* post_add, const int32_t* h_res,
                             const int32_t* h_src, const int32_t* h_op, anemoi_stream_t stream) {
  const char* who = "anemoi_residual_remapped";
  const RemapTable tab{op, pre_mul, pre_add, post_mul, post_add};
  const int rc = check_forward(who, V_raw, V_int, src, tab, h_src, h_op);
  if (rc != ANEMOI_OK) return rc;
  ANEMOI_REQUIRE(y && x && res && h_res && V_int_out > 0 && B > 0 && Ens > 0 && G >= 0 && T > 0, ANEMOI_ERR_INVALID,
                 "%s: bad argument", who);
  for (int c = 0; c < V_int_out; ++c)
    ANEMOI_REQUIRE(h_res[c] >= -1 && h_res[c] < V_int, ANEMOI_ERR_INVALID, "%s: res[%d] = %d outside [-1, %d)", who, c, h_res[c],
                   V_int);
  const int64_t rows = (int64_t)B * Ens * G, total = rows * V_int_out;
  if (total == 0) return ANEMOI_OK;
  hipStream_t st = as_stream(stream);
  if (fits_idx32(total))
    hipLaunchKernelGGL((residual_remapped_kernel<true>), dim3(flat_grid(total)), dim3(256), 0, st, y, V_int_out, x, T, Ens, G,
                       V_raw, total, res, src, tab);
  else
    hipLaunchKernelGGL((residual_remapped_kernel<false>), dim3(flat_grid(total)), dim3(256), 0, st, y, V_int_out, x, T, Ens, G,
                       V_raw, total, res, src, tab);
  return trail::note(check_launch(who), who, "out", ANEMOI_F32, y, V_int_out, rows, V_int_out, st);
}

int anemoi_unmap_output(const float* y, int V_int_out, float* out, int V_out, int64_t rows, const int32_t* s0,
                        const int32_t* s1, const int32_t* op, const float* pre_mul, const float* pre_add,
                        const float* post_mul, const float* post_add, const int32_t* h_s0, const int32_t* h_s1,
                        const int32_t* h_op, anemoi_stream_t stream) {
  const char* who = "anemoi_unmap_output";
  ANEMOI_REQUIRE(y && out && y != out && V_int_out > 0 && V_out > 0 && rows >= 0, ANEMOI_ERR_INVALID, "%s: bad argument", who);
  ANEMOI_REQUIRE(s0 && s1 && op && h_s0 && h_s1 && h_op, ANEMOI_ERR_INVALID, "%s: null s0 / s1 / op table", who);
  ANEMOI_REQUIRE((pre_mul == nullptr) == (pre_add == nullptr) && (post_mul == nullptr) == (post_add == nullptr),
                 ANEMOI_ERR_INVALID, "%s: the mul and add table of a pair come together", who);
  for (int c = 0; c < V_out; ++c) {
    const int o = h_op[c];
    ANEMOI_REQUIRE(o == ANEMOI_REMAP_COPY || (o >= ANEMOI_REMAP_EXPM1 && o <= ANEMOI_REMAP_ATAN2DEG), ANEMOI_ERR_INVALID,
                   "%s: op[%d] = %d is no inverse op code", who, c, o);
    ANEMOI_REQUIRE(h_s0[c] >= 0 && h_s0[c] < V_int_out, ANEMOI_ERR_INVALID, "%s: s0[%d] = %d outside [0, %d)", who, c, h_s0[c],
                   V_int_out);
    ANEMOI_REQUIRE(o != ANEMOI_REMAP_ATAN2DEG || (h_s1[c] >= 0 && h_s1[c] < V_int_out), ANEMOI_ERR_INVALID,
                   "%s: s1[%d] = %d outside [0, %d)", who, c, h_s1[c], V_int_out);
  }
  const int64_t total = rows * V_out;
  if (total == 0) return ANEMOI_OK;
  hipStream_t st = as_stream(stream);
  const RemapTable tab{op, pre_mul, pre_add, post_mul, post_add};
  if (fits_idx32(total) && fits_idx32(rows * V_int_out))
    hipLaunchKernelGGL((unmap_output_kernel<true>), dim3(flat_grid(total)), dim3(256), 0, st, y, V_int_out, out, V_out, total, s0,
                       s1, tab);
  else
    hipLaunchKernelGGL((unmap_output_kernel<false>), dim3(flat_grid(total)), dim3(256), 0, st, y, V_int_out, out, V_out, total,
                       s0, s1, tab);
  return trail::note(check_launch(who), who, "out", ANEMOI_F32, out, V_out, rows, V_out, st);
}

}  // extern "C"
