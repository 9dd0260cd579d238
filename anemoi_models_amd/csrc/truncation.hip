// Truncated residual connection ("8f-9"): one CSR projection kernel,
//   out[s, i, cols_out[p]]  (= or +=)  sum_{k = indptr[i] .. indptr[i+1]-1} val[k] * x'[s, idx[k], cols_in[p]],   p < P,
// that serves the down- and the up-projection of x_skip = A_up (A_down x[:, -1]) and, on the transposed matrices, their
// backward.  A bandwidth-bound gather of short f32 row segments (P * 4 bytes out of rows of ldx * 4).
//
// Mapping: the columns lie across the lanes.  W = the power of two >= min(P, 64) lanes hold one output row, so a wave holds
// R = 64 / W rows (P <= 32) or one 64-column chunk of one row (P > 32: blockIdx.y counts the chunks).  Slabs are blockIdx.z.
// With one row per wave the row index is wave-uniform and indptr / idx / val come through scalar loads; with packed rows
// they are per-lane loads of an address that the W lanes of a row share.  Every output element is owned by exactly one lane,
// which adds its row's terms in ascending CSR position with one FMA each: no atomics, no workspace, the same bits on every
// run and for every slab count.
#include "common.hpp"
#include "trail.hpp"

namespace anemoi {

constexpr int CSR_MAX_BLOCKS_X = 256 * 32;  // row groups beyond this are grid-strided
constexpr int CSR_MAX_GRID_YZ = 65535;

struct CsrProjectArgs {
  const float* x;
  int64_t ldx, xs_outer, xs_inner;
  float* out;
  int64_t ldo, os_outer, os_inner;
  int n_inner;
  int64_t n_out;
  const int64_t* indptr;
  const int32_t* idx;
  const float* val;
  const int32_t* cols_in;
  const int32_t* cols_out;
  int P;
  const float* in_mul;
  const float* in_add;
};

template <int W, bool AFFINE, bool ACCUMULATE>
__global__ __launch_bounds__(256) void csr_project_kernel(const CsrProjectArgs a) {
  constexpr int R = 64 / W;
  const int lane = threadIdx.x & 63;
  const int sub = lane / W, pl = lane % W;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int p = (int)blockIdx.y * W + pl;
  if (p >= a.P) return;  // (no wave-level operation below: lanes leave on their own)
  const int s = (int)blockIdx.z;
  const int64_t so = s / a.n_inner, si = s - so * a.n_inner;
  const float* __restrict__ xs = a.x + so * a.xs_outer + si * a.xs_inner;
  float* __restrict__ os = a.out + so * a.os_outer + si * a.os_inner;
  // val is read as 32-bit words.  A wave-uniform load becomes a scalar load only when the compiler can show that no store of
  // the kernel may change the word; as floats, val may alias the float stores to `out` by type, and `__restrict__` does not
  // help: the pointers come out of the by-value argument struct, where the qualifier on a local copy is not carried to the
  // loads (tried, the listing kept one wave-uniform global_load_dwordx4 per four entries).  indptr and idx are integers and
  // take scalar loads as they are.  Only the choice of load instruction rests on this: the words are the same either way,
  // and ops.csr_project refuses an `out` that overlaps `x`; the CSR arrays are never written by any launch.
  const int32_t* __restrict__ val = reinterpret_cast<const int32_t*>(a.val);
  const int ci = a.cols_in != nullptr ? a.cols_in[p] : p;
  const int co = a.cols_out != nullptr ? a.cols_out[p] : p;
  float mul = 1.f, add = 0.f;
  if constexpr (AFFINE) {
    mul = a.in_mul[ci];
    add = a.in_add[ci];
  }
  const int64_t n_groups = (a.n_out + R - 1) / R;
  for (int64_t g = (int64_t)blockIdx.x * 4 + wave; g < n_groups; g += (int64_t)gridDim.x * 4) {
    const int64_t row = g * R + sub;  // wave-uniform when R == 1: scalar loads of indptr / idx / val
    if (row >= a.n_out) continue;
    const int64_t beg = a.indptr[row], end = a.indptr[row + 1];
    if (ACCUMULATE && beg >= end) continue;  // an empty row leaves out untouched
    float acc = 0.f;
    int64_t k = beg;
    for (; k + 4 <= end; k += 4) {  // four gathers in flight, added in CSR order
      float xv[4], v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        v[u] = __int_as_float(val[k + u]);
        xv[u] = xs[(int64_t)a.idx[k + u] * a.ldx + ci];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if constexpr (AFFINE) xv[u] = fmaf(xv[u], mul, add);
        acc = fmaf(v[u], xv[u], acc);
      }
    }
    for (; k < end; ++k) {
      float xv = xs[(int64_t)a.idx[k] * a.ldx + ci];
      if constexpr (AFFINE) xv = fmaf(xv, mul, add);
      acc = fmaf(__int_as_float(val[k]), xv, acc);
    }
    float* o = os + row * a.ldo + co;
    if constexpr (ACCUMULATE) *o += acc;
    else *o = acc;
  }
}

template <int W>
static void csr_project_launch(const CsrProjectArgs& a, bool affine, bool accumulate, dim3 grid, hipStream_t st) {
  if (affine && accumulate) hipLaunchKernelGGL((csr_project_kernel<W, true, true>), grid, dim3(256), 0, st, a);
  else if (affine) hipLaunchKernelGGL((csr_project_kernel<W, true, false>), grid, dim3(256), 0, st, a);
  else if (accumulate) hipLaunchKernelGGL((csr_project_kernel<W, false, true>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((csr_project_kernel<W, false, false>), grid, dim3(256), 0, st, a);
}

}  // namespace anemoi

using namespace anemoi;

extern "C" {

int anemoi_csr_project(const float* x, int64_t ldx, int64_t xs_outer, int64_t xs_inner, float* out, int64_t ldo,
                       int64_t os_outer, int64_t os_inner, int n_outer, int n_inner, int64_t n_in, int64_t n_out,
                       const int64_t* indptr, const int32_t* idx, const float* val, const int32_t* cols_in,
                       const int32_t* cols_out, int P, const float* in_mul, const float* in_add, int accumulate,
                       anemoi_stream_t stream) {
  ANEMOI_REQUIRE(x && out && indptr && idx && val, ANEMOI_ERR_INVALID, "anemoi_csr_project: null pointer");
  ANEMOI_REQUIRE(P > 0, ANEMOI_ERR_INVALID, "anemoi_csr_project: P = %d columns", P);
  ANEMOI_REQUIRE(n_outer >= 0 && n_inner >= 0 && n_in >= 0 && n_out >= 0, ANEMOI_ERR_INVALID,
                 "anemoi_csr_project: negative size (slabs %d x %d, n_in %lld, n_out %lld)", n_outer, n_inner,
                 (long long)n_in, (long long)n_out);
  ANEMOI_REQUIRE((in_mul == nullptr) == (in_add == nullptr), ANEMOI_ERR_INVALID,
                 "anemoi_csr_project: in_mul and in_add come together");
  ANEMOI_REQUIRE(accumulate == 0 || accumulate == 1, ANEMOI_ERR_INVALID, "anemoi_csr_project: accumulate is 0 or 1, got %d",
                 accumulate);
  // what the kernel can address: unit-stride columns, rows ldx / ldo apart, slabs at non-negative element strides
  ANEMOI_REQUIRE(ldx >= (cols_in ? 1 : P) && ldo >= (cols_out ? 1 : P), ANEMOI_ERR_INVALID,
                 "anemoi_csr_project: row pitch ldx %lld / ldo %lld too small for P = %d", (long long)ldx, (long long)ldo, P);
  ANEMOI_REQUIRE(xs_outer >= 0 && xs_inner >= 0 && os_outer >= 0 && os_inner >= 0, ANEMOI_ERR_INVALID,
                 "anemoi_csr_project: negative slab stride");
  const int64_t slabs = (int64_t)n_outer * n_inner;
  {  // output slabs must not overlap: each level steps over everything below it (either level may be the larger one)
    const int64_t slab = n_out * ldo;
    const bool in_lvl = n_inner > 1, out_lvl = n_outer > 1;
    bool ok = (!in_lvl || os_inner >= slab) && (!out_lvl || os_outer >= slab);
    if (ok && in_lvl && out_lvl)
      ok = os_outer >= (int64_t)n_inner * os_inner || os_inner >= (int64_t)n_outer * os_outer;
    ANEMOI_REQUIRE(ok, ANEMOI_ERR_INVALID, "anemoi_csr_project: output slabs overlap (strides %lld / %lld, slab %lld elements)",
                   (long long)os_outer, (long long)os_inner, (long long)slab);
  }
  const int64_t chunks = ((int64_t)P + 63) / 64;
  ANEMOI_REQUIRE(slabs <= CSR_MAX_GRID_YZ && chunks <= CSR_MAX_GRID_YZ, ANEMOI_ERR_UNSUPPORTED,
                 "anemoi_csr_project: %lld slabs / %lld column chunks (at most %d each)", (long long)slabs, (long long)chunks,
                 CSR_MAX_GRID_YZ);
  if (slabs == 0 || n_out == 0) return ANEMOI_OK;

  CsrProjectArgs a{x, ldx, xs_outer, xs_inner, out, ldo, os_outer, os_inner, n_inner, n_out, indptr, idx, val,
                   cols_in, cols_out, P, in_mul, in_add};
  int w = 1;
  while (w < P && w < 64) w *= 2;
  const int64_t groups = (n_out + (64 / w) - 1) / (64 / w);
  int64_t bx = (groups + 3) / 4;
  if (bx > CSR_MAX_BLOCKS_X) bx = CSR_MAX_BLOCKS_X;
  const dim3 grid((unsigned)bx, (unsigned)(w == 64 ? chunks : 1), (unsigned)slabs);
  hipStream_t st = as_stream(stream);
  const bool affine = in_mul != nullptr, acc = accumulate != 0;
  switch (w) {
    case 1: csr_project_launch<1>(a, affine, acc, grid, st); break;
    case 2: csr_project_launch<2>(a, affine, acc, grid, st); break;
    case 4: csr_project_launch<4>(a, affine, acc, grid, st); break;
    case 8: csr_project_launch<8>(a, affine, acc, grid, st); break;
    case 16: csr_project_launch<16>(a, affine, acc, grid, st); break;
    case 32: csr_project_launch<32>(a, affine, acc, grid, st); break;
    default: csr_project_launch<64>(a, affine, acc, grid, st); break;
  }
  // the record covers the rows of the first slab (the slabs need not be evenly spaced)
  return trail::note(check_launch("anemoi_csr_project"), "anemoi_csr_project", "out", ANEMOI_F32, out, ldo, n_out,
                     cols_out ? ldo : P, st);
}

}  // extern "C"
