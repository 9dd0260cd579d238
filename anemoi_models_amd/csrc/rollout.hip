// Rollout training ("rollout"): the differentiable state advance between two steps of an autoregressive
// rollout and the input gradients of the one-pass I/O kernels (anemoi_assemble_nodes / anemoi_finalize_output).  (The loss of
// a rollout step is in csrc/losses.hip.)
//
// All of them are streaming kernels in the style of csrc/elementwise.hip: a flat grid-stride mapping, 16-byte accesses where
// the rows allow, 32-bit index divisions when the flat index space fits 31 bits.  Every output element is owned by exactly one
// thread -- no atomics, the same bits on every run.
#include "common.hpp"
#include "trail.hpp"

namespace anemoi {

static inline unsigned flat_grid(int64_t total) {
  int64_t blocks = (total + 255) / 256;
  if (blocks > 256 * 16) blocks = 256 * 16;  // grid-stride the rest
  if (blocks < 1) blocks = 1;
  return (unsigned)blocks;
}

// ---------------------------------------------------------------------------------------------
// State advance, out of place.  `slab` = Ens * G * V_in floats of one (b, t); the flat index space is
//   [0, n_copy)          VEC-wide pieces of x_out[:, 0..T-2] = x_in[:, 1..T-1]
//   [n_copy, + B * slab) the elements of the last time slice, by colmap (the arithmetic of advance_input_kernel)
// ---------------------------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(256) void advance_state_kernel(const float* __restrict__ x_in, float* __restrict__ x_out,
                                                            int B, int T_, int64_t slab, int V_in,
                                                            const float* __restrict__ y, int V_out,
                                                            const float* __restrict__ forcing, int F,
                                                            const int32_t* __restrict__ colmap) {
  const int64_t per = slab / VEC;  // (VEC > 1 only when it divides the slab)
  const int64_t n_copy = (int64_t)B * (T_ - 1) * per;
  const int64_t total = n_copy + (int64_t)B * slab;
  const bool fits32 = total < ((int64_t)1 << 31);
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    if (idx < n_copy) {
      int64_t bt, piece, b, t;
      fast_divmod(idx, per, fits32, bt, piece);
      fast_divmod(bt, T_ - 1, fits32, b, t);
      float v[VEC];
      VecIO<float, VEC>::load(x_in + (b * T_ + t + 1) * slab + piece * VEC, v);
      VecIO<float, VEC>::store(x_out + (b * T_ + t) * slab + piece * VEC, v);
    } else {
      const int64_t j = idx - n_copy;  // flat (b, ens, g, v)
      int64_t row, v64, b, in_slab;    // row = (b, ens, g)
      fast_divmod(j, V_in, fits32, row, v64);
      fast_divmod(j, slab, fits32, b, in_slab);
      const int64_t last = (b * T_ + (T_ - 1)) * slab + in_slab;
      const int m = colmap[v64];
      float val;
      if (m >= 0) val = y[row * V_out + m];
      else if (m <= -2 && forcing != nullptr) val = forcing[row * F + (-2 - m)];
      else val = x_in[last];
      x_out[last] = val;
    }
  }
}

// Its backward: dx_in (three regions as above: zeros for t = 0, the shifted copy for 0 < t < T-1, the last slice) and dy.
//   [0, n_head)                 VEC-wide pieces of dx_in[:, 0..T-2]: 0 for t = 0, dx_out[:, t-1] else
//   [n_head, + B * slab)        dx_in[:, T-1]: dx_out[:, T-2] (T > 1) + dx_out[:, T-1] in the persisting columns
//   [.., + B * Ens * G * V_out) dy[.., m] = dx_out[:, T-1, .., inv[m]] where inv[m] >= 0, else 0
template <int VEC>
__global__ __launch_bounds__(256) void advance_state_backward_kernel(const float* __restrict__ dx_out,
                                                                     float* __restrict__ dx_in, float* __restrict__ dy,
                                                                     int B, int T_, int64_t slab, int V_in, int V_out,
                                                                     const int32_t* __restrict__ colmap,
                                                                     const int32_t* __restrict__ inv, int has_forcing) {
  const int64_t per = slab / VEC;
  const int64_t n_head = (int64_t)B * (T_ - 1) * per;
  const int64_t n_last = (int64_t)B * slab;
  const int64_t n_dy = n_last / V_in * V_out;
  const int64_t total = n_head + n_last + n_dy;
  const bool fits32 = total < ((int64_t)1 << 31);
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    if (idx < n_head) {
      int64_t bt, piece, b, t;
      fast_divmod(idx, per, fits32, bt, piece);
      fast_divmod(bt, T_ - 1, fits32, b, t);
      float v[VEC];
      if (t == 0) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) v[k] = 0.f;
      } else {
        VecIO<float, VEC>::load(dx_out + (b * T_ + t - 1) * slab + piece * VEC, v);
      }
      VecIO<float, VEC>::store(dx_in + (b * T_ + t) * slab + piece * VEC, v);
    } else if (idx < n_head + n_last) {
      const int64_t j = idx - n_head;
      int64_t row, v64, b, in_slab;
      fast_divmod(j, V_in, fits32, row, v64);
      fast_divmod(j, slab, fits32, b, in_slab);
      const int64_t last = (b * T_ + (T_ - 1)) * slab + in_slab;
      const int m = colmap[v64];
      const bool persists = m == -1 || (m <= -2 && !has_forcing);
      float val = T_ > 1 ? dx_out[last - slab] : 0.f;
      if (persists) val = T_ > 1 ? val + dx_out[last] : dx_out[last];
      dx_in[last] = val;
    } else {
      const int64_t j = idx - n_head - n_last;  // flat (row, m)
      int64_t row, m, b, eg;
      fast_divmod(j, V_out, fits32, row, m);
      const int v = inv[m];
      float val = 0.f;
      if (v >= 0) {
        const int64_t rows_per_b = slab / V_in;  // Ens * G
        fast_divmod(row, rows_per_b, fits32, b, eg);
        val = dx_out[(b * T_ + (T_ - 1)) * slab + eg * V_in + v];
      }
      dy[j] = val;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Input gradient of anemoi_assemble_nodes: dx[b, t, ens, g, v0..v0+VEC) = float(grad[(b, ens, g), t * V + v0 ..]).
// ---------------------------------------------------------------------------------------------
template <typename T, int VEC>
__global__ __launch_bounds__(256) void assemble_nodes_backward_kernel(const T* __restrict__ grad, int64_t ldg,
                                                                      float* __restrict__ dx, int B, int T_, int Ens,
                                                                      int64_t G, int V) {
  const int vp = V / VEC;  // (VEC > 1 only when it divides V)
  const int64_t total = (int64_t)B * T_ * Ens * G * vp;
  const bool fits32 = total < ((int64_t)1 << 31);
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    int64_t q, piece, bte, g, bt, e, b, t;
    fast_divmod(idx, vp, fits32, q, piece);
    fast_divmod(q, G, fits32, bte, g);
    fast_divmod(bte, Ens, fits32, bt, e);
    fast_divmod(bt, T_, fits32, b, t);
    const int64_t row = (b * Ens + e) * G + g;
    float v[VEC];
    VecIO<T, VEC>::load(grad + row * ldg + t * V + piece * VEC, v);
    VecIO<float, VEC>::store(dx + idx * VEC, v);
  }
}

// ---------------------------------------------------------------------------------------------
// Input gradient of the prognostic residual of anemoi_finalize_output: dx is zero except for the last time slice, where input
// column v receives dy[.., c] of the output column(s) c with src[c] == v.  The inverse of src is built per workgroup in LDS
// (first[v], count[v]); a column that feeds several outputs (count > 1) sums them in output-column order.
// ---------------------------------------------------------------------------------------------
constexpr int RESIDUAL_BWD_MAX_V = 1024;

template <int VEC>
__global__ __launch_bounds__(256) void prognostic_residual_backward_kernel(const float* __restrict__ dy, int V_out,
                                                                           float* __restrict__ dx, int B, int T_,
                                                                           int64_t slab, int V_in,
                                                                           const int32_t* __restrict__ src) {
  __shared__ int32_t first[RESIDUAL_BWD_MAX_V];
  __shared__ int32_t count[RESIDUAL_BWD_MAX_V];
  for (int v = threadIdx.x; v < V_in; v += blockDim.x) {
    int f = -1, n = 0;
    for (int c = 0; c < V_out; ++c) {
      if (src[c] == v) {
        if (f < 0) f = c;
        ++n;
      }
    }
    first[v] = f;
    count[v] = n;
  }
  __syncthreads();
  const int64_t per = slab / VEC;
  const int64_t n_head = (int64_t)B * (T_ - 1) * per;
  const int64_t total = n_head + (int64_t)B * slab;
  const bool fits32 = total < ((int64_t)1 << 31);
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    if (idx < n_head) {
      int64_t bt, piece, b, t;
      fast_divmod(idx, per, fits32, bt, piece);
      fast_divmod(bt, T_ - 1, fits32, b, t);
      float z[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) z[k] = 0.f;
      VecIO<float, VEC>::store(dx + (b * T_ + t) * slab + piece * VEC, z);
    } else {
      const int64_t j = idx - n_head;
      int64_t row, v64, b, in_slab;
      fast_divmod(j, V_in, fits32, row, v64);
      fast_divmod(j, slab, fits32, b, in_slab);
      const int v = (int)v64, n = count[v];
      float val = 0.f;
      if (n == 1) {
        val = dy[row * V_out + first[v]];
      } else if (n > 1) {
        for (int c = first[v]; c < V_out; ++c)
          if (src[c] == v) val += dy[row * V_out + c];
      }
      dx[(b * T_ + (T_ - 1)) * slab + in_slab] = val;
    }
  }
}

static int check_state_shape(const char* who, int B, int T, int Ens, int64_t G, int V_in, int V_out) {
  ANEMOI_REQUIRE(B > 0 && T > 0 && Ens > 0 && G >= 0 && V_in > 0 && V_out > 0, ANEMOI_ERR_INVALID,
                 "%s: bad shape B=%d T=%d Ens=%d G=%lld V_in=%d V_out=%d", who, B, T, Ens, (long long)G, V_in, V_out);
  return ANEMOI_OK;
}

}  // namespace anemoi

using namespace anemoi;

extern "C" {

int anemoi_advance_state(const float* x_in, float* x_out, int B, int T, int Ens, int64_t G, int V_in, const float* y,
                         int V_out, const float* forcing, int F, const int32_t* colmap, anemoi_stream_t stream) {
  ANEMOI_REQUIRE(x_in && x_out && y && colmap, ANEMOI_ERR_INVALID, "anemoi_advance_state: null pointer");
  if (int rc = check_state_shape("anemoi_advance_state", B, T, Ens, G, V_in, V_out)) return rc;
  ANEMOI_REQUIRE(F >= 0 && (forcing != nullptr || F == 0), ANEMOI_ERR_INVALID, "anemoi_advance_state: bad forcing (F=%d)", F);
  const int64_t slab = (int64_t)Ens * G * V_in;
  const int64_t numel = (int64_t)B * T * slab;
  ANEMOI_REQUIRE(x_out + numel <= x_in || x_in + numel <= x_out, ANEMOI_ERR_INVALID,
                 "anemoi_advance_state: x_out must not alias x_in (anemoi_advance_input is the in-place form)");
  if (numel == 0) return ANEMOI_OK;
  hipStream_t st = as_stream(stream);
  if (slab % 4 == 0 && aligned16(x_in) && aligned16(x_out))
    hipLaunchKernelGGL(advance_state_kernel<4>, dim3(flat_grid((int64_t)B * (T - 1) * (slab / 4) + (int64_t)B * slab)),
                       dim3(256), 0, st, x_in, x_out, B, T, slab, V_in, y, V_out, forcing, F, colmap);
  else
    hipLaunchKernelGGL(advance_state_kernel<1>, dim3(flat_grid(numel)), dim3(256), 0, st, x_in, x_out, B, T, slab, V_in,
                       y, V_out, forcing, F, colmap);
  return trail::note(check_launch("anemoi_advance_state"), "anemoi_advance_state", "out", ANEMOI_F32, x_out, V_in,
                     (int64_t)B * T * Ens * G, V_in, st);
}

int anemoi_advance_state_backward(const float* dx_out, float* dx_in, float* dy, int B, int T, int Ens, int64_t G,
                                  int V_in, int V_out, const int32_t* colmap, const int32_t* inv_colmap,
                                  int has_forcing, anemoi_stream_t stream) {
  ANEMOI_REQUIRE(dx_out && dx_in && dy && colmap && inv_colmap, ANEMOI_ERR_INVALID,
                 "anemoi_advance_state_backward: null pointer");
  if (int rc = check_state_shape("anemoi_advance_state_backward", B, T, Ens, G, V_in, V_out)) return rc;
  const int64_t slab = (int64_t)Ens * G * V_in;
  const int64_t numel = (int64_t)B * T * slab;
  ANEMOI_REQUIRE(dx_in + numel <= dx_out || dx_out + numel <= dx_in, ANEMOI_ERR_INVALID,
                 "anemoi_advance_state_backward: dx_in must not alias dx_out");
  if (numel == 0) return ANEMOI_OK;
  hipStream_t st = as_stream(stream);
  const int64_t rows = (int64_t)B * Ens * G;
  const int64_t tail = (int64_t)B * slab + rows * V_out;
  if (slab % 4 == 0 && aligned16(dx_out) && aligned16(dx_in))
    hipLaunchKernelGGL(advance_state_backward_kernel<4>, dim3(flat_grid((int64_t)B * (T - 1) * (slab / 4) + tail)),
                       dim3(256), 0, st, dx_out, dx_in, dy, B, T, slab, V_in, V_out, colmap, inv_colmap, has_forcing);
  else
    hipLaunchKernelGGL(advance_state_backward_kernel<1>, dim3(flat_grid((int64_t)B * (T - 1) * slab + tail)), dim3(256), 0,
                       st, dx_out, dx_in, dy, B, T, slab, V_in, V_out, colmap, inv_colmap, has_forcing);
  int rc = trail::note(check_launch("anemoi_advance_state_backward"), "anemoi_advance_state_backward", "dx", ANEMOI_F32,
                       dx_in, V_in, (int64_t)B * T * Ens * G, V_in, st);
  return trail::note(rc, "anemoi_advance_state_backward", "dy", ANEMOI_F32, dy, V_out, rows, V_out, st);
}

int anemoi_assemble_nodes_backward(int dtype, const void* grad, int64_t ldg, float* dx, int B, int T, int Ens, int64_t G,
                                   int V, anemoi_stream_t stream) {
  ANEMOI_REQUIRE(grad && dx, ANEMOI_ERR_INVALID, "anemoi_assemble_nodes_backward: null pointer");
  ANEMOI_REQUIRE(B > 0 && T > 0 && Ens > 0 && G >= 0 && V > 0, ANEMOI_ERR_INVALID,
                 "anemoi_assemble_nodes_backward: bad shape B=%d T=%d Ens=%d G=%lld V=%d", B, T, Ens, (long long)G, V);
  ANEMOI_REQUIRE(ldg >= (int64_t)T * V, ANEMOI_ERR_INVALID, "anemoi_assemble_nodes_backward: ldg %lld < T * V = %lld",
                 (long long)ldg, (long long)T * V);
  ANEMOI_REQUIRE(dtype == ANEMOI_F32 || dtype == ANEMOI_BF16, ANEMOI_ERR_UNSUPPORTED,
                 "anemoi_assemble_nodes_backward: dtype %d", dtype);
  const int64_t numel = (int64_t)B * T * Ens * G * V;
  if (numel == 0) return ANEMOI_OK;
  hipStream_t st = as_stream(stream);
  const int64_t esize = dtype == ANEMOI_F32 ? 4 : 2;
  // four columns per thread: every 4-column piece of a row starts on a (4 * element size)-byte boundary
  const bool vec = V % 4 == 0 && ldg % 4 == 0 && ((uintptr_t)grad % (4 * esize)) == 0 && aligned16(dx);
#define ANEMOI_ASMB(TT, VV)                                                                                                 \
  hipLaunchKernelGGL((assemble_nodes_backward_kernel<TT, VV>), dim3(flat_grid(numel / VV)), dim3(256), 0, st,                  \
                     static_cast<const TT*>(grad), ldg, dx, B, T, Ens, G, V)
  if (dtype == ANEMOI_F32) {
    if (vec) ANEMOI_ASMB(float, 4);
    else ANEMOI_ASMB(float, 1);
  } else {
    if (vec) ANEMOI_ASMB(bf16_t, 4);
    else ANEMOI_ASMB(bf16_t, 1);
  }
#undef ANEMOI_ASMB
  return trail::note(check_launch("anemoi_assemble_nodes_backward"), "anemoi_assemble_nodes_backward", "dx", ANEMOI_F32, dx,
                     V, (int64_t)B * T * Ens * G, V, st);
}

int anemoi_prognostic_residual_backward(const float* dy, int V_out, float* dx, int B, int T, int Ens, int64_t G, int V_in,
                                        const int32_t* src, anemoi_stream_t stream) {
  ANEMOI_REQUIRE(dy && dx && src, ANEMOI_ERR_INVALID, "anemoi_prognostic_residual_backward: null pointer");
  if (int rc = check_state_shape("anemoi_prognostic_residual_backward", B, T, Ens, G, V_in, V_out)) return rc;
  ANEMOI_REQUIRE(V_in <= RESIDUAL_BWD_MAX_V, ANEMOI_ERR_UNSUPPORTED,
                 "anemoi_prognostic_residual_backward: V_in %d > %d input variables", V_in, RESIDUAL_BWD_MAX_V);
  const int64_t slab = (int64_t)Ens * G * V_in;
  const int64_t numel = (int64_t)B * T * slab;
  if (numel == 0) return ANEMOI_OK;
  hipStream_t st = as_stream(stream);
  if (slab % 4 == 0 && aligned16(dx))
    hipLaunchKernelGGL(prognostic_residual_backward_kernel<4>,
                       dim3(flat_grid((int64_t)B * (T - 1) * (slab / 4) + (int64_t)B * slab)), dim3(256), 0, st, dy, V_out,
                       dx, B, T, slab, V_in, src);
  else
    hipLaunchKernelGGL(prognostic_residual_backward_kernel<1>, dim3(flat_grid(numel)), dim3(256), 0, st, dy, V_out, dx, B, T,
                       slab, V_in, src);
  return trail::note(check_launch("anemoi_prognostic_residual_backward"), "anemoi_prognostic_residual_backward", "dx",
                     ANEMOI_F32, dx, V_in, (int64_t)B * T * Ens * G, V_in, st);
}

}  // extern "C"
