// Output boundings of the TRAINING forward ("8f-12"): the op list of layers/bounding.py -- the one the
// inference kernel walks (csrc/elementwise.hip: bound_output_kernel) -- as a differentiable kernel pair, one launch each way
// for the whole bounding list instead of a gather, an activation and an index_put per module and their index-accumulation
// backwards.
//
// What the backward needs of the forward is a TAPE: per op the value it read, and for an op with a multiplier the multiplier it
// read -- (n_ops + n_multiplier_ops) floats per row, laid out [entry][row] so that the lanes of a wave (consecutive rows)
// write and read consecutive addresses.  No [rows, V_out] copy of the output is kept, and n_ops has no cap.
//
// Every element of y, of the tape and of dx is owned by one thread (the thread of its row): no atomics, no workspace, nothing
// read back, the same bits on every run.
#include "bound_op.hpp"
#include "common.hpp"
#include "trail.hpp"

namespace anemoi {

constexpr int BOUND_ROWS = 256;  // rows per workgroup = threads per workgroup

static inline unsigned row_grid(int64_t rows) {
  int64_t blocks = (rows + BOUND_ROWS - 1) / BOUND_ROWS;
  if (blocks > 256 * 16) blocks = 256 * 16;  // grid-stride the rest
  if (blocks < 1) blocks = 1;
  return (unsigned)blocks;
}

// Forward, in place on y [rows, V_out]: one thread per row walks the ops IN ORDER (y[c] = f_i(y[c]) * (mul >= 0 ? y[mul] : 1))
// and records what each op read.  Entry e of the tape is the e-th value read in this walk; an entry index at or past n_tape (a
// caller whose n_tape disagrees with op_mul) is never written.
__global__ __launch_bounds__(BOUND_ROWS) void bound_train_forward_kernel(float* __restrict__ y, int V_out, int64_t rows,
                                                                         int n_ops, const int32_t* __restrict__ op_col,
                                                                         const float* __restrict__ op_lo,
                                                                         const float* __restrict__ op_hi,
                                                                         const int32_t* __restrict__ op_mul,
                                                                         const float* __restrict__ op_slope,
                                                                         float* __restrict__ tape, int n_tape) {
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < rows;
       row += (int64_t)gridDim.x * blockDim.x) {
    float* yr = y + row * V_out;
    float* tr = tape + row;
    int e = 0;
    for (int i = 0; i < n_ops; ++i) {
      const int c = op_col[i];
      const float v = yr[c];
      if (e < n_tape) tr[(int64_t)e * rows] = v;
      ++e;
      float f = bound_op(v, op_lo[i], op_hi[i], op_slope[i]);
      const int m = op_mul[i];
      if (m >= 0) {
        const float ym = yr[m];
        if (e < n_tape) tr[(int64_t)e * rows] = ym;
        ++e;
        f *= ym;
      }
      yr[c] = f;
    }
  }
}

// Backward: dx [rows, V_out] from the incoming gradient g (read only) and the tape.  A workgroup owns BOUND_ROWS consecutive
// rows, i.e. ONE contiguous piece of g and dx: it copies the piece with 16-byte accesses (the untouched columns are done with
// that), then each thread walks the ops of its own row in REVERSE on dx:
//   go = dx[c];  dx[c] = go * f_i'(v) * ym;  dx[mul] += go * f_i(v)
// go is read before dx[c] is written because mul may be c itself (a fraction whose total is among its own variables).
// The barrier between the two phases orders the copy (other threads' stores to this thread's row) before the walk.
template <bool VEC4>
__global__ __launch_bounds__(BOUND_ROWS) void bound_train_backward_kernel(const float* __restrict__ g,
                                                                          float* __restrict__ dx, int V_out, int64_t rows,
                                                                          int n_ops, const int32_t* __restrict__ op_col,
                                                                          const float* __restrict__ op_lo,
                                                                          const float* __restrict__ op_hi,
                                                                          const int32_t* __restrict__ op_mul,
                                                                          const float* __restrict__ op_slope,
                                                                          const float* __restrict__ tape, int n_tape) {
  const int64_t n_pieces = (rows + BOUND_ROWS - 1) / BOUND_ROWS;
  for (int64_t piece = blockIdx.x; piece < n_pieces; piece += gridDim.x) {  // (uniform per workgroup: the barrier is safe)
    const int64_t row0 = piece * BOUND_ROWS;
    const int64_t n_rows = rows - row0 < BOUND_ROWS ? rows - row0 : BOUND_ROWS;
    const int64_t base = row0 * V_out, n = n_rows * V_out;
    int64_t done = 0;
    if constexpr (VEC4) {  // base is a multiple of 4 elements (BOUND_ROWS is), the buffers are 16-byte aligned
      const float4* g4 = reinterpret_cast<const float4*>(g + base);
      float4* d4 = reinterpret_cast<float4*>(dx + base);
      for (int64_t j = threadIdx.x; j < n / 4; j += BOUND_ROWS) d4[j] = g4[j];
      done = n / 4 * 4;
    }
    for (int64_t j = done + threadIdx.x; j < n; j += BOUND_ROWS) dx[base + j] = g[base + j];
    __syncthreads();
    const int64_t row = row0 + threadIdx.x;
    if (row < rows) {
      float* dr = dx + row * V_out;
      const float* tr = tape + row;
      int e = n_tape;
      for (int i = n_ops - 1; i >= 0; --i) {
        const int c = op_col[i], m = op_mul[i];
        float ym = 1.f;
        if (m >= 0) {
          --e;
          if (e >= 0) ym = tr[(int64_t)e * rows];
        }
        --e;
        const float v = e >= 0 ? tr[(int64_t)e * rows] : 0.f;
        const float lo = op_lo[i], hi = op_hi[i], s = op_slope[i];
        const float go = dr[c];
        const float d = bound_op_grad(v, lo, hi, s);
        const float gc = d == 1.f ? go : go * d;  // (inside the bounds: the bits of go)
        if (m >= 0) {
          dr[c] = gc * ym;
          dr[m] += go * bound_op(v, lo, hi, s);
        } else {
          dr[c] = gc;
        }
      }
    }
  }
}

static int check_bound_train(const char* who, const void* y, int V_out, int64_t rows, int n_ops, const int32_t* op_col,
                             const float* op_lo, const float* op_hi, const int32_t* op_mul, const float* op_slope,
                             const void* tape, int n_tape) {
  ANEMOI_REQUIRE(y && V_out > 0 && rows >= 0 && n_ops >= 0, ANEMOI_ERR_INVALID, "%s: bad argument", who);
  ANEMOI_REQUIRE(n_ops == 0 || (op_col && op_lo && op_hi && op_mul), ANEMOI_ERR_INVALID, "%s: null op list", who);
  ANEMOI_REQUIRE(n_ops == 0 || op_slope, ANEMOI_ERR_INVALID, "%s: null slope list", who);
  ANEMOI_REQUIRE(n_tape >= n_ops && n_tape <= 2 * (int64_t)n_ops, ANEMOI_ERR_INVALID,
                 "%s: n_tape %d is not n_ops + the number of multiplier ops (n_ops = %d)", who, n_tape, n_ops);
  ANEMOI_REQUIRE(n_tape == 0 || rows == 0 || tape, ANEMOI_ERR_INVALID, "%s: null tape", who);
  return ANEMOI_OK;
}

}  // namespace anemoi

using namespace anemoi;

extern "C" {

int anemoi_bound_output_train(float* y, int V_out, int64_t rows, int n_ops, const int32_t* op_col, const float* op_lo,
                              const float* op_hi, const int32_t* op_mul, const float* op_slope, float* tape, int n_tape,
                              anemoi_stream_t stream) {
  const char* who = "anemoi_bound_output_train";
  if (int rc = check_bound_train(who, y, V_out, rows, n_ops, op_col, op_lo, op_hi, op_mul, op_slope, tape, n_tape)) return rc;
  if (rows == 0 || n_ops == 0) return ANEMOI_OK;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(bound_train_forward_kernel, dim3(row_grid(rows)), dim3(BOUND_ROWS), 0, st, y, V_out, rows, n_ops, op_col,
                     op_lo, op_hi, op_mul, op_slope, tape, n_tape);
  int rc = trail::note(check_launch(who), who, "out", ANEMOI_F32, y, V_out, rows, V_out, st);
  return trail::note(rc, who, "tape", ANEMOI_F32, tape, rows, n_tape, rows, st);
}

int anemoi_bound_output_backward(const float* g, float* dx, int V_out, int64_t rows, int n_ops, const int32_t* op_col,
                                 const float* op_lo, const float* op_hi, const int32_t* op_mul, const float* op_slope,
                                 const float* tape, int n_tape, anemoi_stream_t stream) {
  const char* who = "anemoi_bound_output_backward";
  ANEMOI_REQUIRE(g != nullptr, ANEMOI_ERR_INVALID, "%s: null gradient", who);
  if (int rc = check_bound_train(who, dx, V_out, rows, n_ops, op_col, op_lo, op_hi, op_mul, op_slope, tape, n_tape)) return rc;
  const int64_t numel = rows * V_out;
  ANEMOI_REQUIRE(dx + numel <= g || g + numel <= dx, ANEMOI_ERR_INVALID, "%s: dx must not alias g", who);
  if (rows == 0) return ANEMOI_OK;
  hipStream_t st = as_stream(stream);
  if (aligned16(g) && aligned16(dx))
    hipLaunchKernelGGL(bound_train_backward_kernel<true>, dim3(row_grid(rows)), dim3(BOUND_ROWS), 0, st, g, dx, V_out, rows,
                       n_ops, op_col, op_lo, op_hi, op_mul, op_slope, tape, n_tape);
  else
    hipLaunchKernelGGL(bound_train_backward_kernel<false>, dim3(row_grid(rows)), dim3(BOUND_ROWS), 0, st, g, dx, V_out, rows,
                       n_ops, op_col, op_lo, op_hi, op_mul, op_slope, tape, n_tape);
  return trail::note(check_launch(who), who, "dx", ANEMOI_F32, dx, V_out, rows, V_out, st);
}

}  // extern "C"
