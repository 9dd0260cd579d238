// Host side of the thin Linear (csrc/gemm_thin.hip): argument validation, refusal and launch geometry.  No device call
// in here, so that tools/thin_plan_check.cpp can run it under the host sanitizers without a GPU.
#pragma once

#include "common.hpp"

namespace anemoi {
namespace thin {

// How the weight sits in the four waves' registers.
//   ROWS:   every wave holds all of W and takes its own 16-row blocks;
//   NSPLIT: wave w holds the N / 4 output columns from w N / 4 on, the four waves share a row block;
//   KSPLIT: wave w holds the K / 4 input columns from w K / 4 on, the four partial sums are added through LDS in wave order.
enum Mode { MODE_ROWS = 0, MODE_NSPLIT = 1, MODE_KSPLIT = 2 };

struct Shape {
  int n, k, mode;
  int blocks_per_cu;  // resident workgroups per CU that the kernel's register use allows
};

// the kernel table of gemm_thin.hip, in its order
constexpr Shape SHAPES[] = {
    {256, 64, MODE_ROWS, 1}, {64, 256, MODE_ROWS, 1}, {256, 256, MODE_NSPLIT, 1}, {80, 1024, MODE_KSPLIT, 1}, {16, 1024, MODE_KSPLIT, 1},
    {16, 256, MODE_ROWS, 1},  {256, 128, MODE_NSPLIT, 1},
};
constexpr int N_SHAPES = (int)(sizeof(SHAPES) / sizeof(SHAPES[0]));

struct Plan {
  int shape;           // index into SHAPES
  int pair;            // bf16 stores of 16 bytes: two 16-column MFMA tiles interleaved per lane (ROWS / NSPLIT, bf16 out)
  int64_t row_blocks;  // ceil(M / 16)
  unsigned grid_x, grid_y;
};

inline bool mult(int64_t v, int64_t m) { return v % m == 0; }

// Status the entry point returns before its first launch; fills `p` on ANEMOI_OK.  `cus`: compute units of the device.
inline int plan(const anemoi_linear_thin_args* a, int cus, Plan& p) {
  ANEMOI_REQUIRE(a != nullptr, ANEMOI_ERR_INVALID, "anemoi_linear_thin: null argument block");
  ANEMOI_REQUIRE(a->struct_bytes == (int64_t)sizeof(anemoi_linear_thin_args), ANEMOI_ERR_INVALID,
                 "anemoi_linear_thin: argument block out of sync with the library (%lld bytes, expected %lld)",
                 (long long)a->struct_bytes, (long long)sizeof(anemoi_linear_thin_args));
  ANEMOI_REQUIRE(a->out_dtype == ANEMOI_BF16 || a->out_dtype == ANEMOI_F32, ANEMOI_ERR_INVALID,
                 "anemoi_linear_thin: out_dtype %d", a->out_dtype);
  ANEMOI_REQUIRE(a->M >= 0 && a->N > 0 && a->K > 0 && a->batch >= 0, ANEMOI_ERR_INVALID,
                 "anemoi_linear_thin: M=%lld N=%d K=%d batch=%d", (long long)a->M, a->N, a->K, a->batch);
  const int batch = a->batch > 1 ? a->batch : 1;
  const bool stats_only = a->stats_out != nullptr;
  const bool fold = a->colsum != nullptr || a->stats != nullptr;
  int shape = -1;
  for (int i = 0; i < N_SHAPES; ++i)
    if (SHAPES[i].n == a->N && SHAPES[i].k == a->K) shape = i;
  ANEMOI_REQUIRE(shape >= 0, ANEMOI_ERR_UNSUPPORTED, "anemoi_linear_thin: no register-resident kernel for N=%d K=%d", a->N, a->K);
  ANEMOI_REQUIRE(a->M > 0, ANEMOI_ERR_UNSUPPORTED, "anemoi_linear_thin: M = 0");
  ANEMOI_REQUIRE(a->M <= ((int64_t)1 << 34), ANEMOI_ERR_UNSUPPORTED, "anemoi_linear_thin: M=%lld (more than 2^30 row blocks)", (long long)a->M);
  ANEMOI_REQUIRE(batch == 1 || (SHAPES[shape].mode != MODE_KSPLIT && !fold && !stats_only), ANEMOI_ERR_UNSUPPORTED,
                 "anemoi_linear_thin: batch=%d with a K-split shape, a LayerNorm fold or statistics", batch);
  ANEMOI_REQUIRE(batch <= 65535, ANEMOI_ERR_UNSUPPORTED, "anemoi_linear_thin: batch=%d", batch);
  ANEMOI_REQUIRE(!(stats_only && a->residual != nullptr), ANEMOI_ERR_UNSUPPORTED,
                 "anemoi_linear_thin: statistics only with a residual");
  ANEMOI_REQUIRE((a->colsum != nullptr) == (a->stats != nullptr), ANEMOI_ERR_INVALID,
                 "anemoi_linear_thin: the LayerNorm fold needs both colsum and stats");
  ANEMOI_REQUIRE(a->x != nullptr && a->w != nullptr && (stats_only || a->y != nullptr), ANEMOI_ERR_INVALID,
                 "anemoi_linear_thin: null pointer");
  const int64_t width_x = (int64_t)a->K, width_y = (int64_t)a->N;
  ANEMOI_REQUIRE(a->ldx >= width_x && (stats_only || a->ldy >= width_y) && (a->residual == nullptr || a->ldr >= width_y),
                 ANEMOI_ERR_INVALID, "anemoi_linear_thin: leading dimension below the row width");
  if (batch > 1) {
    ANEMOI_REQUIRE(a->stride_x >= 0 && a->stride_w >= 0 && a->stride_y >= 0 && a->stride_r >= 0, ANEMOI_ERR_INVALID,
                   "anemoi_linear_thin: negative problem stride");
    ANEMOI_REQUIRE(mult(a->stride_x, 8) && mult(a->stride_w, 8), ANEMOI_ERR_INVALID,
                   "anemoi_linear_thin: stride_x / stride_w must be multiples of 8 elements");
  }
  const int out_mult = a->out_dtype == ANEMOI_BF16 ? 8 : 4;
  ANEMOI_REQUIRE(aligned16(a->x) && aligned16(a->w) && mult(a->ldx, 8), ANEMOI_ERR_INVALID,
                 "anemoi_linear_thin: x / w must be 16-byte aligned, ldx a multiple of 8");
  ANEMOI_REQUIRE(stats_only || (aligned16(a->y) && mult(a->ldy, out_mult) && (batch == 1 || mult(a->stride_y, out_mult))),
                 ANEMOI_ERR_INVALID, "anemoi_linear_thin: y must be 16-byte aligned, ldy / stride_y multiples of %d", out_mult);
  ANEMOI_REQUIRE(a->residual == nullptr || (aligned16(a->residual) && mult(a->ldr, 8) && (batch == 1 || mult(a->stride_r, 8))),
                 ANEMOI_ERR_INVALID, "anemoi_linear_thin: residual must be 16-byte aligned, ldr / stride_r multiples of 8");
  ANEMOI_REQUIRE(aligned16(a->bias) && aligned16(a->colsum) && ((uintptr_t)a->stats & 7) == 0 && ((uintptr_t)a->stats_out & 7) == 0,
                 ANEMOI_ERR_INVALID, "anemoi_linear_thin: bias / colsum must be 16-byte aligned, stats 8-byte aligned");
  ANEMOI_REQUIRE(cus > 0, ANEMOI_ERR_INVALID, "anemoi_linear_thin: %d compute units", cus);

  const Shape& s = SHAPES[shape];
  p.shape = shape;
  const int tiles_per_wave = s.n / 16 / (s.mode == MODE_NSPLIT ? 4 : 1);
  p.pair = (s.mode != MODE_KSPLIT && tiles_per_wave % 2 == 0 && a->out_dtype == ANEMOI_BF16 && !stats_only) ? 1 : 0;
  p.row_blocks = (a->M + 15) / 16;
  // work items of one problem: a ROWS workgroup takes four row blocks at a time (one per wave), the other modes one
  const int64_t items = s.mode == MODE_ROWS ? (p.row_blocks + 3) / 4 : p.row_blocks;
  int64_t per_problem = ((int64_t)cus * s.blocks_per_cu + batch - 1) / batch;
  if (per_problem < 1) per_problem = 1;
  p.grid_x = (unsigned)(items < per_problem ? items : per_problem);
  p.grid_y = (unsigned)batch;
  return ANEMOI_OK;
}

}  // namespace thin
}  // namespace anemoi
