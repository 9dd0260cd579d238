// The column reduction [units, V] -> [groups, V] shared by the per-variable losses (csrc/losses.hip) and the ensemble scores
// (csrc/ensemble.hip): its geometry, the launcher of the one finish kernel, the host sequence of an entry point and the shape
// checks.  A unit is what one pass of a thread consumes: a row of the losses, a point (E member rows and one target row) of the
// ensemble scores.
//
// The determinism contract: no atomics; the workgroup count, the group and the contiguous chunk of units of every workgroup are
// functions of (n_groups, units_per_group, V, max_blocks) alone; every sum has a fixed order.
//
// Stage 1 (weighted_error_kernel, ensemble_score_kernel), V <= 256: thread t < L * V (L = 256 / V lanes) owns column t % V and
// lane t / V, so that one pass of the workgroup over L units reads the contiguous floats unit0 * V + t.  A thread adds the terms
// of its column in ascending unit order, then the L lanes of a column are summed through LDS in lane order.  V > 256: column
// tiles of 256, one unit per pass.  Workgroup k of group l writes its [V] partial to workspace[(l * W + k) * V].
// Stage 2: one thread per (l, v) adds the W partials in ascending workgroup order and applies `scale`.
//
// The two stage-1 kernels each write the tile loop and the lane sum out around their body.  A device frame that takes the body
// as a callable was tried and is not used: the body then runs through the optimiser once on its own before it is inlined, and
// the register counts of the ensemble kernels moved with it (profiles/loss_frame_refactor.md).
#pragma once

#include "common.hpp"
#include "trail.hpp"

namespace anemoi {
namespace column_reduce {

constexpr int64_t PER_BLOCK = 4096;  // (unit, column) pairs per workgroup before the workgroup count of a group saturates

static inline int lanes(int V) { return V <= 256 ? 256 / V : 1; }

// units of one workgroup's chunk: a multiple of the lanes (only the last chunk of a group has a ragged pass)
static inline int64_t chunk_units(int64_t units_per_group, int V, int64_t max_blocks) {
  int64_t blocks = (units_per_group * (int64_t)V + PER_BLOCK - 1) / PER_BLOCK;
  if (blocks > max_blocks) blocks = max_blocks;
  if (blocks < 1) blocks = 1;
  const int64_t l = lanes(V);
  const int64_t chunk = ((units_per_group + blocks - 1) / blocks + l - 1) / l * l;
  return chunk < l ? l : chunk;
}

static inline int64_t blocks(int64_t units_per_group, int V, int64_t max_blocks) {  // per group
  const int64_t chunk = chunk_units(units_per_group, V, max_blocks);
  const int64_t blocks = (units_per_group + chunk - 1) / chunk;
  return blocks < 1 ? 1 : blocks;
}

// Launches stage 2 (the kernel is defined once, in csrc/losses.hip: the library is built without relocatable device code).
void launch_finish(const float* partial, int64_t blocks, int64_t n_out, int V, float scale, float* out, hipStream_t st);

// What every entry point does around its stage 1: stage1(grid, units_per_group, chunk) launches it into `workspace`.  Returns the
// status of the launches; n_blocks receives the workgroups per group, or 0 when nothing was launched (a refused call, or no
// units: `out` is zeroed).  The trail notes stay with the entry point: "partials" is [n_groups * n_blocks, V] of `workspace`.
template <typename Stage1>
static int run(const char* who, int64_t units, int V, int64_t n_groups, int64_t max_blocks, float scale, float* out,
               float* workspace, int64_t workspace_floats, hipStream_t st, int64_t& n_blocks, Stage1 stage1) {
  n_blocks = 0;
  ANEMOI_REQUIRE(out != nullptr, ANEMOI_ERR_INVALID, "%s: null pointer (out)", who);
  const int64_t n_out = n_groups * V;
  if (units == 0) {
    hipError_t e = hipMemsetAsync(out, 0, n_out * sizeof(float), st);
    if (e != hipSuccess) return fail(ANEMOI_ERR_LAUNCH, "%s: %s", who, hipGetErrorString(e));
    return ANEMOI_OK;
  }
  const int64_t per_group = units / n_groups;
  const int64_t w = blocks(per_group, V, max_blocks), need = n_groups * w * V;
  ANEMOI_REQUIRE(workspace != nullptr && workspace_floats >= need, ANEMOI_ERR_INVALID,
                 "%s: workspace of %lld floats, %lld needed", who, (long long)workspace_floats, (long long)need);
  stage1(dim3((unsigned)w, (unsigned)n_groups), per_group, chunk_units(per_group, V, max_blocks));
  launch_finish(workspace, w, n_out, V, scale, out, st);
  n_blocks = w;
  return check_launch(who);
}

// The checks every entry point of the two families makes, in two parts: its own (the kind's parameter, the member count) stand
// between them.
static inline int check_operands(const char* who, int kind, int n_kinds, const float* pred, const float* target,
                                 const float* row_w) {
  ANEMOI_REQUIRE(pred && target && row_w, ANEMOI_ERR_INVALID, "%s: null pointer", who);
  ANEMOI_REQUIRE(kind >= 0 && kind < n_kinds, ANEMOI_ERR_INVALID, "%s: unknown kind %d", who, kind);
  return ANEMOI_OK;
}

static inline int check_shape(const char* who, int64_t rows, int V, int64_t G, int64_t n_groups) {
  ANEMOI_REQUIRE(rows >= 0 && V > 0 && G > 0 && n_groups > 0, ANEMOI_ERR_INVALID,
                 "%s: bad shape rows=%lld V=%d G=%lld n_groups=%lld", who, (long long)rows, V, (long long)G,
                 (long long)n_groups);
  ANEMOI_REQUIRE(G * (int64_t)V < ((int64_t)1 << 31), ANEMOI_ERR_UNSUPPORTED, "%s: G * V does not fit 31 bits", who);
  ANEMOI_REQUIRE(n_groups <= 65535, ANEMOI_ERR_UNSUPPORTED, "%s: %lld groups, at most 65535", who, (long long)n_groups);
  ANEMOI_REQUIRE(rows % (n_groups * G) == 0, ANEMOI_ERR_INVALID,
                 "%s: rows %lld is not a multiple of n_groups * G = %lld * %lld", who, (long long)rows, (long long)n_groups,
                 (long long)G);
  return ANEMOI_OK;
}

}  // namespace column_reduce
}  // namespace anemoi
