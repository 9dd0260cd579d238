// The multi-tensor frame shared by the optimizer step (csrc/optim.hip) and the weight average (csrc/average.hip): the launch
// geometry, the chunk accessors, the checks every list entry point makes and the walk over a list in frames.
//
// One launch serves up to OPT_MAX_TENSORS tensors whose device pointers, lengths and chunk prefix counts travel BY VALUE in the
// kernel argument block (HIP's 4 KB limit fixes OPT_MAX_TENSORS): there is no table in device memory, so nothing on the host has
// to stay alive for a graph replay.  A tensor is cut into chunks of OPT_CHUNK elements; workgroup b owns the (tensor, chunk)
// pair found by a binary search of b in the prefix counts -- scalar loads from the argument block, wave-uniform.  A longer list
// is several launches.  Within a chunk, pass u of thread t owns the four elements (u * 256 + t) * 4 .. + 3: one 16-byte access
// when every pointer of the tensor is 16-byte aligned, else (a view at an odd element offset) up to four dword accesses of the
// SAME elements -- the arithmetic and its order do not know which.  The ragged tail of a tensor is the last, short group.
#pragma once

#include "common.hpp"
#include "trail.hpp"

namespace anemoi {

constexpr int OPT_MAX_TENSORS = 88;
constexpr int OPT_CHUNK = 4096;
constexpr int OPT_PASSES = OPT_CHUNK / (256 * 4);
constexpr int OPT_MAX_GROUPS = 32;  // parameter groups per launch of a one-wave scalar kernel (one thread each)

struct OptFrame {
  int32_t n;                                 // tensors of this launch
  int32_t chunk_start[OPT_MAX_TENSORS + 1];  // workgroups before tensor i; [n] = the grid
  int64_t numel[OPT_MAX_TENSORS];
};

// the tensor of workgroup b: the last i with chunk_start[i] <= b (empty tensors never enter a frame, so the counts rise strictly)
__device__ __forceinline__ int opt_find(const OptFrame& f, int b) {
  int lo = 0, hi = f.n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (f.chunk_start[mid] <= b) lo = mid;
    else hi = mid;
  }
  return lo;
}

// Elements i .. i + 3 of a chunk of `cnt` elements; those at and behind cnt read as 0.  FULL (a whole chunk of a 16-byte
// aligned tensor: a workgroup-uniform choice) is straight-line 16-byte code; the other form serves tails and odd views.
template <bool FULL>
__device__ __forceinline__ void opt_load4(const float* __restrict__ base, int i, int cnt, bool vec, float (&r)[4]) {
  if (FULL || (vec && i + 4 <= cnt)) {
    VecIO<float, 4>::load(base + i, r);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = i + k < cnt ? base[i + k] : 0.f;
  }
}

template <bool FULL>
__device__ __forceinline__ void opt_store4(float* __restrict__ base, int i, int cnt, bool vec, const float (&r)[4]) {
  if (FULL || (vec && i + 4 <= cnt)) {
    VecIO<float, 4>::store(base + i, r);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i + k < cnt) base[i + k] = r[k];
  }
}

static inline int64_t opt_chunks(int64_t numel) { return (numel + OPT_CHUNK - 1) / OPT_CHUNK; }

// The checks every list entry point makes before any launch.  `arrays` / `names`: the host pointer arrays the entry point
// reads, each n_tensors device pointers, non-null wherever the length is not 0.
static int opt_check_list(const char* who, const anemoi_multi_tensor_args* a, int n_arrays, void* const* const* arrays,
                          const char* const* names) {
  ANEMOI_REQUIRE(a != nullptr, ANEMOI_ERR_INVALID, "%s: null argument block", who);
  ANEMOI_REQUIRE(a->struct_bytes == (int64_t)sizeof(anemoi_multi_tensor_args), ANEMOI_ERR_INVALID,
                 "%s: argument block of %lld bytes, this library expects %lld (header / library out of sync)", who,
                 (long long)a->struct_bytes, (long long)sizeof(anemoi_multi_tensor_args));
  ANEMOI_REQUIRE(a->n_tensors >= 0, ANEMOI_ERR_INVALID, "%s: negative n_tensors %lld", who, (long long)a->n_tensors);
  if (a->n_tensors == 0) return ANEMOI_OK;
  ANEMOI_REQUIRE(a->numel != nullptr, ANEMOI_ERR_INVALID, "%s: null pointer (numel)", who);
  for (int k = 0; k < n_arrays; ++k)
    ANEMOI_REQUIRE(arrays[k] != nullptr, ANEMOI_ERR_INVALID, "%s: null pointer (%s)", who, names[k]);
  for (int64_t i = 0; i < a->n_tensors; ++i) {
    ANEMOI_REQUIRE(a->numel[i] >= 0, ANEMOI_ERR_INVALID, "%s: negative numel[%lld] = %lld", who, (long long)i,
                   (long long)a->numel[i]);
    if (a->numel[i] == 0) continue;
    for (int k = 0; k < n_arrays; ++k)
      ANEMOI_REQUIRE(arrays[k][i] != nullptr, ANEMOI_ERR_INVALID, "%s: null pointer (%s[%lld])", who, names[k], (long long)i);
  }
  return ANEMOI_OK;
}

// Walks the list in frames of at most OPT_MAX_TENSORS non-empty tensors (and fewer than 2^31 chunks) and calls
// launch(frame, index of each frame tensor in the list, chunks of the list before the frame).
template <typename Launch>
static void opt_for_each_frame(const anemoi_multi_tensor_args* a, Launch launch) {
  OptFrame f;
  int64_t idx[OPT_MAX_TENSORS];
  int64_t chunks_before = 0, frame_chunks = 0;
  f.n = 0;
  f.chunk_start[0] = 0;
  for (int64_t i = 0; i <= a->n_tensors; ++i) {
    const bool end = i == a->n_tensors;
    const int64_t c = end ? 0 : opt_chunks(a->numel[i]);
    if (!end && c == 0) continue;
    if (f.n > 0 && (end || f.n == OPT_MAX_TENSORS || frame_chunks + c > 0x7fffffff)) {
      launch(f, idx, chunks_before);
      chunks_before += frame_chunks;
      frame_chunks = 0;
      f.n = 0;
    }
    if (end) break;
    idx[f.n] = i;
    f.numel[f.n] = a->numel[i];
    frame_chunks += c;
    f.chunk_start[++f.n] = (int32_t)frame_chunks;
  }
}

}  // namespace anemoi
