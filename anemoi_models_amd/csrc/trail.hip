// Launch trail (include/anemoi_amd.h "Launch trail"): per-output digests recorded on the device, on the caller's stream.
//
// One record per noted [rows, cols] matrix (leading dimension ld, elements of 1, 2 or 4 bytes):
//   digest    = sum_i (b_i + 1) * m(i)  mod 2^64,  i = r * cols + c,  b_i = the element's bits zero-extended,
//               m(i) = ((i + 1) * 0x9E3779B97F4A7C15 mod 2^64) | 1
//   nonfinite = number of NaN / +-Inf elements (float dtypes)
//   absmax    = bits of the largest finite |x| (bf16 widened to f32)
// All integer arithmetic: independent of the summation order, so the lane -> wave -> workgroup -> one-atomic-per-workgroup
// reduction below gives the same record on every run and on the host (tests/_trail_ref.py).
//
// The kernel is a bandwidth-bound read of the matrix.  A row is cut into 16-byte "slots" counted from the 16-byte boundary
// at or below the row's first element: a slot that lies wholly inside the row is one 16-byte load per lane, the (at most
// two) partial slots of a row are read element by element, so neither the padding between rows nor anything in front of an
// unaligned base is touched.  256-lane workgroups take `lpr` lanes per row (a power of two, so no division per slot) and
// 256 / lpr rows at a time; a row longer than 1024 slots is cut into units of 1024 slots (one 64-bit division per unit of
// >= 16 KiB, none otherwise).  All indexing is 64-bit.  The grid is capped at 2048 workgroups and strides over the units.
#include "trail.hpp"

#include <string>
#include <vector>

namespace anemoi {
namespace trail {

namespace {

constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;
constexpr int kBlock = 256;
constexpr int kUnitSlots = 1024;  // slots of one (row, unit) work item: 4 per lane at 256 lanes per row
constexpr int kMaxGrid = 2048;

struct Record {  // 32 bytes, zeroed on the stream before the kernel adds to it
  unsigned long long digest;
  unsigned long long nonfinite;
  uint32_t absmax;
  uint32_t pad;
  unsigned long long reserved;
};
static_assert(sizeof(Record) == 32, "trail record is 32 bytes");

struct Acc {
  uint64_t digest = 0;
  uint32_t nonfinite = 0;  // per lane: < 2^32 elements even for a 2^40-element matrix on the smallest grid that reads it
  uint32_t absmax = 0;
};

template <int ES>
struct Bits;
template <>
struct Bits<1> { typedef uint8_t type; };
template <>
struct Bits<2> { typedef uint16_t type; };
template <>
struct Bits<4> { typedef uint32_t type; };

// `mpre` = (i + 1) * kGolden of the element's logical index i
template <int ES, bool FLT>
__device__ __forceinline__ void fold(Acc& a, uint32_t b, uint64_t mpre) {
  a.digest += ((uint64_t)b + 1ull) * (mpre | 1ull);
  if constexpr (FLT) {
    const uint32_t mag = ES == 2 ? (b & 0x7fffu) << 16 : b & 0x7fffffffu;  // |x| as f32 bits: ordered like the value
    if (mag >= 0x7f800000u)
      ++a.nonfinite;
    else
      a.absmax = mag > a.absmax ? mag : a.absmax;
  }
}

template <int ES, bool FLT>
__global__ __launch_bounds__(kBlock) void digest_kernel(const void* base_, int64_t ld, int64_t rows, int64_t cols, int lpr_log2,
                                                        int64_t units_per_row, int64_t n_units, Record* rec) {
  typedef typename Bits<ES>::type T;
  constexpr int VEC = 16 / ES;
  const T* base = static_cast<const T*>(base_);
  const int lpr = 1 << lpr_log2;
  const int lane_in_row = threadIdx.x & (lpr - 1);
  const int row_in_block = threadIdx.x >> lpr_log2;
  const int64_t rows_per_block = kBlock >> lpr_log2;

  Acc a;
  for (int64_t u = blockIdx.x; u < n_units; u += gridDim.x) {
    int64_t rg = u, k = 0;
    if (units_per_row != 1) {
      rg = u / units_per_row;
      k = u - rg * units_per_row;
    }
    const int64_t r = rg * rows_per_block + row_in_block;
    if (r >= rows) continue;
    const T* row = base + r * ld;
    const int mis = (int)((reinterpret_cast<uintptr_t>(row) / ES) & (VEC - 1));  // elements past the 16-byte boundary below
    const int64_t nslots = (mis + cols + VEC - 1) / VEC;
    const int64_t jend = nslots < (k + 1) * kUnitSlots ? nslots : (k + 1) * kUnitSlots;
    const uint64_t i0 = (uint64_t)r * (uint64_t)cols;
    for (int64_t j = k * kUnitSlots + lane_in_row; j < jend; j += lpr) {
      const int64_t c0 = j * VEC - mis;  // logical column of the slot's first element (< 0 in an unaligned row's head slot)
      uint64_t mpre = (i0 + (uint64_t)c0 + 1ull) * kGolden;
      if (c0 >= 0 && c0 + VEC <= cols) {
        const uint4 t = *reinterpret_cast<const uint4*>(row + c0);
        const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          uint32_t b;
          if constexpr (ES == 4) b = w[e];
          else if constexpr (ES == 2) b = (w[e >> 1] >> (16 * (e & 1))) & 0xffffu;
          else b = (w[e >> 2] >> (8 * (e & 3))) & 0xffu;
          fold<ES, FLT>(a, b, mpre);
          mpre += kGolden;
        }
      } else {  // head / tail slot of the row: only the elements of the row itself are read
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const int64_t c = c0 + e;
          if (c >= 0 && c < cols) fold<ES, FLT>(a, (uint32_t)row[c], mpre);
          mpre += kGolden;
        }
      }
    }
  }

  // lane -> wave (cross-lane) -> workgroup (LDS) -> one set of integer atomics per workgroup
  unsigned long long d = a.digest, nf = a.nonfinite;
  uint32_t mx = a.absmax;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    d += __shfl_xor(d, off, 64);
    nf += __shfl_xor(nf, off, 64);
    const uint32_t o = (uint32_t)__shfl_xor((int)mx, off, 64);
    mx = o > mx ? o : mx;
  }
  __shared__ unsigned long long s_d[kBlock / 64], s_nf[kBlock / 64];
  __shared__ uint32_t s_mx[kBlock / 64];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_d[wave] = d;
    s_nf[wave] = nf;
    s_mx[wave] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kBlock / 64; ++w) {
      d += s_d[w];
      nf += s_nf[w];
      mx = s_mx[w] > mx ? s_mx[w] : mx;
    }
    if (d != 0) atomicAdd(&rec->digest, d);
    if (nf != 0) atomicAdd(&rec->nonfinite, nf);
    if (mx != 0) atomicMax(&rec->absmax, mx);
  }
}

int elem_size(int dtype) {
  switch (dtype) {
    case ANEMOI_F32: case ANEMOI_I32: return 4;
    case ANEMOI_BF16: return 2;
    case ANEMOI_U8: return 1;
    default: return 0;
  }
}

template <int ES, bool FLT>
void launch(const void* ptr, int64_t ld, int64_t rows, int64_t cols, Record* rec, hipStream_t stream) {
  constexpr int VEC = 16 / ES;
  if (ld == cols || rows == 1) {  // contiguous: one long row (the logical index r * cols + c is the same)
    cols *= rows;
    rows = 1;
    ld = cols;
  }
  const int64_t spr = (cols + 2 * (VEC - 1)) / VEC;  // slots per row, for any misalignment of the row start
  int lpr_log2 = 0;
  while (lpr_log2 < 8 && ((int64_t)1 << lpr_log2) < spr) ++lpr_log2;
  const int64_t rows_per_block = kBlock >> lpr_log2;
  const int64_t units_per_row = (spr + kUnitSlots - 1) / kUnitSlots;
  const int64_t n_units = (rows + rows_per_block - 1) / rows_per_block * units_per_row;
  const int grid = (int)(n_units < kMaxGrid ? n_units : kMaxGrid);
  hipLaunchKernelGGL((digest_kernel<ES, FLT>), dim3(grid), dim3(kBlock), 0, stream, ptr, ld, rows, cols, lpr_log2, units_per_row,
                     n_units, rec);
}

}  // namespace

struct Entry {
  std::string name;
  int dtype;
  int64_t rows, cols;
};

struct State {
  Record* records = nullptr;
  int64_t capacity = 0;
  int64_t dropped = 0;
  std::vector<Entry> entries;  // host-side metadata of the records written; kept after anemoi_trail_end for anemoi_trail_entry
};

static State& state() {
  static thread_local State s;
  return s;
}

int note_armed(const char* who, const char* tag, int dtype, const void* ptr, int64_t ld, int64_t rows, int64_t cols,
               hipStream_t stream) {
  State* st = armed_state();
  if (st == nullptr) return ANEMOI_OK;
  const int es = elem_size(dtype);
  ANEMOI_REQUIRE(who != nullptr, ANEMOI_ERR_INVALID, "anemoi_trail_note: null name");
  ANEMOI_REQUIRE(es != 0, ANEMOI_ERR_INVALID, "anemoi_trail_note(%s): dtype %d is none of f32/bf16/i32/u8", who, dtype);
  ANEMOI_REQUIRE(rows >= 0 && cols >= 0 && (rows <= 1 || ld >= cols), ANEMOI_ERR_INVALID,
                 "anemoi_trail_note(%s): bad shape rows=%lld cols=%lld ld=%lld", who, (long long)rows, (long long)cols,
                 (long long)ld);
  const bool empty = rows == 0 || cols == 0;
  ANEMOI_REQUIRE(empty || ptr != nullptr, ANEMOI_ERR_INVALID, "anemoi_trail_note(%s): null pointer", who);
  ANEMOI_REQUIRE(reinterpret_cast<uintptr_t>(ptr) % es == 0, ANEMOI_ERR_INVALID,
                 "anemoi_trail_note(%s): pointer not aligned to its element size", who);
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &cap) != hipSuccess) {
    (void)hipGetLastError();
    cap = hipStreamCaptureStatusNone;
  }
  ANEMOI_REQUIRE(cap == hipStreamCaptureStatusNone, ANEMOI_ERR_UNSUPPORTED,
                 "anemoi_trail_note(%s): a launch trail cannot record while the stream is being captured into a HIP graph "
                 "(eager execution only)", who);
  if ((int64_t)st->entries.size() >= st->capacity) {
    ++st->dropped;
    return ANEMOI_OK;
  }
  Record* rec = st->records + st->entries.size();
  hipError_t e = hipMemsetAsync(rec, 0, sizeof(Record), stream);
  if (e != hipSuccess) return fail(ANEMOI_ERR_LAUNCH, "anemoi_trail_note(%s): hipMemsetAsync: %s", who, hipGetErrorString(e));
  if (!empty) {
    switch (dtype) {
      case ANEMOI_F32: launch<4, true>(ptr, ld, rows, cols, rec, stream); break;
      case ANEMOI_I32: launch<4, false>(ptr, ld, rows, cols, rec, stream); break;
      case ANEMOI_BF16: launch<2, true>(ptr, ld, rows, cols, rec, stream); break;
      default: launch<1, false>(ptr, ld, rows, cols, rec, stream); break;
    }
    const int rc = check_launch("anemoi_trail_note");
    if (rc != ANEMOI_OK) return rc;
  }
  std::string name(who);
  if (tag != nullptr && tag[0] != 0) name.append(":").append(tag);
  st->entries.push_back(Entry{std::move(name), dtype, rows, cols});
  return ANEMOI_OK;
}

}  // namespace trail
}  // namespace anemoi

using namespace anemoi;

extern "C" {

int anemoi_trail_begin(void* records, int64_t capacity) {
  ANEMOI_REQUIRE(records != nullptr, ANEMOI_ERR_INVALID, "anemoi_trail_begin: null record buffer");
  ANEMOI_REQUIRE(capacity > 0, ANEMOI_ERR_INVALID, "anemoi_trail_begin: capacity %lld is not positive", (long long)capacity);
  ANEMOI_REQUIRE(trail::armed_state() == nullptr, ANEMOI_ERR_INVALID,
                 "anemoi_trail_begin: a trail is already armed on this thread (anemoi_trail_end it first)");
  trail::State& st = trail::state();
  st.records = static_cast<trail::Record*>(records);
  st.capacity = capacity;
  st.dropped = 0;
  st.entries.clear();
  trail::armed_state() = &st;
  return ANEMOI_OK;
}

int anemoi_trail_end(int64_t* n_written, int64_t* n_dropped) {
  ANEMOI_REQUIRE(trail::armed_state() != nullptr, ANEMOI_ERR_INVALID, "anemoi_trail_end: no trail is armed on this thread");
  trail::State& st = trail::state();
  trail::armed_state() = nullptr;
  if (n_written != nullptr) *n_written = (int64_t)st.entries.size();
  if (n_dropped != nullptr) *n_dropped = st.dropped;
  return ANEMOI_OK;
}

int anemoi_trail_entry(int64_t i, const char** name, int* dtype, int64_t* rows, int64_t* cols) {
  trail::State& st = trail::state();
  ANEMOI_REQUIRE(i >= 0 && i < (int64_t)st.entries.size(), ANEMOI_ERR_INVALID,
                 "anemoi_trail_entry: index %lld outside the %lld records of this thread's last trail", (long long)i,
                 (long long)st.entries.size());
  const trail::Entry& e = st.entries[(size_t)i];
  if (name != nullptr) *name = e.name.c_str();
  if (dtype != nullptr) *dtype = e.dtype;
  if (rows != nullptr) *rows = e.rows;
  if (cols != nullptr) *cols = e.cols;
  return ANEMOI_OK;
}

int anemoi_trail_note(const char* name, int dtype, const void* ptr, int64_t ld, int64_t rows, int64_t cols,
                      anemoi_stream_t stream) {
  return trail::note(ANEMOI_OK, name, nullptr, dtype, ptr, ld, rows, cols, as_stream(stream));
}

}  // extern "C"
