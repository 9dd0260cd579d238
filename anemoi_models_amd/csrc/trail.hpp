// Launch trail: while a trail is armed on the calling thread, every exported entry point appends one 32-byte record per
// output buffer it wrote (digest / non-finite count / largest finite magnitude, include/anemoi_amd.h "Launch trail"),
// computed on the device, on the entry point's own stream, by the kernels of csrc/trail.hip.  Unarmed, trail::note() is one
// thread-local load and a branch.
#pragma once

#include "common.hpp"

namespace anemoi {
namespace trail {

struct State;

// the armed trail of the calling thread, or nullptr (thread_local like err_buf(): one trail per host thread)
inline State*& armed_state() {
  static thread_local State* s = nullptr;
  return s;
}

// out of line (csrc/trail.hip): appends the record of `ptr` ([rows, cols], leading dimension `ld` elements) to the armed trail
int note_armed(const char* who, const char* tag, int dtype, const void* ptr, int64_t ld, int64_t rows, int64_t cols,
               hipStream_t stream);

// The hook.  `rc` is the status of the launch(es) that wrote the buffer, usually check_launch(...) itself: a failed launch is
// passed through and nothing is recorded.  `who` is the entry point's name and `tag` names the output ("out", "lse", ...):
// the record is called "who:tag".  An entry point with several outputs chains: rc = note(rc, ...); return note(rc, ...).
inline int note(int rc, const char* who, const char* tag, int dtype, const void* ptr, int64_t ld, int64_t rows, int64_t cols,
                hipStream_t stream) {
  if (rc != ANEMOI_OK || armed_state() == nullptr) return rc;
  return note_armed(who, tag, dtype, ptr, ld, rows, cols, stream);
}

}  // namespace trail
}  // namespace anemoi
