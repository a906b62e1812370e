// What the extern "C" entry points of the chain families (siren_chain / modsiren / siren_gradient / modsiren_gradient /
// rff / gabor .hip) ask of their arguments, host side only.  One refusal grammar: every check names the argument it
// refuses, sets mri_last_error() through fail() and returns MRI_ERR_INVALID_ARGUMENT; an entry point runs them in the
// order it wants its arguments judged, the first refusal is the one reported.
//   "n = 5000000000 out of range"                       check_rows
//   "<name> is NULL", "<name> must be A-byte aligned"    check_buffer(s)
//   "<name>[l] is NULL", "<name>[l] must be ..."         check_pointers
//   "<what> needs a 16-byte aligned workspace of ..."    check_workspace
//   "<what>: <name> is not finite"                       check_finite
// A family states its shape rule once, in a check_<family>_shape(what, ...) of its own file, which its *_supported
// function and every one of its entry points call.
#pragma once
#include <algorithm>
#include <cmath>
#include <initializer_list>

#include "common.h"

namespace mri {

#define MRI_CHECK(call)              \
  do {                               \
    if (int rc_ = (call)) return rc_; \
  } while (0)

// for check_buffers / check_pointers: presence only (the kernels read these float by float)
constexpr int kAnyAlignment = 1;

// the grid of a persistent tile loop: one workgroup per CU, fewer when the tiles run out
inline int persistent_blocks(int64_t n, int per_tile) { return (int)std::min<int64_t>(ceil_div(n, per_tile), 256); }

inline int check_rows(int64_t n) {
  MRI_REQUIRE(n >= 0 && n < (1ll << 31), "n = %lld out of range", (long long)n);
  return MRI_OK;
}

// ... of a loss-mode forward: n rows of a batch of n_total, whose mean the gradient is scaled by 1 / grad_divisor
inline int check_batch_slice(int64_t n, int64_t n_total, float grad_divisor) {
  MRI_CHECK(check_rows(n));
  MRI_REQUIRE(n_total >= n, "n_total = %lld is less than n = %lld (n is a slice of the batch)", (long long)n_total,
              (long long)n);
  MRI_REQUIRE(grad_divisor > 0.f, "grad_divisor = %g is not positive", (double)grad_divisor);
  return MRI_OK;
}

inline int check_finite(const char* what, const char* name, float v) {
  MRI_REQUIRE(std::isfinite(v), "%s: %s is not finite", what, name);
  return MRI_OK;
}

inline int check_buffer(const char* name, const void* p, int alignment) {
  MRI_REQUIRE(p, "%s is NULL", name);
  MRI_REQUIRE(aligned_to(p, alignment), "%s must be %d-byte aligned", name, alignment);
  return MRI_OK;
}

struct NamedBuffer {
  const char* name;
  const void* p;
};
inline int check_buffers(std::initializer_list<NamedBuffer> buffers, int alignment) {
  for (const NamedBuffer& b : buffers) MRI_CHECK(check_buffer(b.name, b.p, alignment));
  return MRI_OK;
}

// entries [first, first + count) of each named array of device pointers (float* const*, const float* const*)
inline int check_pointers(std::initializer_list<NamedBuffer> arrays, int first, int count, int alignment) {
  for (const NamedBuffer& a : arrays) {
    MRI_REQUIRE(a.p, "%s is NULL", a.name);
    const void* const* const entry = static_cast<const void* const*>(a.p);
    for (int l = first; l < first + count; ++l) {
      MRI_REQUIRE(entry[l], "%s[%d] is NULL", a.name, l);
      MRI_REQUIRE(aligned_to(entry[l], alignment), "%s[%d] must be %d-byte aligned", a.name, l, alignment);
    }
  }
  return MRI_OK;
}

// `need` bytes as `sizer` (the entry point's *_workspace_bytes function) counts them; need == 0 passes any workspace
inline int check_workspace(const char* what, const char* sizer, const void* workspace, int64_t workspace_bytes,
                           int64_t need) {
  if (need == 0) return MRI_OK;
  const char* const wrong = !workspace                   ? "workspace is NULL"
                            : workspace_bytes < need     ? "workspace is short of that"
                            : !aligned_to(workspace, 16) ? "workspace must be 16-byte aligned"
                                                         : nullptr;
  MRI_REQUIRE(!wrong, "%s needs a 16-byte aligned workspace of %lld bytes (%s): %s, got %lld bytes", what,
              (long long)need, sizer, wrong, (long long)workspace_bytes);
  return MRI_OK;
}

// what the coordinate-gradient entry points ask of n, x, y and dydx (n = 0 passes: the caller returns then)
inline int check_gradient_io(const float* x, int64_t n, const float* y, const float* dydx) {
  MRI_CHECK(check_rows(n));
  if (n == 0) return MRI_OK;
  return check_buffers({{"x", x}, {"y", y}, {"dydx", dydx}}, 4);
}

}  // namespace mri
