// layout_debug.h — what the mpn_debug_* pass-throughs to the layout, packing and halo kernels share (debug flavour only; DESIGN.md
// section 13.17): layout_debug.hip and the entries that sit beside a file-local kernel in pipeline.hip, graph_pool.hip and resnet.hip.
// Every buffer comes with its size in BYTES; one smaller than the footprint of its layout, or off the alignment the kernel's vector
// accesses need, is refused before anything is launched — a layout mistake of a test becomes MPN_EINVAL, never an access outside the
// test's allocation.
#pragma once
#include <cstdint>

#include "mpn_internal.h"

#ifdef MPN_DEBUG_HOOKS
namespace mpn {
inline bool ldbg_short(const char *fn, const char *name, size_t have, size_t want) {
  if (have >= want) return false;
  set_error("%s: %s holds %zu bytes, the launch's footprint is %zu", fn, name, have, want);
  return true;
}
inline bool ldbg_misaligned(const char *fn, const char *name, const void *ptr, size_t bytes) {
  if ((reinterpret_cast<uintptr_t>(ptr) & (bytes - 1)) == 0) return false;
  set_error("%s: invalid argument: %s must be %zu-byte aligned", fn, name, bytes);
  return true;
}
}  // namespace mpn
// a non-null buffer of `have` bytes that the launch touches `want` bytes of, through accesses `align` bytes wide
#define LDBG_BUF(buf, have, want, align)                                                              \
  do {                                                                                                \
    MPN_CHECK_ARG((buf) != nullptr);                                                                  \
    if (::mpn::ldbg_misaligned(__func__, #buf, (buf), (size_t)(align))) return MPN_EINVAL;            \
    if (::mpn::ldbg_short(__func__, #buf, (size_t)(have), (size_t)(want))) return MPN_EINVAL;         \
  } while (0)
#endif
