// The host-side vocabulary of the control kernels (xde_cde.hip, xde_cdegrad.hip, xde_spline.hip): what an element is, the grid of a
// count of work items, the natural control's private method code, the refusal rules of their entry points — each rule and its message
// stated once — and the dispatch from a dtype code and run-time flags to a kernel instantiation.
#pragma once

#include <initializer_list>
#include <type_traits>

#include "xde_common.hpp"

namespace xde {

// CdeArgs::method / GradArgs::method of the natural control (xde_hip_spline.h): it has entry points of its own, so no public method code
// reaches it
constexpr int kMethodNatural = 3;
static_assert(kMethodNatural != XDE_HISTORY_LINEAR && kMethodNatural != XDE_HISTORY_CUBIC && kMethodNatural != XDE_HISTORY_BEZIER,
              "the natural control's private method code must be none of the XDE_HISTORY_* codes");

inline int elem_size(int dtype) { return dtype == XDE_F32 ? 4 : 8; }
inline int vec_width(int dtype) { return 16 / elem_size(dtype); }  // elements of a 16-byte vector
inline bool misaligned(const void* p, int dtype) { return (reinterpret_cast<uintptr_t>(p) & uintptr_t(elem_size(dtype) - 1)) != 0; }

inline int pow2ceil(int x) {
  int r = 1;
  while (r < x) r <<= 1;
  return r;
}

// workgroups of a grid-stride launch over `work` items, one per lane
inline unsigned grid_for(int64_t work) {
  const int64_t blocks = (work + kBlock - 1) / kBlock;
  return static_cast<unsigned>(blocks > grid_cap() ? grid_cap() : blocks);
}

// The refusals of one entry point, as a chain of rules in the order they are checked: the first rule that is broken sets `rc` and the
// thread's error message, every rule after it is skipped.
using Ptrs = std::initializer_list<const void*>;
struct ArgCheck {
  const char* who;
  int rc = XDE_OK;

  ArgCheck& refuse(const std::string& what) {
    rc = fail(XDE_EBADARG, who + what);
    return *this;
  }
  // a cotangent pair of which one may be missing
  ArgCheck& either(const void* a, const void* b) { return !rc && !a && !b ? refuse(kNull) : *this; }
  // (an operand that may be null is not listed here)
  ArgCheck& not_null(Ptrs required) {
    if (!rc)
      for (const void* p : required)
        if (!p) return refuse(kNull);
    return *this;
  }
  // `names`: the sizes as the message prints them ("B, H, C")
  ArgCheck& sizes(const char* names, std::initializer_list<int64_t> values) {
    if (!rc)
      for (int64_t v : values)
        if (v < 1) return refuse(std::string(": bad sizes (need ") + names + " >= 1)");
    return *this;
  }
  ArgCheck& knots(int Tn) { return !rc && Tn < 2 ? refuse(": bad sizes (need Tn >= 2)") : *this; }
  ArgCheck& dtype(int dtype) { return !rc && dtype != XDE_F32 && dtype != XDE_F64 ? refuse(": bad dtype") : *this; }
  ArgCheck& time_dtype(int dtype) { return !rc && dtype != XDE_F32 && dtype != XDE_F64 ? refuse(": bad time_dtype") : *this; }
  // a public entry point: the natural control's private code is no method of it (checked before anything else)
  ArgCheck& public_method(int method) { return !rc && method == kMethodNatural ? refuse(kUnknownMethod) : *this; }
  ArgCheck& control_method(int method) {
    if (rc) return *this;
    if (method == XDE_HISTORY_BEZIER)
      return refuse(": XDE_HISTORY_BEZIER is not a control path (its four-row window does not pass through the data); "
                    "XDE_HISTORY_LINEAR and XDE_HISTORY_CUBIC are served");
    return method != XDE_HISTORY_LINEAR && method != XDE_HISTORY_CUBIC && method != kMethodNatural ? refuse(kUnknownMethod) : *this;
  }
  // (a null operand is aligned: it passed not_null, or may be null)
  ArgCheck& aligned(Ptrs operands, int dtype) {
    if (!rc)
      for (const void* p : operands)
        if (misaligned(p, dtype)) return refuse(": operand not aligned to its element type");
    return *this;
  }
  ArgCheck& time_aligned(const void* t_dev, int time_dtype) {
    return !rc && misaligned(t_dev, time_dtype) ? refuse(": t_dev not aligned to its element type") : *this;
  }
  static constexpr const char *kNull = ": null pointer", *kUnknownMethod = ": unknown method";
};

// what the launches at one time (the contractions, the control's cotangent) take besides their operands, in the headers' order
struct TimedCall {
  const void* t_dev;
  double t_host;
  int time_dtype;
  int64_t B;
  int H, C, Tn, method, dtype;
  void* stream;
};

// The two ladders of the entry points that enqueue.  `required` and `optional` (may be null) are the operands of `dtype`.
// rows on a knot grid (the spline build, the gather and their transposes); `names`, `sizes`: as ArgCheck::sizes takes them
inline int check_rows(ArgCheck no, Ptrs required, Ptrs optional, const char* names, std::initializer_list<int64_t> sizes, int Tn,
                      int dtype) {
  return no.not_null(required).sizes(names, sizes).knots(Tn).dtype(dtype).aligned(required, dtype).aligned(optional, dtype).rc;
}
inline int check_timed(ArgCheck no, Ptrs required, const TimedCall& c) {
  return no.not_null(required).sizes("B, H, C", {c.B, c.H, c.C}).knots(c.Tn).dtype(c.dtype).time_dtype(c.time_dtype)
      .control_method(c.method).aligned(required, c.dtype).time_aligned(c.t_dev, c.time_dtype).rc;
}

// dtype code -> fn(TypeTag<float>{}) or fn(TypeTag<double>{}); a run-time bool -> fn(std::true_type{}) or fn(std::false_type{}).  A
// generic lambda takes the tag and names the kernel instantiation with it, so only the combinations the lambdas spell out exist.
template <typename T>
struct TypeTag {
  using type = T;
};
template <typename Fn>
void with_dtype(int dtype, Fn&& fn) {
  if (dtype == XDE_F32) fn(TypeTag<float>{});
  else fn(TypeTag<double>{});
}
template <typename Fn>
void with_flag(bool flag, Fn&& fn) {
  if (flag) fn(std::true_type{});
  else fn(std::false_type{});
}

}  // namespace xde
