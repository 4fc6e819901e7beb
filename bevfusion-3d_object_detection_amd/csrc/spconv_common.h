// spconv_common.h -- what the sparse-convolution units (spconv_rulebook.hip, spconv.hip, spconv_wgrad.hip) share: the vector
// operand types and the helper that turns the run-time choice of a kernel instantiation into compile-time constants (the
// convolution geometry is the rulebook unit's alone and lives there).  Everything sits in an anonymous namespace.
#pragma once
#include "common.h"

#include <type_traits>

namespace bfhip {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// ---- run-time choice of a kernel instantiation -> compile-time constants.  `f` is a generic lambda; it is called exactly
// once, with std::integral_constants whose ::value name the instantiation, so every kernel is launched from one statement:
//   dispatch_tile(NT, R, io16, [&](auto nt, auto r, auto io) { hipLaunchKernelGGL((kernel<nt.value, r.value, io.value>), ...); });
// The callers validate their arguments first: a value outside the listed ones calls nothing.
template <int... Vs, typename F>
inline void dispatch_int(int v, F &&f) {
  (void)((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

// rows per wave / 16 (R) and the feature storage (IO16: bf16, else fp32): the weight gradient's choice
template <typename F>
inline void dispatch_row_tile(int R, bool io16, F &&f) {
  dispatch_int<1, 2, 4>(R, [&](auto r) { io16 ? f(r, std::true_type{}) : f(r, std::false_type{}); });
}

// ... and the 16-column tiles of the output (NT) on top of it: the gather-GEMMs' choice
template <typename F>
inline void dispatch_tile(int NT, int R, bool io16, F &&f) {
  dispatch_int<1, 2, 4, 8>(NT, [&](auto nt) { dispatch_row_tile(R, io16, [&](auto r, auto io) { f(nt, r, io); }); });
}

}  // namespace
}  // namespace bfhip
