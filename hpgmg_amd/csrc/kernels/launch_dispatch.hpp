// launch_dispatch.hpp -- the two idioms every launcher of libhpgmg_hip.so shares, written once:
//   with_variant  a run-time int (operator variant, wave count, tile height, a variant * 3 + smoother key) becomes a template argument;
//                 only the listed values are instantiated, and a value outside the list launches nothing -- the caller records the refusal;
//   launch_lds    a kernel whose dynamic LDS exceeds the 64 KiB default is allowed its maximum once, then launched on g_stream.
#pragma once
#include <type_traits>
#include "common.hpp"

namespace hpgmg {

template <int... Vs> struct variant_list {};
// the recurring lists of operator variants (include/hpgmg_hip.h); a launcher with a list of its own spells it out at the call
constexpr variant_list<HPGMG_HIP_7PT_VC_HELMHOLTZ, HPGMG_HIP_7PT_VC_POISSON, HPGMG_HIP_7PT_CC> k7ptVariants{};
constexpr variant_list<HPGMG_HIP_FV4_VC_HELMHOLTZ, HPGMG_HIP_FV4_VC_POISSON> kFv4Variants{};
constexpr variant_list<HPGMG_HIP_FV4_VC_HELMHOLTZ, HPGMG_HIP_FV4_VC_POISSON, HPGMG_HIP_7PT_VC_HELMHOLTZ, HPGMG_HIP_7PT_VC_POISSON, HPGMG_HIP_7PT_CC> kDirectVariants{};   // stencil_direct_kernel
constexpr variant_list<HPGMG_HIP_27PT_CC, HPGMG_HIP_FV4_VC_HELMHOLTZ, HPGMG_HIP_FV4_VC_POISSON, HPGMG_HIP_7PT_VC_HELMHOLTZ, HPGMG_HIP_7PT_VC_POISSON, HPGMG_HIP_7PT_CC> kAllVariants{};
// variant * 3 + smoother for the three 7-point variants and a launcher's three smoothers (tail.hip, brick_visit.hip; each asserts that its smoother ids are 0, 1, 2)
constexpr variant_list<0, 1, 2, 3, 4, 5, 6, 7, 8> k7ptSmootherKeys{};
static_assert(HPGMG_HIP_7PT_VC_HELMHOLTZ == 0 && HPGMG_HIP_7PT_VC_POISSON == 1 && HPGMG_HIP_7PT_CC == 2, "k7ptSmootherKeys decodes key / 3 as a 7-point variant");

// Calls f(std::integral_constant<int, Vi>{}) for the listed value equal to `value` and stores what it returns (a launcher's status) in *status.
// Returns whether a value matched.  In f, `constexpr int V = v;` names the constant.
template <int... Vs, typename F>
inline bool with_variant(variant_list<Vs...>, int value, int *status, F &&f) {
  return ((value == Vs && ((void)(*status = f(std::integral_constant<int, Vs>{})), true)) || ...);
}
template <int... Vs, typename F>
inline bool with_variant(int value, int *status, F &&f) { return with_variant(variant_list<Vs...>{}, value, status, f); }
// the same for a flag: f(std::true_type{}) or f(std::false_type{})
template <typename F>
inline int with_bool(bool flag, F &&f) { return flag ? f(std::true_type{}) : f(std::false_type{}); }
// One flag per kernel instance: its MaxDynamicSharedMemorySize attribute has been set.
template <auto Kernel> inline bool lds_attribute_set = false;
template <auto Kernel, typename... Args>
inline int launch_lds(size_t max_lds, dim3 grid, dim3 block, size_t lds, const Args &...args) {
  if (!lds_attribute_set<Kernel>) { HPGMG_CHECK(hipFuncSetAttribute((const void *)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)max_lds)); lds_attribute_set<Kernel> = true; }
  hipLaunchKernelGGL(Kernel, grid, block, lds, g_stream, args...);
  return 0;
}

}  // namespace hpgmg
