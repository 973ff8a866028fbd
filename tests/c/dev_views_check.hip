// dev_views_check.hip — which engine's kernels can name which device fields (simgrid_amd/csrc/lmm_dev.hpp), checked by
// the compiler alone: host-side static_asserts, compiled with the Makefile's flags and -fsyntax-only by
// tests/test_dev_views.py.  Dev is the system and the max-min state the engines share; FrDev adds the frontier
// engine's eight fields, FbDev FairBottleneck's nineteen, and neither view has the other's.
#include "../../simgrid_amd/csrc/lmm_dev.hpp"

#include <cstddef>
#include <type_traits>

using namespace lmmdev;

#define HAS_MEMBER(name)                                                                     \
  template <class T, class = void> struct has_##name : std::false_type {};                   \
  template <class T> struct has_##name<T, std::void_t<decltype(&T::name)>> : std::true_type {};

#define FR_FIELDS(X) X(csr_cs) X(pvb) X(key32) X(vslot) X(minfl) X(fq_a) X(fq_b) X(fq_n)
#define FB_FIELDS(X)                                                                                               \
  X(fixr) X(vtmp) X(vst) X(vstb) X(nch) X(ch_cnst) X(ch_beg) X(c_ch) X(pcnt) X(pacc) X(erased) X(xnb) X(xmin) X(fbd) \
  X(fb_long) X(vperm) X(csc_vp) X(mu_p) X(hprog)
// (what stays in Dev: a sample of every group, the round engine's five mode fields among them)
#define DEV_FIELDS(X)                                                                                             \
  X(nV) X(nnz) X(csc_u) X(csc_p) X(csc_row) X(pen) X(cflags) X(cdup) X(x) X(vstate) X(ratio) X(key) X(cst) X(bsum) \
  X(rdq) X(rqst) X(useg) X(ucnt) X(crec) X(ctl) X(vstat) X(flagbits) X(anat) X(anat_r)

FR_FIELDS(HAS_MEMBER)
FB_FIELDS(HAS_MEMBER)
DEV_FIELDS(HAS_MEMBER)

#define COUNT(name) +1
static_assert(0 FR_FIELDS(COUNT) == 8 && 0 FB_FIELDS(COUNT) == 19, "the 27 moved members");

#define NOT_IN_DEV(name) static_assert(!has_##name<Dev>::value, "Dev still has " #name);
#define IN_FR(name) static_assert(has_##name<FrDev>::value && has_##name<FrFields>::value, "FrDev lacks " #name);
#define NOT_IN_FR(name) static_assert(!has_##name<FrDev>::value, "FrDev has FairBottleneck's " #name);
#define IN_FB(name) static_assert(has_##name<FbDev>::value && has_##name<FbFields>::value, "FbDev lacks " #name);
#define NOT_IN_FB(name) static_assert(!has_##name<FbDev>::value, "FbDev has the frontier's " #name);
#define IN_ALL(name) \
  static_assert(has_##name<Dev>::value && has_##name<FrDev>::value && has_##name<FbDev>::value, "missing " #name);
FR_FIELDS(NOT_IN_DEV)
FB_FIELDS(NOT_IN_DEV)
FR_FIELDS(IN_FR)
FB_FIELDS(NOT_IN_FR)
FB_FIELDS(IN_FB)
FR_FIELDS(NOT_IN_FB)
DEV_FIELDS(IN_ALL)

// the views are kernel arguments and pass to `const Dev&` helpers through the base
static_assert(std::is_trivially_copyable<Dev>::value && std::is_trivially_copyable<FrDev>::value &&
                  std::is_trivially_copyable<FbDev>::value,
              "kernel arguments");
static_assert(std::is_base_of<Dev, FrDev>::value && std::is_base_of<FrFields, FrDev>::value, "FrDev : Dev, FrFields");
static_assert(std::is_base_of<Dev, FbDev>::value && std::is_base_of<FbFields, FbDev>::value, "FbDev : Dev, FbFields");
static_assert(sizeof(FrDev) == sizeof(Dev) + sizeof(FrFields) && sizeof(FbDev) == sizeof(Dev) + sizeof(FbFields),
              "a view is the Dev and its engine's fields, nothing else");

// Dev with all 27 members was 720 bytes (8 x 8 frontier, 8 + 18 x 8 FairBottleneck, the rest unchanged)
constexpr size_t kDevBefore = 720;
static_assert(sizeof(Dev) + sizeof(FrFields) + sizeof(FbFields) == kDevBefore, "a member was added or lost in the split");
static_assert(sizeof(Dev) < kDevBefore, "sizeof(Dev) shrank");

// Member order of Dev: a kernel loads adjacent arguments it uses as one wider scalar load, so three diagnostic members
// keep hot ones apart (lmm_dev.hpp): x | anat | vstate | anat_r | ratio and ctl | flagbits | vstat.  An edit that closes
// one of these gaps regroups the argument loads of the round engine's kernels (profiles/dev_views_compile.json).
static_assert(offsetof(Dev, anat) == offsetof(Dev, x) + 8 && offsetof(Dev, vstate) == offsetof(Dev, anat) + 8,
              "anat stands between x and vstate");
static_assert(offsetof(Dev, anat_r) == offsetof(Dev, vstate) + 8 && offsetof(Dev, ratio) == offsetof(Dev, anat_r) + 16,
              "anat_r stands between vstate and ratio");
static_assert(offsetof(Dev, flagbits) == offsetof(Dev, ctl) + 8 && offsetof(Dev, vstat) == offsetof(Dev, flagbits) + 8,
              "flagbits stands between ctl and vstat");

// the sizes, written into the compiler's output (tests/test_dev_views.py reads them; DESIGN.md quotes them)
template <size_t Dev_, size_t FrDev_, size_t FbDev_> struct [[deprecated("sizes")]] DevViewSizes {};
DevViewSizes<sizeof(Dev), sizeof(FrDev), sizeof(FbDev)> dev_view_sizes;
