// nuts_part.inc — body of nuts_partK.hip: the NUTS kernel instantiations of
// the layouts in GM_NUTS_PART_LAYOUTS(X) (X(LPC, E)), both dtypes, every
// built-in target, identity and adaptive metric; see nuts_launch.h.
#include "gm_layouts.h"
#include "nuts_device.h"
#include "nuts_launch.h"

// GM_NUTS_REC 1 (nuts_rec_partK.hip): the recording instantiations instead
#ifndef GM_NUTS_REC
#define GM_NUTS_REC 0
#endif
#if GM_NUTS_REC
#define GM_NUTS_PART_FN nuts_launch_rec_part
#else
#define GM_NUTS_PART_FN nuts_launch_part
#endif
#define GM_NUTS_CAT2(a, b) a##b
#define GM_NUTS_CAT(a, b) GM_NUTS_CAT2(a, b)

namespace gm {

hipError_t GM_NUTS_CAT(GM_NUTS_PART_FN, GM_NUTS_PART)(gm_dtype dt, const TargetDev& tg, const Layout& lay,
                                                      NutsLaunch& a, hipStream_t st, const NutsLdsBudget& b,
                                                      bool* found) {
  constexpr bool REC = GM_NUTS_REC != 0;
  // the kernel's argument block: the caller's NutsRecLaunch when recording
  typename NutsLaunchOf<REC>::type& ka = static_cast<typename NutsLaunchOf<REC>::type&>(a);
  auto f = [&]<class T, int LPC, int E, class TG>(TG t) -> hipError_t {
    const long long threads = a.C * LPC;
    const unsigned blocks = (unsigned)((threads + 255) / 256);
    const size_t lds = nuts_size_lds(a, b, blocks, t.template lds_bytes<LPC, E>(), LPC, E, sizeof(T));
    // the metric kinds the run can meet, at compile time (MassDev)
    // (the frozen-dense kernel only at 16 x 2, the layout whose dense metric
    // lives in LDS; nuts_run sets dense_frozen for it alone)
    if constexpr (LPC == 16 && E == 2) {
      if (a.mass_mode == 2 && a.dense_frozen) {
        hipLaunchKernelGGL((nuts_kernel<T, LPC, E, TG, 3, REC>), dim3(blocks), dim3(256), lds, st, ka, t);
        return hipGetLastError();
      }
    }
    if (a.mass_mode == 2)
      hipLaunchKernelGGL((nuts_kernel<T, LPC, E, TG, 2, REC>), dim3(blocks), dim3(256), lds, st, ka, t);
    else if (a.mass_mode == 1)
      hipLaunchKernelGGL((nuts_kernel<T, LPC, E, TG, 1, REC>), dim3(blocks), dim3(256), lds, st, ka, t);
    else
      hipLaunchKernelGGL((nuts_kernel<T, LPC, E, TG, 0, REC>), dim3(blocks), dim3(256), lds, st, ka, t);
    return hipGetLastError();
  };
  *found = false;
#define GM_NUTS_TRY(L_, E_)                                                            \
  if (lay.lanes == L_ && lay.elems == E_) {                                            \
    *found = true;                                                                     \
    return dt == GM_F32 ? dispatch_target<float, L_, E_>(tg, f) : dispatch_target<double, L_, E_>(tg, f); \
  }
  GM_NUTS_PART_LAYOUTS(GM_NUTS_TRY)
#undef GM_NUTS_TRY
  return hipSuccess;
}

}  // namespace gm

#if defined(GM_NUTS_PROF) && GM_NUTS_PART == 0 && !GM_NUTS_REC
// measurement build only: the per-wave iteration profile of the last NUTS
// launch (nuts_device.h), n = waves x NPROF_SLOTS (43) unsigned 64-bit words
extern "C" int gm_nuts_prof_read(void* out, long long n) {
  if (n > (long long)gm::NPROF_WAVES * gm::NPROF_SLOTS) return 1;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(gm::gm_nuts_prof_buf), n * 8, 0, hipMemcpyDeviceToHost) == hipSuccess
             ? 0 : 2;
}
#endif
