// The WEIGHTED instances of the flat, coalesced-flat and one-lookup gather forms ("sls_weighted_flat" 1): the kernel
// templates of sls_dev.h on the element type Wgt<policy>, for every row policy and every (G, NL, BPW, NT) / (G, BW) that plan_sls can
// reach.  A translation unit of its own so that its 476 instances compile beside sls.hip's, not behind them; sls.hip's
// launch_sls_e logs the launch and hands a weighted plan of these three forms to launch_sls_wflat.
#include "drs_internal.h"
#include "launch_host.h"
#include "owner_dev.h"
#include "sls_dev.h"

namespace drs {
namespace {

template <class E>
hipError_t launch_wflat_e(const SlsArgs& a, const SlsPlan& p, hipStream_t s, hipEvent_t stop) {
  const dim3 grid((unsigned)p.grid);
  switch (p.form) {
    case SlsForm::flatc:
      with_int<8, 16, 32>(p.G, [&](auto G) { with_int<5, 10, 20>(p.NL, [&](auto NL) { with_int<0, 1>(p.nt, [&](auto NT) {
        launch_k(sls_flatc_kernel<G, NL, NT != 0, Wgt<E>>, grid, s, stop, a, p.L);
      }); }); });
      break;
    case SlsForm::flat:   // (xcd_order 1, as the unweighted launch)
      with_int<8, 16, 32>(p.G, [&](auto G) { with_int<5, 10, 20>(p.NL, [&](auto NL) { with_int<0, 1>(p.nt, [&](auto NT) {
        with_int<1, 2, 4>(p.BPW, [&](auto BPW) {
          if constexpr (BPW == 1 || NL <= 10) launch_k(sls_flat_kernel<G, NL, BPW, NT != 0, Wgt<E>>, grid, s, stop, a, p.L, 1);
        });
      }); }); });
      break;
    case SlsForm::one:
      with_int<4, 8, 16, 32>(p.G, [&](auto G) { with_int<64, 16>(p.BW, [&](auto BW) {
        launch_k(sls_one_kernel<G, BW, Wgt<E>>, grid, s, stop, a, p.tiles);
      }); });
      break;
    default:   // (the ring walk and the any-width form keep their weighted instances in sls.hip)
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace

hipError_t launch_sls_wflat(const SlsArgs& a, const SlsPlan& p, hipStream_t s, hipEvent_t stop) {
  if (!p.weighted || p.grid <= 0) return hipErrorInvalidValue;
  switch (p.dtype) {
    case DRS_TABLE_FP16: return launch_wflat_e<F16>(a, p, s, stop);
    case DRS_TABLE_BF16: return launch_wflat_e<BF16>(a, p, s, stop);
    case DRS_TABLE_FP8_E4M3: return a.tab_scale ? launch_wflat_e<F8>(a, p, s, stop) : hipErrorInvalidValue;
    case DRS_TABLE_INT8_ROWWISE: return a.ln_pad ? launch_wflat_e<I8L>(a, p, s, stop) : launch_wflat_e<I8>(a, p, s, stop);
    case DRS_TABLE_INT4_ROWWISE: return a.ln_pad ? launch_wflat_e<I4L>(a, p, s, stop) : launch_wflat_e<I4>(a, p, s, stop);
    default: return launch_wflat_e<F32>(a, p, s, stop);
  }
}

}  // namespace drs
