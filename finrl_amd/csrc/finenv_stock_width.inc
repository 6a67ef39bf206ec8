// finenv_stock_width.inc -- everything a finenv_stock_np{32,64,128}.hip holds but its width: the kernels
// of finenv_stock_kernels.inc / finenv_stock_wide.inc in namespace np<FINENV_NP>, the choice of step-kernel
// instantiation (made once per handle: the step plan of finenv_stock.hip), and the aux launcher.  One translation unit per width because each
// takes most of a minute to compile and they build side by side; design notes: finenv_stock.hip.
#include "finenv_stock_common.h"

#define FINENV_CAT_(a, b) a##b
#define FINENV_CAT(a, b) FINENV_CAT_(a, b)
#define FINENV_WIDTH_NS FINENV_CAT(np, FINENV_NP)

namespace {
namespace FINENV_WIDTH_NS {
#include "finenv_stock_kernels.inc"
#include "finenv_stock_wide.inc"      // templates only: instantiated below at kNPad == 128

// Which instantiation steps this batch (results never depend on the choice, only the time does).
template <bool TURB, bool STATS>
finenv_stock_impl::StepPlan choose_step(const finenv_stock_config &cfg, bool win, bool desync)
{
    constexpr size_t lds = sizeof(float) * kLdsStep;
    if constexpr (!kWide) {
        // per-env windows: the DES form only.  A lock-step WIN instantiation was measured too: no faster
        // on windows [0, T) (21.41 vs 21.36 us), and the build holding it ran the no-window headline 1 %
        // slower in the in-process A/B against the parent (cause not isolated; DESIGN.md 4.5)
        if (win) return {stock_step_kernel<TURB, STATS, true, true>, lds};
        // envs may sit on different days: the instantiation with the per-env fast paths
        if (desync) return {stock_step_kernel<TURB, STATS, true, false>, lds};
    } else {
        if constexpr (kNPad == 128) {
            // NASDAQ-100 shape (BASELINE configs[3]): compile-time ticker count, 40.7 KB of LDS, 4 blocks
            // per CU; its 16-bit keys hold hmax <= 255, larger goes to the generic kernel
            using G = WideGeom<100>;
            if (cfg.n_tickers == 100 && cfg.hmax <= G::kMaxHmax)
                return win ? finenv_stock_impl::StepPlan{stock_step_wide_kernel<TURB, STATS, 100, true>, G::kBytes}
                           : finenv_stock_impl::StepPlan{stock_step_wide_kernel<TURB, STATS, 100, false>, G::kBytes};
        }
        if (win) return {stock_step_kernel<TURB, STATS, false, true>, lds};
    }
    // (32-wide: the three-wave lock-step form, 192 threads per block)
    return {stock_step_kernel<TURB, STATS, false, false>, lds, kBlockThreads<false>};
}
}  // namespace np<FINENV_NP>
}  // namespace

namespace finenv_stock_impl {

StepPlan FINENV_CAT(choose_step_np, FINENV_NP)(const finenv_stock_config &cfg, bool win, bool desync)
{
    using namespace FINENV_WIDTH_NS;
    const bool turb = cfg.use_turbulence != 0, stats = cfg.track_stats != 0;
    if (turb && stats) return choose_step<true, true>(cfg, win, desync);
    if (turb) return choose_step<true, false>(cfg, win, desync);
    if (stats) return choose_step<false, true>(cfg, win, desync);
    return choose_step<false, false>(cfg, win, desync);
}

void FINENV_CAT(launch_aux_np, FINENV_NP)(const Params &p, int mode, hipStream_t stream)
{
    using namespace FINENV_WIDTH_NS;
    const int waves = (p.cfg.n_envs + kWave - 1) / kWave;
    const dim3 grid((unsigned)((waves + kAuxWaves - 1) / kAuxWaves));
    hipLaunchKernelGGL(stock_aux_kernel, grid, dim3(kWave * kAuxWaves), 0, stream, p, mode);
}

}  // namespace finenv_stock_impl
