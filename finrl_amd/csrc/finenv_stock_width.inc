// finenv_stock_width.inc -- everything a finenv_stock_np{32,64,128}.hip holds but its width: the kernels
// of finenv_stock_kernels.inc / finenv_stock_wide.inc in namespace np<FINENV_NP>, the choice of step-kernel
// instantiation, and the launchers finenv_stock.hip calls.  One translation unit per width because each
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
int launch_step(const Params &p, int device, hipStream_t stream)
{
    constexpr size_t lds = sizeof(float) * kLdsStep;
    const bool win = p.win != nullptr;          // per-env windows: the WIN instantiations
    if constexpr (!kWide) {
        // per-env windows: the DES form only.  A lock-step WIN instantiation was measured too: no faster
        // on windows [0, T) (21.41 vs 21.36 us), and the build holding it ran the no-window headline 1 %
        // slower in the in-process A/B against the parent (cause not isolated; DESIGN.md 4.5)
        if (win) return launch_step_rounds<stock_step_kernel<TURB, STATS, true, true>>(p, lds, device, stream);
        // envs may sit on different days: the instantiation with the per-env fast paths
        if (p.desync_hint) return launch_step_rounds<stock_step_kernel<TURB, STATS, true, false>>(p, lds, device, stream);
    } else {
        if constexpr (kNPad == 128) {
            // NASDAQ-100 shape (BASELINE configs[3]): compile-time ticker count, 40.7 KB of LDS, 4 blocks
            // per CU; its 16-bit keys hold hmax <= 255, larger goes to the generic kernel
            using G = WideGeom<100>;
            if (p.cfg.n_tickers == 100 && p.cfg.hmax <= G::kMaxHmax)
                return win ? launch_step_rounds<stock_step_wide_kernel<TURB, STATS, 100, true>>(p, G::kBytes, device, stream)
                           : launch_step_rounds<stock_step_wide_kernel<TURB, STATS, 100, false>>(p, G::kBytes, device, stream);
        }
        if (win) return launch_step_rounds<stock_step_kernel<TURB, STATS, false, true>>(p, lds, device, stream);
    }
    return launch_step_rounds<stock_step_kernel<TURB, STATS, false, false>>(p, lds, device, stream);
}
}  // namespace np<FINENV_NP>
}  // namespace

namespace finenv_stock_impl {

int FINENV_CAT(launch_step_np, FINENV_NP)(const Params &p, bool turb, bool stats, int device, hipStream_t stream)
{
    using namespace FINENV_WIDTH_NS;
    if (turb && stats) return launch_step<true, true>(p, device, stream);
    if (turb) return launch_step<true, false>(p, device, stream);
    if (stats) return launch_step<false, true>(p, device, stream);
    return launch_step<false, false>(p, device, stream);
}

void FINENV_CAT(launch_aux_np, FINENV_NP)(const Params &p, int mode, hipStream_t stream)
{
    using namespace FINENV_WIDTH_NS;
    const int waves = (p.cfg.n_envs + kWave - 1) / kWave;
    const dim3 grid((unsigned)((waves + kAuxWaves - 1) / kAuxWaves));
    hipLaunchKernelGGL(stock_aux_kernel, grid, dim3(kWave * kAuxWaves), 0, stream, p, mode);
}

}  // namespace finenv_stock_impl
