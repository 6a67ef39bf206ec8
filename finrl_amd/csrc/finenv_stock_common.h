// finenv_stock_common.h -- shared by the translation units of the batched StockTradingEnv:
// finenv_stock.hip (C ABI, dispatch, terminal-summary kernel) and finenv_stock_np{32,64,128}.hip
// (the step / aux kernels compiled per padded ticker count, one file each so `make -j` builds
// them side by side).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <cstddef>
#include <new>
#include <type_traits>

#include "finenv.h"
#include "finenv_dev.h"
#include "finenv_host.h"

namespace finenv_stock_impl {
struct Params {
    finenv_stock_config cfg;
    finenv_stock_panel panel;
    finenv_stock_state st;
    const float *actions;
    float *obs;
    float *reward;
    uint8_t *done;
    float *term_obs;
    int32_t *realised;
    const uint8_t *mask;
    double *stats_out;
    int32_t auto_reset;
    int32_t D;
    int32_t obs_pitch;    // row pitch of `obs` in floats (>= D; D = packed rows)
    int32_t desync_hint;  // envs may sit on different days (selects the kernel instantiation only)
    int32_t day0;
    uint32_t magicN;      // ceil(2^32 / N) for N >= 2 (exact f / N for f < 2^16)
    int32_t block_base;   // first 64-env group of this launch (batches larger than one resident round of
                          // blocks are stepped as several launches: launch_step_rounds, finenv_stock.hip)
    int32_t diag;         // FINENV_DIAG builds only: phase-skip bitmask (timing experiments)
    unsigned long long *dbg;   // FINENV_DIAG builds only: [block][kStampRoles][16] s_memrealtime stamps
    double *last;         // last-episode block [FINENV_STOCK_LAST_FIELDS][E] or NULL
    const int32_t *win;   // per-env windows [2][E] (starts, ends) or NULL (finenv_stock_set_windows)
};
}  // namespace finenv_stock_impl

namespace {

constexpr int kWave = 64;
constexpr int kStepThreads = 2 * kWave;       // trader + streamer (the lock-step 32-wide kernel adds a sorter wave)
constexpr int kStampRoles = 3;                // stamp rows per block of the diagnostic build (tools/phase_times.py)

using finenv_stock_impl::Params;

#ifdef FINENV_DIAG
#define DIAG(bit) (p.diag & (bit))
// phase stamps (100 MHz wall clock) for tools/phase_times.py; diagnostic build only
#define STAMP(k)                                                                          \
    do {                                                                                  \
        if (p.dbg != nullptr && lane == 0) {                                              \
            __builtin_amdgcn_sched_barrier(0);                                            \
            p.dbg[((size_t)(blockIdx.x + p.block_base) * kStampRoles + role) * 16 + (k)] = __builtin_amdgcn_s_memrealtime(); \
            __builtin_amdgcn_sched_barrier(0);                                            \
        }                                                                                 \
    } while (0)
#else
#define DIAG(bit) 0
#define STAMP(k) do { } while (0)
#endif

// per-env state fields: [field][env] blocks (include/finenv.h)
#define SF(fld) (*at(p.st.f64, (unsigned)(fld) * (unsigned)E + (unsigned)e))
#define SI(fld) (*at(p.st.i32, (unsigned)(fld) * (unsigned)E + (unsigned)e))
#define HOLD(i) SI(FINENV_STOCK_I32_FIELDS + (i))
#define SH0(i) SI(FINENV_STOCK_I32_FIELDS + N + (i))
#define SL(fld) (*at(p.last, (unsigned)(fld) * (unsigned)E + (unsigned)e))

// Latch the finished episode of lane e into the last-episode block `last` (p.last).  Called by the step
// kernels in their once-per-episode branch (term_mask != 0), before an auto-reset rewrites the state: at
// `term` no trade happens and nothing has been written back, so the state in memory IS the terminal state.
// Everything but the end asset is loaded afresh here, so no value is carried from the top of the kernel
// into this branch (the step kernels sit at the register-file edge).
__device__ __forceinline__ void latch_last_episode(const Params &p, double *last, int E, int e,
                                                   double end_asset)
{
#define LB(fld) (*at(last, (unsigned)(fld) * (unsigned)E + (unsigned)e))
    LB(FINENV_SL_COUNT) = LB(FINENV_SL_COUNT) + 1.0;
    LB(FINENV_SL_EPISODE) = (double)SI(FINENV_SI_EPISODE);
    LB(FINENV_SL_BEGIN_ASSET) = SF(FINENV_SF_ASSET0);
    LB(FINENV_SL_END_ASSET) = end_asset;
    LB(FINENV_SL_COST) = SF(FINENV_SF_COST);
    LB(FINENV_SL_TRADES) = (double)SI(FINENV_SI_TRADES);
    LB(FINENV_SL_RET_N) = (double)(SI(FINENV_SI_DAY) - SI(FINENV_SI_START_DAY));
    LB(FINENV_SL_RET_SUM) = SF(FINENV_SF_RET_SUM);
    LB(FINENV_SL_RET_SUMSQ) = SF(FINENV_SF_RET_SUMSQ);
#undef LB
}

// Params::last of a step kernel's argument (its only one), read from the kernel-argument segment in the
// once-per-episode branch.  A plain `p.last` there is loaded at the top of the kernel with the other
// arguments.  The kernels of finenv_stock_kernels.inc are at the SGPR limit, and that one more pair live
// across the whole step moved their SGPR spills into the trade loops (DOW30 step 1 % slower with the block
// detached, in-process A/B).  The empty asm keeps the load below it.  (stock_step_wide_kernel measured the
// other way round: it reads p.last.)
__device__ __forceinline__ double *last_block()
{
    const char *ka = (const char *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    return *reinterpret_cast<double *const *>(ka + offsetof(Params, last));
}

// Per-env episode windows (finenv_stock_set_windows): win_start / win_last_day of finenv_dev.h.  The step
// kernels read the end every step (one coalesced 4-byte load beside SI(DAY)) and the start only on their
// wave-uniform reset path.

// ---- pieces of the step rule (env_stocktrading.py:220-357) that every form of stock_step_kernel and
// stock_step_wide_kernel state the same way.  (SF / SI capture the names p, E and e: keep these parameter names.)

// reciprocal + one Newton step of a unit price: floor(cash * x) is then within 1 of cash // unit for
// |cash / unit| < 2^40, and the sign of one FMA remainder makes it exact (the buy loops)
__device__ __forceinline__ double refined_rcp(double u)
{
    const double x = __builtin_amdgcn_rcp(u);
    return fma(fma(-u, x, 1.0), x, x);
}

// reset(), :359-393: the scalars of a fresh episode that no step carries in registers (the aux kernel's reset
// and the step kernels' auto-reset)
__device__ __forceinline__ void store_episode_start(const Params &p, int E, int e, double asset0, int start)
{
    SF(FINENV_SF_ASSET0) = asset0;
    SF(FINENV_SF_RET_SUM) = 0.0;
    SF(FINENV_SF_RET_SUMSQ) = 0.0;
    SI(FINENV_SI_START_DAY) = start;
}

// Running sums of pct_change(asset_memory) for the terminal Sharpe (:243-251), for a step that did not end the
// episode.  asset_memory[-1] is this step's begin asset bit for bit (same cash, holdings, price row and
// summation order as the previous step's end asset) -- except on the first step of an episode, where it is
// asset_memory[0] (NumPy's pairwise sum, :364-378): no per-step copy is kept.
__device__ __forceinline__ void store_sharpe_sums(const Params &p, int E, int e, bool valid, double begin, double end,
                                                  bool first_step, double st_mean, double st_m2)
{
    double st_prev = begin;
    if (__any(first_step)) {
        const double a0 = SF(FINENV_SF_ASSET0);
        st_prev = first_step ? a0 : begin;
    }
    const double ret = end / st_prev - 1.0;
    if (valid) {
        SF(FINENV_SF_RET_SUM) = st_mean + ret;
        SF(FINENV_SF_RET_SUMSQ) = st_m2 + ret * ret;
    }
}

// state write-back of the trader's scalars (end_carry: the next step's begin asset)
template <bool TURB>
__device__ __forceinline__ void store_trader(const Params &p, int E, int e, double cash, double end_carry, double cost,
                                             int trades, int day, int pd, double last_reward, double turb,
                                             int episode_inc)
{
    SF(FINENV_SF_CASH) = cash;
    SF(FINENV_SF_BEGIN_ASSET) = end_carry;
    SF(FINENV_SF_COST) = cost;
    SI(FINENV_SI_TRADES) = trades;
    SI(FINENV_SI_DAY) = day;
    SI(FINENV_SI_PRICE_DAY) = pd;
    SF(FINENV_SF_LAST_REWARD) = last_reward;
    if (TURB) SF(FINENV_SF_TURBULENCE) = turb;
    if (episode_inc) SI(FINENV_SI_EPISODE) += 1;
}

// Diagnostic build: the wave's end clock, slot 15 of its stamp row
__device__ __forceinline__ void stamp_wave_end(const Params &p, int lane, int role)
{
#ifdef FINENV_DIAG
    if (p.dbg != nullptr && lane == 0) p.dbg[((size_t)blockIdx.x * kStampRoles + role) * 16 + 15] = __builtin_amdgcn_s_memtime();
#endif
}

__device__ __forceinline__ void ce(int &a, int &b)
{
    const int lo = min(a, b);
    const int hi = max(a, b);
    a = lo;
    b = hi;
}

}  // namespace

// Exported by the per-width translation units (C++ linkage, library-internal).
namespace finenv_stock_impl {
// How step() launches (kept in the handle, finenv_stock.hip).  Each width names the kernel instantiation that
// steps a handle of this config and its dynamic LDS bytes -- `win`: per-env windows are attached, `desync`:
// finenv_stock_set_desync_hint -- and launches nothing and touches no device; plan_step() fills in the rest.
struct StepPlan {
    void (*kernel)(Params);
    size_t lds_bytes;
    int threads = kStepThreads;   // threads per block
    int round;            // blocks resident on the device at once: occupancy per CU x CUs
    int lds_refused;      // the kernel needs > 64 KiB of LDS and the device refused the opt-in
};
StepPlan choose_step_np32(const finenv_stock_config &cfg, bool win, bool desync);
StepPlan choose_step_np64(const finenv_stock_config &cfg, bool win, bool desync);
StepPlan choose_step_np128(const finenv_stock_config &cfg, bool win, bool desync);
// init / reset / observe (mode 0 / 1 / 2)
void launch_aux_np32(const Params &p, int mode, hipStream_t stream);
void launch_aux_np64(const Params &p, int mode, hipStream_t stream);
void launch_aux_np128(const Params &p, int mode, hipStream_t stream);
}  // namespace finenv_stock_impl
