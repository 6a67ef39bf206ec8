// finenv_twowave.h -- what the cash-penalty and stop-loss envs share (finenv_cashpenalty.hip,
// finenv_stoploss.hip): the kernel argument, the device helpers of their trader + streamer step
// kernels (one 128-thread block per 64 envs) and the host side of their C ABI.  Everything is a
// template on the env's own argument struct P or handle H; the step kernels themselves, the state layout
// macros and the extern "C" entry points stay in the two files.  The episode history reads the audit
// row, which is the same for both: its kernels are one object of their own, finenv_twowave_history.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "finenv.h"
#include "finenv_dev.h"
#include "finenv_host.h"

// ---- episode history (finenv_<kind>_set_history) --------------------------------------------
// account_information / actions_memory / transaction_memory of every env's current episode, kept on
// the device: two small kernels with their own argument struct, shared by both envs -- the audit
// head is the same and nothing here depends on the env kind.  They ride behind the step / reset
// kernels as separate launches on the same stream and read what those left in memory: the audit row,
// done and the caller's action tile.  The rule is in include/finenv.h.  The kernels are compiled once,
// in finenv_twowave_history.hip, not into both envs' objects.
namespace finenv_twowave {

struct HistoryArgs {
    finenv_twowave_history h;
    const double *audit;          // record: this step's audit rows [E][FINENV_AUDIT_HEAD + N]
    const float *actions;         // record: this step's action tile [E][N]
    const uint8_t *done;          // record: this step's done [E]
    const uint8_t *mask;          // arm: envs to arm, or NULL = all
    const int32_t *date_index;    // arm: the state's FINENV_K?_DATE_INDEX row [E]
    const int32_t *win;           // arm: the window block [4][E], or NULL
    double *out;                  // (unused since the metrics kernel is finenv_history.hip's: the two stay so
    double annualization;         //  that the record kernel behind every step keeps the bytes it was timed with)
    int32_t E, N, n_days;
    uint32_t magicN;              // ceil(2^32 / N) for N >= 2
};

void launch_history_record(const HistoryArgs &a, hipStream_t stream);     // tw_history_record_kernel
void launch_history_arm(const HistoryArgs &a, hipStream_t stream);        // tw_history_arm_kernel

}  // namespace finenv_twowave

namespace {

// The kernel argument.  CpParams / SlParams derive from it and add nothing: the kernels keep their
// symbols, and the helpers below read the LDS strides from the argument's type.
template <class Cfg, class Panel, class State, int kMaxAssets>
struct TwoWaveParams {
    static constexpr int kRow = kMaxAssets + 1;        // f32 rows [el][cash | holdings]
    static constexpr int kClStride = kMaxAssets + 1;   // f64 close rows [el][i]: odd stride, conflict-free
    Cfg cfg;
    Panel panel;
    State st;
    const float *actions;
    float *obs;
    float *reward;
    uint8_t *done;
    float *term_obs;
    const uint8_t *mask;
    int32_t auto_reset;
    int32_t D;
    uint32_t magicN;
    int32_t rs_hi;                  // random_start: draw in [0, rs_hi) on the device (0 = off)
    unsigned long long rs_seed;
    double *audit;                  // optional [E][FINENV_AUDIT_HEAD + N] per-step log row, or NULL
    unsigned long long *dbg;        // FINENV_DIAG builds only: [block][16] s_memrealtime stamps
    // finenv_<kind>_set_windows (the WIN instantiations; NULL otherwise).  Last member: every other
    // kernel argument keeps its offset
    int32_t *win;                   // [4][E]: pending start / end, active start / end
};

// ---- per-env episode windows (finenv_<kind>_set_windows) -------------------------------------
// WIN: env e runs the ACTIVE window [s_e, t_e) = win[2][e], win[3][e] of panel rows; a reset (host or
// auto) first copies the PENDING window win[0][e], win[1][e] into the active rows and starts the env
// inside it.  Every value read from the block is clamped into the panel, and so is the date index:
// bad device-side content is a wrong answer, never an access outside the panel or the state.
#define TWWIN(r) (*at(p.win, (unsigned)(r) * (unsigned)p.cfg.n_envs + (unsigned)e))

// the active window's end t_e, in [1, n_days]; without windows: n_days
template <bool WIN, class P>
__device__ __forceinline__ int tw_win_end(const P &p, int e)
{
    if (!WIN) return p.cfg.n_days;
    return min(max(TWWIN(3), 1), p.cfg.n_days);
}

// the pending window: s in [0, n_days - 1], t in [s + 1, n_days]; without windows: the panel
template <bool WIN, class P>
__device__ __forceinline__ void tw_win_pending(const P &p, int e, int *s, int *t)
{
    *s = 0;
    *t = p.cfg.n_days;
    if (!WIN) return;
    *s = min(max(TWWIN(0), 0), p.cfg.n_days - 1);
    *t = min(max(TWWIN(1), *s + 1), p.cfg.n_days);
}

// the date index as the state holds it; WIN: clamped into the panel
template <bool WIN, class P>
__device__ __forceinline__ int tw_date(const P &p, int di)
{
    return WIN ? min(max(di, 0), p.cfg.n_days - 1) : di;
}

// "last date" of the episode, `end` = tw_win_end().  (WIN: >=, so that a date index past a window
// that bad content made shorter never advances out of the panel)
template <bool WIN>
__device__ __forceinline__ bool tw_last_date(int di, int end)
{
    return WIN ? di >= end - 1 : di == end - 1;
}

// The one starting-point rule of a reset (finenv_<kind>_reset, the auto-reset inside step and the
// streamer's speculation of it): tw_next_start<WIN>(p, e, episode, next_start), where `episode` and
// `next_start` are the kernel's own expressions for the env's episode counter and NEXT_START -- only
// the one the rule uses is evaluated, i.e. loaded.  random_start (rs_hi > 0) draws from the first half
// of the frame's dates (:134-138); WIN: of the PENDING window [s, t), which tw_win_promote() makes the
// active one when the env is reset -- s + draw in [0, max(1, (t - s) >> 1)), only the sign of rs_hi
// is read; else s + NEXT_START as an offset from the window's first row, clamped into the window.
// (A macro around the WIN form: in a kernel scope with p and e, the no-window arm is then the
//  expression these kernels always had, and compiles to the same instructions.)
#define TW_NEXT_START(WIN, episode, next_start)                                                    \
    (!(WIN) ? (p.rs_hi > 0 ? draw_start(p.rs_seed, e, (episode) + 1, p.rs_hi) : (next_start))     \
            : tw_next_start_win(p, e, [&]() { return episode; }, [&]() { return next_start; }))
template <class P, class Episode, class NextStart>
__device__ __forceinline__ int tw_next_start_win(const P &p, int e, Episode episode, NextStart next_start)
{
    int s, t;
    tw_win_pending<true>(p, e, &s, &t);
    const int len = t - s;
    return s + (p.rs_hi > 0 ? draw_start(p.rs_seed, e, episode() + 1, max(1, len >> 1))
                            : min(max(next_start(), 0), len - 1));
}

// pending -> active, by the lane that owns env e, in the once-per-episode branch that resets it (the
// pair tw_next_start() read in this launch, loaded again beside the episode counter that branch
// increments rather than held in two registers across the step)
template <bool WIN, class P>
__device__ __forceinline__ void tw_win_promote(const P &p, int e)
{
    if (!WIN) return;
    int s, t;
    tw_win_pending<WIN>(p, e, &s, &t);
    TWWIN(2) = s;
    TWWIN(3) = t;
}

// rows[el*kRow + 0] = f32 cash, rows[el*kRow + 1 + i] = f32 holdings_i; columns > N: info row
template <bool kCompact = false, class P>
__device__ __forceinline__ void tw_write_rows(float *__restrict__ dst, const P &p, int e0,
                                              int nenv_w, int row_day,
                                              unsigned long long lane_mask, const float *rows,
                                              int lane)
{
    const int N = p.cfg.n_assets, D = p.D, W = D - 1 - N;
    write_obs_rows_generic<8, 32, kCompact>(
        dst, W > 0 ? p.panel.info : nullptr, D, e0, nenv_w, row_day, lane_mask, rows, P::kRow, lane,
        [=](int day, int col) { return day * W + col - 1 - N; },
        [=](int col) { return col <= N ? col : -1; });
}

// f64 closes of every env's own date into LDS [el][i] (stride kClStride), 64 row loads in flight
template <class P>
__device__ __forceinline__ void tw_gather_closes(double *trl, const P &p, int di, int lane)
{
    const int N = p.cfg.n_assets;
    const int li = min(lane, N - 1);
    double cv[kWaveSize];
#pragma unroll
    for (int j = 0; j < kWaveSize; ++j) {
        const int de = __builtin_amdgcn_readlane(di, j);
        cv[j] = *at(p.panel.close, (unsigned)(de * N + li));
    }
#pragma unroll
    for (int j = 0; j < kWaveSize; ++j)
        if (lane < N) trl[j * P::kClStride + lane] = cv[j];
}

// Chunk 0 of rows [el_lo, el_hi): market values parked in LDS ([el][64]) with cash / holdings
// patched in from rows[].  Only stores towards HBM (LDS reads run ahead of them).
template <int NCH, class P>
__device__ __forceinline__ void tw_head_store(float *__restrict__ dst, const P &p, int e0,
                                              int nenv_w, unsigned long long lane_mask,
                                              const float *rows, const float *park, int lane,
                                              int el_lo, int el_hi)
{
    const int N = p.cfg.n_assets, D = p.D;
    float *const base = dst + (size_t)e0 * D;
    const bool head = lane <= N, in = NCH > 1 || lane < D;
    const unsigned long long want = ((el_hi - el_lo >= 64) ? ~0ull : ((1ull << (el_hi - el_lo)) - 1ull))
                                    << el_lo;
    if (nenv_w >= el_hi && (lane_mask & want) == want) {       // all rows: LDS reads 8 rows ahead
        for (int g = el_lo; g < el_hi; g += 8) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float hv = rows[(g + j) * P::kRow + (head ? lane : 0)];
                const float pv = park[(g + j) * kWaveSize + lane];
                v[j] = head ? hv : pv;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (in) *at(base, (unsigned)((g + j) * D + lane)) = v[j];
        }
        return;
    }
    for (int el = el_lo; el < el_hi; ++el) {
        if (el >= nenv_w || !((lane_mask >> el) & 1ull)) continue;
        const float hv = rows[el * P::kRow + (head ? lane : 0)];
        const float v = head ? hv : park[el * kWaveSize + lane];
        if (in) *at(base, (unsigned)(el * D + lane)) = v;
    }
}

// ---- host side ------------------------------------------------------------------------------

// What struct finenv_cashpenalty and struct finenv_stoploss hold.
template <class Cfg, class Panel, class State>
struct TwoWaveHandle : finenv_host::Handle {
    int32_t rs_hi;
    unsigned long long rs_seed;
    double *audit;
    Cfg cfg;
    Panel panel;
    State st;
    uint32_t magicN;
    int32_t *win;                   // finenv_<kind>_set_windows
    int has_hist;                   // finenv_<kind>_set_history
    finenv_twowave_history hist;
};

// the kernel argument as the handle fills it; the entry point adds its own pointers
template <class P, class H>
P tw_params(const H *h)
{
    P p;
    memset(&p, 0, sizeof(p));
    p.cfg = h->cfg;
    p.panel = h->panel;
    p.st = h->st;
    p.D = h->D;
    p.magicN = h->magicN;
    p.rs_hi = h->rs_hi;
    p.rs_seed = h->rs_seed;
    p.audit = h->audit;
    p.win = h->win;
    return p;
}

// finenv_<kind>_create: at most max_assets assets; the f64 state block has f64_fields + books * N rows
// of E doubles.  Every byte offset the kernels form must fit 32 bits (at()).
template <class H, class Cfg>
int tw_create(const Cfg *cfg, H **out, int max_assets, int f64_fields, int books)
{
    if (!cfg || !out) return FINENV_ERR_INVALID;
    *out = nullptr;
    if (cfg->n_envs < 1 || cfg->n_assets < 1 || cfg->n_assets > max_assets ||
        cfg->n_cols < 0 || cfg->n_days < 1 || cfg->shares_increment < 1 || !(cfg->hmax >= 0) ||
        !(cfg->initial_amount > 0))
        return FINENV_ERR_INVALID;
    const long long E = cfg->n_envs, N = cfg->n_assets, T = cfg->n_days;
    const long long D = 1 + N + N * cfg->n_cols, lim = (1ll << 32) - 1;
    if ((f64_fields + books * N) * E * 8 > lim || T * N * cfg->n_cols * 4 > lim ||
        T * N * 8 > lim || 64 * D * 4 > lim || E * N * 4 > lim)
        return FINENV_ERR_INVALID;
    H *h = finenv_host::new_handle<H>(cfg, D);
    if (!h) return FINENV_ERR_NOMEM;
    h->magicN = finenv_host::magic_for(N);
    *out = h;
    return FINENV_OK;
}

template <class H, class Panel, class State>
int tw_bind(H *h, const Panel *panel, const State *st)
{
    if (!h || !panel || !st) return FINENV_ERR_INVALID;
    if (!panel->close || (!panel->info && h->cfg.n_cols > 0) ||
        (!panel->turb && h->cfg.use_turbulence) || !st->f64 || !st->i32)
        return finenv_host::fail(h, FINENV_ERR_INVALID, "bind: null pointer");
    return finenv_host::bind(h, panel, st);
}

template <class H>
int tw_set_random_start(H *h, int32_t hi, uint64_t seed)
{
    if (!h || hi < 0 || hi > h->cfg.n_days) return FINENV_ERR_INVALID;
    h->rs_hi = hi;
    h->rs_seed = seed;
    return FINENV_OK;
}

template <class H>
int tw_set_audit(H *h, double *audit)
{
    if (!h) return FINENV_ERR_INVALID;
    h->audit = audit;
    return FINENV_OK;
}

template <class H>
int tw_set_windows(H *h, int32_t *win)
{
    if (!h) return FINENV_ERR_INVALID;
    h->win = win;
    return FINENV_OK;
}

template <class H>
finenv_twowave::HistoryArgs tw_history_args(const H *h)
{
    finenv_twowave::HistoryArgs a;
    memset(&a, 0, sizeof(a));
    a.h = h->hist;
    a.audit = h->audit;
    static_assert((int)FINENV_KI_DATE_INDEX == (int)FINENV_LI_DATE_INDEX, "one arm kernel for both envs");
    a.date_index = h->st.i32 + (size_t)FINENV_KI_DATE_INDEX * h->cfg.n_envs;
    a.win = h->win;
    a.E = h->cfg.n_envs;
    a.N = h->cfg.n_assets;
    a.n_days = h->cfg.n_days;
    a.magicN = h->magicN;
    return a;
}

// finenv_<kind>_reset restarts episodes: the reference's reset() empties the lists
template <class H>
void tw_launch_history_arm(const H *h, const uint8_t *mask, hipStream_t stream)
{
    finenv_twowave::HistoryArgs a = tw_history_args(h);
    a.mask = mask;
    finenv_twowave::launch_history_arm(a, stream);
}

template <class H>
int tw_set_history(H *h, const finenv_twowave_history *hist)
{
    if (!h) return FINENV_ERR_INVALID;
    const bool missing = hist && (!hist->cash || !hist->asset_value || !hist->reward ||
                                  !hist->reason || !hist->start || !hist->end || !hist->ntx ||
                                  !hist->len || !hist->flags);
    return finenv_host::set_history(
        h, h->hist, h->has_hist, hist,
        missing ? "set_history: null cash/asset_value/reward/reason/start/end/ntx/len/flags" : nullptr, 1);
}

// the metrics' series: the total assets cash + asset_value of the armed records and their pct_change()
template <class H>
finenv_host::HistorySeries tw_history_series(const H *h)
{
    return {h->hist.cash, h->hist.asset_value, nullptr, h->hist.len, h->hist.flags, FINENV_HIST_ARMED,
            h->hist.capacity, h->cfg.n_envs};
}

inline dim3 tw_grid(int E) { return dim3((unsigned)((E + kWaveSize - 1) / kWaveSize)); }   // one block per 64 envs

template <class K, int NCH, class P>
void tw_launch(const P &p, dim3 grid, hipStream_t stream)
{
    const dim3 block(2 * kWaveSize);
    if (p.win != nullptr) {                   // a window block is attached
        if (p.cfg.discrete_actions)
            hipLaunchKernelGGL((K::template step<NCH, true, true>()), grid, block, 0, stream, p);
        else
            hipLaunchKernelGGL((K::template step<NCH, false, true>()), grid, block, 0, stream, p);
    } else if (p.cfg.discrete_actions) {
        hipLaunchKernelGGL((K::template step<NCH, true, false>()), grid, block, 0, stream, p);
    } else {
        hipLaunchKernelGGL((K::template step<NCH, false, false>()), grid, block, 0, stream, p);
    }
}

// finenv_<kind>_step.  K names the env's kernels: K::step<NCH, DISCRETE, WIN>() with NCH 1 = rows of one
// chunk, 2 = rows of up to 320 columns (the streamer copies the market data as 16-byte quads), 0 = wider
// rows (one-wave form, on K::wide_grid(E) blocks); DISCRETE = cfg.discrete_actions; WIN = a window
// block is attached.
template <class K, class P, class H>
int tw_step(H *h, const float *actions, float *obs, float *reward, uint8_t *done, float *term_obs,
            int32_t auto_reset, void *stream, const char *what)
{
    if (const int rc = finenv_host::ready(h, "step")) return rc;
    const finenv_host::DeviceGuard guard(h->device);
    if (!actions || !obs || !reward || !done)
        return finenv_host::fail(h, FINENV_ERR_INVALID, "step: null actions/obs/reward/done");
    if (h->has_hist && !h->audit)
        return finenv_host::fail(h, FINENV_ERR_INVALID, "step: history needs an audit block");
    P p = tw_params<P>(h);
    p.actions = actions;
    p.obs = obs;
    p.reward = reward;
    p.done = done;
    p.term_obs = term_obs;
    p.auto_reset = auto_reset;
#ifdef FINENV_DIAG
    p.dbg = g_finenv_dbg;
#endif
    const int E = h->cfg.n_envs;
    if (h->D <= kWaveSize) tw_launch<K, 1>(p, tw_grid(E), (hipStream_t)stream);
    else if (h->D <= kWaveSize + 4 * kWaveSize) tw_launch<K, 2>(p, tw_grid(E), (hipStream_t)stream);
    else tw_launch<K, 0>(p, K::wide_grid(E), (hipStream_t)stream);
    if (h->has_hist) {                        // the record of this step, from what the kernel above leaves
        finenv_twowave::HistoryArgs a = tw_history_args(h);
        a.actions = actions;
        a.done = done;
        finenv_twowave::launch_history_record(a, (hipStream_t)stream);
    }
    return finenv_host::check_launch(h, what);
}

}  // namespace
