// finenv_cashpenalty.hip -- MI355X (gfx950) kernel + C ABI for the batched cash-penalty env
// (finrl/meta/env_stock_trading/env_stocktrading_cashpenalty.py: step :291-372,
// get_transactions :249-289, get_reward :237-247, reset :131-157).
//
// lane = env, one 128-thread block per 64 envs, two specialised waves:
//   wave 0 "trader"  : owns the env state.  No ordering between tickers in this env: transactions
//                      are computed per ticker (fp64), two dot products give proceeds / spend, one
//                      test decides cash shortage -- a short fp64 loop per lane.
//   wave 1 "streamer": gathers every env's next panel row (date + 1, or the known restart row on
//                      the last date) and writes the market-data chunks of the observation rows
//                      while the trader computes.  When the trader has decided which episodes end
//                      (cash shortage) it publishes every env's row through an LDS flag -- no
//                      barrier, the trader never waits; the streamer then fetches the chunk that
//                      holds cash / holdings for the decided rows plus the market-data chunks of
//                      the (rare) re-decided rows and parks chunk 0 in LDS.  After the one hand-off
//                      barrier both waves store 32 rows of chunk 0 each.
// One wave used to do both: its 192 row stores alone are 10 us of a 27 us wave (a wave issues one
// store per ~45 ns), with one wave per SIMD on the chip and the other half of the queue idle.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "finenv.h"
#include "finenv_dev.h"
#include "finenv_host.h"
#include "finenv_twowave.h"

namespace {

constexpr int kWave = 64;
constexpr int kMaxN = FINENV_CASHPENALTY_MAX_ASSETS;
struct CpParams : TwoWaveParams<finenv_cashpenalty_config, finenv_cashpenalty_panel,
                                finenv_cashpenalty_state, kMaxN> {};
constexpr int kRow = CpParams::kRow, kClStride = CpParams::kClStride;
constexpr int kWaves = 2;                    // trader + streamer
constexpr int kLdsRows = kWave * kRow;         // f32 [el][33]: action tile, then cash / holdings
constexpr int kLdsClose = kClStride * kWave * 2;   // f64 closes [el][i]
constexpr int kLdsPerBlock = kLdsRows + kLdsClose + kWave + 2;  // + the rows the trade decided (i32), flag
constexpr int kFix = 4;                        // re-decided rows per block the streamer patches in registers
static_assert(kWave * kWave <= kLdsClose, "the parked chunk 0 reuses the close rows");

#define KF(fld) (*at(p.st.f64, (unsigned)(fld) * (unsigned)E + (unsigned)e))
#define KI(fld) (*at(p.st.i32, (unsigned)(fld) * (unsigned)E + (unsigned)e))
#define KH(i) KF(FINENV_CASHPENALTY_F64_FIELDS + (i))

__device__ __forceinline__ double cp_reward(const finenv_cashpenalty_config &c, int step,
                                            double total, double cash)     // :237-247
{
    if (step == 0) return 0.0;
    const double pen = fmax(0.0, total * c.cash_penalty_proportion - cash);
    double r = ((total - pen) / c.initial_amount) - 1;
    r /= (double)step;
    return r;
}

// (launch bounds: four 2-wave blocks per CU = two waves per SIMD, i.e. at most 256 VGPRs -- at
//  65,536 envs every block of the grid is then resident at once; DISCRETE = cfg.discrete_actions as
//  a template flag: with both transaction formulas in one body the step kernel was 66 KB, over the
//  64 KB instruction cache two CUs share; WIN = per-env episode windows, finenv_cashpenalty_set_windows:
//  the helpers in finenv_twowave.h)
template <bool RESET_ONLY, int NCH, bool DISCRETE, bool WIN>
__global__ void __launch_bounds__(kWave *kWaves) __attribute__((amdgpu_waves_per_eu(2)))
cashpenalty_kernel(const CpParams p)
{
    __shared__ __attribute__((aligned(16))) float lds_all[kLdsPerBlock];
    const int lane = threadIdx.x & (kWave - 1);
    const int role = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float *rows = lds_all;
    double *trl = reinterpret_cast<double *>(lds_all + kLdsRows);
    int *decided = reinterpret_cast<int *>(lds_all + kLdsRows + kLdsClose);
    const int E = p.cfg.n_envs, N = p.cfg.n_assets;
    const int e0 = blockIdx.x * kWave;
    const int nenv_w = min(kWave, E - e0);
    const bool valid = lane < nenv_w;
    const int e = valid ? e0 + lane : e0;
    float *row = rows + lane * kRow;
    const finenv_cashpenalty_config &c = p.cfg;

    if (RESET_ONLY) {                                                          // :131-157
        if (role != 0) return;
        const bool sel = valid && (p.mask == nullptr || p.mask[e] != 0);
        const int start = TW_NEXT_START(WIN, KI(FINENV_KI_EPISODE), KI(FINENV_KI_NEXT_START));
        if (sel) {
            tw_win_promote<WIN>(p, e);
            KI(FINENV_KI_START) = start;
            KI(FINENV_KI_DATE_INDEX) = start;
            KI(FINENV_KI_EPISODE) += 1;
            KF(FINENV_KF_TURBULENCE) = 0.0;
            KF(FINENV_KF_SUM_TRADES) = 0.0;
            KF(FINENV_KF_COH) = c.initial_amount;
            for (int i = 0; i < N; ++i) KH(i) = 0.0;
        }
        if (p.obs == nullptr) return;
        row[0] = (float)c.initial_amount;
        for (int i = 0; i < N; ++i) row[1 + i] = 0.0f;
        wave_sync();
        tw_write_rows(p.obs, p, e0, nenv_w, start, __ballot(sel), rows, lane);
        return;
    }

    volatile int *const flag = decided + kWave;
    if (NCH > 0 && role == 0 && lane == 0) *flag = 0;         // (visible after the staging barrier)

    if (role != 0) {
        // ---- streamer ---------------------------------------------------------------------------
        if (NCH == 0) return;                 // rows wider than 320 columns: the trader writes them
        STAMP64(8);
        const int W = p.D - 1 - N;
        const int di_s = tw_date<WIN>(p, KI(FINENV_KI_DATE_INDEX));
        const bool last = tw_last_date<WIN>(di_s, tw_win_end<WIN>(p, e));         // :299
        int ns = 0;
        if (p.auto_reset && __any(last))
            ns = TW_NEXT_START(WIN, KI(FINENV_KI_EPISODE), KI(FINENV_KI_NEXT_START));
        // the row the next observation shows unless a cash shortage ends the episode here
        const int row_spec = last ? (p.auto_reset ? ns : di_s) : di_s + 1;
        tw_gather_closes(trl, p, di_s, lane);
        lds_barrier();                        // staging barrier: the trader reads its close rows
        const unsigned long long valid_mask = __ballot(valid);
        float *const base = p.obs + (size_t)e0 * p.D;
        // market-data columns [64, D) of every row (NCH == 2: 64 < D <= 320): ONE 16-byte-per-lane load
        // and store per row at 4-byte aligned addresses, the last quad shifted back to end at D (a
        // wave's 64 vector-memory slots retire in order, ~47 ns each: the dword form -- up to four
        // loads and four stores per row -- covered rows up to 192 columns in 256 slots, this one
        // rows up to 320 columns in 128), 32 rows of loads ahead of their stores
        typedef float f4 __attribute__((ext_vector_type(4)));
        typedef f4 f4u __attribute__((aligned(4)));
        const int nq = (p.D - kWave + 3) >> 2;                 // quads per row (<= 64)
        const bool qa = NCH > 1 && lane < nq;
        // (> N: market data only.  Lanes past the last quad load it once more and store nothing: every lane
        //  loads, and a quad starting at column 64 of a row narrower than 68 ends past the row -- on the
        //  panel's last date, past the end of panel.info)
        const int qstart = min(kWave + 4 * lane, p.D - 4);
        auto quad_src = [&](int de) {
            return reinterpret_cast<const f4u *>(reinterpret_cast<const char *>(p.panel.info) +
                                                 (size_t)((unsigned)(de * W + qstart - 1 - N) * 4u));
        };
        auto quad_dst = [&](int el) {
            return reinterpret_cast<f4u *>(reinterpret_cast<char *>(base) +
                                           (size_t)((unsigned)(el * p.D + qstart) * 4u));
        };
        if (NCH > 1) {
            for (int g = 0; g < kWave; g += 32) {
                f4 t[32];
#pragma unroll
                for (int j = 0; j < 32; ++j)
                    t[j] = *quad_src(__builtin_amdgcn_readlane(row_spec, g + j));
#pragma unroll
                for (int j = 0; j < 32; ++j) pin(t[j]);
                if (g == 0) STAMP64(9);
#pragma unroll
                for (int j = 0; j < 32; ++j)
                    if (g + j < nenv_w && qa) *quad_dst(g + j) = t[j];
            }
        }
        STAMP64(10);
        while (*flag == 0) __builtin_amdgcn_s_sleep(2);       // the trader has decided every env's row
        asm volatile("" ::: "memory");
        const int dec = decided[lane];
        const unsigned long long fix = __ballot(valid && dec != row_spec);
        const int nfix = __builtin_popcountll(fix);
        float t0[kWave];
        f4 tf[kFix];
        if (W > 0) {
#pragma unroll
            for (int el = 0; el < kWave; ++el) {
                const int de = __builtin_amdgcn_readlane(dec, el);
                const bool ld = lane > N && (NCH > 1 || lane < p.D);
                t0[el] = *at(p.panel.info, (unsigned)(ld ? de * W + lane - 1 - N : 0));
            }
            if (NCH > 1 && nfix > 0) {
                unsigned long long m = fix;
#pragma unroll
                for (int j = 0; j < kFix; ++j) {
                    const int el = m != 0ull ? __builtin_ctzll(m) : 0;
                    m &= m - 1ull;
                    tf[j] = *quad_src(__builtin_amdgcn_readlane(dec, el));
                }
            }
        } else {
#pragma unroll
            for (int el = 0; el < kWave; ++el) t0[el] = 0.0f;
        }
        float *const park = reinterpret_cast<float *>(trl);      // (the trader is done with the closes)
#pragma unroll
        for (int el = 0; el < kWave; ++el) park[el * kWave + lane] = t0[el];
        STAMP64(11);
        lds_barrier();                        // cash / holdings are published; chunk 0 is parked
        tw_head_store<NCH>(p.obs, p, e0, nenv_w, valid_mask, rows, park, lane, kWave / 2, kWave);
        if (NCH > 1 && nfix > 0 && W > 0) {
            unsigned long long m = fix;
#pragma unroll
            for (int j = 0; j < kFix; ++j) {
                if (m == 0ull) continue;
                const int el = __builtin_ctzll(m);
                m &= m - 1ull;
                if (qa) *quad_dst(el) = tf[j];
            }
            if (m != 0ull) tw_write_rows<true>(p.obs, p, e0, nenv_w, dec, m, rows, lane);
        }
        STAMP64(12);
        return;
    }

    STAMP64(0);
    // ---- round trip 1: per-env scalars (the action tile is issued behind them) ----------------
    int di = tw_date<WIN>(p, KI(FINENV_KI_DATE_INDEX));
    const int start = KI(FINENV_KI_START);
    const int end = tw_win_end<WIN>(p, e);
    double coh = KF(FINENV_KF_COH);
    double turb = c.use_turbulence ? KF(FINENV_KF_TURBULENCE) : 0.0;
    double sum_trades = KF(FINENV_KF_SUM_TRADES);
    double logged_total = KF(FINENV_KF_LOGGED_TOTAL), logged_cash = KF(FINENV_KF_LOGGED_CASH);
    // holdings of every asset, kept in registers (issued behind the scalars: one round trip together
    // with the action tile; the first form fetched them in four dependent batches of 8 and read
    // them a second time for the book update: 12 us of a 28 us step)
    double hb[kMaxN], clb[kMaxN];
#pragma unroll
    for (int i = 0; i < kMaxN; ++i) hb[i] = KH(min(i, N - 1));
    stage_action_tile(rows, kRow, p.actions + (size_t)e0 * N, nenv_w, N, p.magicN, lane);
    const int step = di - start;                                                 // current_step
    const bool at_end = tw_last_date<WIN>(di, end);                              // :299
    // closes: every env sits on its own date (random starts), so a per-lane load touches 64
    // different rows per instruction.  Row-wise instead: lane i < N loads close[date_el][i] for one
    // env el per instruction (one 8N-byte segment), all 64 rows in flight, parked in LDS [el][i];
    // each lane then reads its own row back.  The STREAMER does this gather (it needs the dates
    // anyway) while the trader's own loads are in flight: the date -> close-row dependency is off
    // the trader's path, which meets the streamer at the staging barrier.
    if (NCH == 0) {
        tw_gather_closes(trl, p, di, lane);
        wave_sync();
    } else {
        lds_barrier();
    }
#pragma unroll
    for (int i = 0; i < kMaxN; ++i) clb[i] = trl[lane * kClStride + min(i, N - 1)];
    STAMP64(1);
    float act[kMaxN];
#pragma unroll
    for (int i = 0; i < kMaxN; ++i) act[i] = row[min(i, N - 1)];

    double reward;
    bool done = at_end;
    const float hmaxf = (float)c.hmax;
    const bool turbulent = c.use_turbulence && turb >= c.turbulence_threshold;
    double asset_value = 0.0, proceeds = 0.0, spend = 0.0;
#pragma unroll
    for (int i = 0; i < kMaxN; ++i)
        if (i < N) sum_trades += fabs((double)act[i]);                           // :293
    double tr_[kMaxN];
    if (!at_end) {
#pragma unroll
        for (int i = 0; i < kMaxN; ++i) {
            if (i >= N) continue;              // (continue, not break: keeps the loop fully unrollable)
            const double h = hb[i], cl = clb[i];
            asset_value += h * cl;                                               // np.dot, :310
            const float a32 = act[i] * hmaxf;                                    // :257 (float32)
            const float a = cl > 0.0 ? a32 : 0.0f;                               // :260
            double tr;
            if (DISCRETE) {                                                      // :263-274
                // integer-valued doubles instead of int64 arithmetic (exact below 2^53; a software
                // 64-bit division per asset, unrolled, was 30 KB of code)
                const double q = floordiv_true((double)a, cl);
                const double inc = (double)c.shares_increment;
                const double num = q >= 0.0 ? q : q + inc;
                tr = floordiv_true(num, inc) * inc;
            } else {
                tr = (double)a / cl;                                             // :276
            }
            // :279 np.maximum(tr, -h) as compare + select (fmax() quiets both operands first: three
            // extra fp64 instructions per asset at 8 cycles each); a NaN tr (close == 0) gives -h like fmax
            tr = !(tr >= -h) ? -h : tr;
            tr = turbulent ? -h : tr;                                            // :282-287
            tr_[i] = tr;
            proceeds += (tr < 0.0 ? -tr : 0.0) * cl;                             // :323-324
            spend += (tr > 0.0 ? tr : 0.0) * cl;                                 // :328-329
        }
        logged_cash = coh;                                                       // :312-314
        logged_total = coh + asset_value;
    }
    STAMP64(2);
    reward = cp_reward(c, step, logged_total, logged_cash);                      // :317 / :301
    bool keep_buys = true;
    double coh_new = coh;
    if (!at_end) {
        double costs = proceeds * c.sell_cost_pct;                               // :325
        const double coh1 = coh + proceeds;                                      // :326
        costs += spend * c.buy_cost_pct;                                         // :330
        if (spend + costs > coh1) {                                              // :333
            if (c.patient) {                                                     // :334-339
                keep_buys = false;
                spend = 0.0;
                costs = 0.0;
            } else {
                done = true;                                                     // :341-344
            }
        }
        coh_new = coh1 - spend - costs;                                          // :351
    }
    if (p.audit != nullptr && valid) {      // harness log row (account_information / transaction_memory)
        double *au = p.audit + (size_t)e * (size_t)(FINENV_AUDIT_HEAD + N);
        au[FINENV_AUDIT_BEGIN_CASH] = coh;                                       // :312
        au[FINENV_AUDIT_ASSET_VALUE] = asset_value;                              // :313
        au[FINENV_AUDIT_REWARD] = reward;                                        // :317
        au[FINENV_AUDIT_FLAGS] = (double)((at_end ? FINENV_AUDIT_F_LAST_DATE : 0) |
            ((!at_end && (done || !keep_buys)) ? FINENV_AUDIT_F_CASH_SHORTAGE : 0) |
            ((!at_end && turbulent) ? FINENV_AUDIT_F_TURBULENCE : 0));
#pragma unroll
        for (int i = 0; i < kMaxN; ++i) {
            if (i >= N) continue;
            const double tr = at_end ? 0.0 : tr_[i];
            au[FINENV_AUDIT_HEAD + i] = (tr > 0.0 && !keep_buys) ? 0.0 : tr;     // :336 / :345
        }
    }
    const bool advance = !done;
    // ---- the row of the panel each env's next observation shows: date + 1, the unchanged date on a
    // terminal step, or the new starting point on an auto-reset ----------------------------------
    int ns_reset = 0;
    if (p.auto_reset && __any(done))
        ns_reset = TW_NEXT_START(WIN, KI(FINENV_KI_EPISODE), KI(FINENV_KI_NEXT_START));
    const int row_final = done ? (p.auto_reset ? ns_reset : di) : di + 1;
    if (NCH > 0) {                            // publish (LDS is in-order per wave: rows first, then the flag)
        decided[lane] = row_final;
        asm volatile("" ::: "memory");
        *flag = 1;
    }
    if (advance) {
        coh = coh_new;
#pragma unroll
        for (int i = 0; i < kMaxN; ++i) {
            if (i >= N) continue;
            const double tr = tr_[i];
            const double hn = hb[i] + ((tr > 0.0 && !keep_buys) ? 0.0 : tr);     // :352
            if (valid) KH(i) = hn;
            row[1 + i] = (float)hn;
        }
        di += 1;                                                                 // :353
        if (c.use_turbulence) turb = *at(p.panel.turb, (unsigned)di);            // :354-357
    } else {
#pragma unroll
        for (int i = 0; i < kMaxN; ++i)
            if (i < N) row[1 + i] = (float)hb[i];
    }
    STAMP64(3);
    row[0] = (float)coh;
    if (valid) {
        *at(p.reward, (unsigned)e) = (float)reward;
        *at(p.done, (unsigned)e) = done ? 1 : 0;
        KF(FINENV_KF_SUM_TRADES) = sum_trades;
        KF(FINENV_KF_LOGGED_TOTAL) = logged_total;
        KF(FINENV_KF_LOGGED_CASH) = logged_cash;
    }
    wave_sync();
    const unsigned long long valid_mask = __ballot(valid);
    const unsigned long long done_mask = __ballot(done && valid);
    int row_day = di;
    if (done_mask != 0ull) {
        if (p.term_obs != nullptr)
            tw_write_rows<true>(p.term_obs, p, e0, nenv_w, di, done_mask, rows, lane);   // once per episode
        if (p.auto_reset) {                                                      // reset()
            wave_sync();
            if (done) {
                const int ns = ns_reset;
                di = ns;
                row_day = ns;
                coh = c.initial_amount;
                turb = 0.0;
                row[0] = (float)coh;
                for (int i = 0; i < N; ++i) {
                    if (valid) KH(i) = 0.0;
                    row[1 + i] = 0.0f;
                }
                if (valid) {
                    tw_win_promote<WIN>(p, e);
                    KI(FINENV_KI_START) = ns;
                    KI(FINENV_KI_EPISODE) += 1;
                    KF(FINENV_KF_SUM_TRADES) = 0.0;
                }
            }
            wave_sync();
        }
    }
    STAMP64(4);
    if (NCH > 0) {
        lds_barrier();                        // chunk 0 is parked: rows 0..31 here, 32..63 by the streamer
        tw_head_store<NCH>(p.obs, p, e0, nenv_w, valid_mask, rows,
                           reinterpret_cast<const float *>(trl), lane, 0, kWave / 2);
    } else {
        tw_write_rows(p.obs, p, e0, nenv_w, row_day, valid_mask, rows, lane);
    }
    STAMP64(5);
    if (valid) {
        KF(FINENV_KF_COH) = coh;
        KI(FINENV_KI_DATE_INDEX) = di;
        if (c.use_turbulence) KF(FINENV_KF_TURBULENCE) = turb;
    }
}

}  // namespace

struct finenv_cashpenalty : TwoWaveHandle<finenv_cashpenalty_config, finenv_cashpenalty_panel,
                                         finenv_cashpenalty_state> {};

namespace {
// every step kernel runs one block per 64 envs: the wide form (NCH = 0) leaves its second wave idle
struct CpKernels {
    template <int NCH, bool DISCRETE, bool WIN>
    static constexpr auto step() { return &cashpenalty_kernel<false, NCH, DISCRETE, WIN>; }
    static dim3 wide_grid(int E) { return tw_grid(E); }
};
}  // namespace

extern "C" {

int finenv_cashpenalty_create(const finenv_cashpenalty_config *cfg, finenv_cashpenalty **out)
{
    return tw_create(cfg, out, FINENV_CASHPENALTY_MAX_ASSETS, FINENV_CASHPENALTY_F64_FIELDS, 1);
}

void finenv_cashpenalty_destroy(finenv_cashpenalty *h) { delete h; }
const char *finenv_cashpenalty_last_error(const finenv_cashpenalty *h)
{
    return finenv_host::last_error(h);
}
int finenv_cashpenalty_obs_dim(const finenv_cashpenalty *h) { return finenv_host::obs_dim(h); }

int finenv_cashpenalty_bind(finenv_cashpenalty *h, const finenv_cashpenalty_panel *panel,
                            const finenv_cashpenalty_state *st)
{
    return tw_bind(h, panel, st);
}

int finenv_cashpenalty_set_random_start(finenv_cashpenalty *h, int32_t hi, uint64_t seed)
{
    return tw_set_random_start(h, hi, seed);
}

int finenv_cashpenalty_set_audit(finenv_cashpenalty *h, double *audit) { return tw_set_audit(h, audit); }

int finenv_cashpenalty_set_windows(finenv_cashpenalty *h, int32_t *win) { return tw_set_windows(h, win); }

int finenv_cashpenalty_set_history(finenv_cashpenalty *h, const finenv_twowave_history *hist)
{
    return tw_set_history(h, hist);
}

int finenv_cashpenalty_history_arm(finenv_cashpenalty *h, const uint8_t *mask, void *stream)
{
    return finenv_host::history_arm(h, mask, stream, "cashpenalty_history_arm",
                                    tw_launch_history_arm<finenv_cashpenalty>);
}

int finenv_cashpenalty_history_metrics(finenv_cashpenalty *h, double annualization, double *out, void *stream)
{
    return finenv_host::history_metrics(h, annualization, out, stream, "cashpenalty_history_metrics",
                                        tw_history_series<finenv_cashpenalty>);
}

int finenv_cashpenalty_reset(finenv_cashpenalty *h, const uint8_t *mask, float *obs_out,
                             void *stream)
{
    if (const int rc = finenv_host::ready(h, "reset")) return rc;
    const finenv_host::DeviceGuard guard(h->device);
    CpParams p = tw_params<CpParams>(h);
    p.mask = mask;
    p.obs = obs_out;
    const auto reset = p.win != nullptr ? &cashpenalty_kernel<true, 0, false, true>
                                        : &cashpenalty_kernel<true, 0, false, false>;
    hipLaunchKernelGGL(reset, tw_grid(h->cfg.n_envs), dim3(kWave * kWaves), 0, (hipStream_t)stream, p);
    if (h->has_hist) tw_launch_history_arm(h, mask, (hipStream_t)stream);
    return finenv_host::check_launch(h, "cashpenalty_reset");
}

int finenv_cashpenalty_step(finenv_cashpenalty *h, const float *actions, float *obs,
                            float *reward, uint8_t *done, float *term_obs, int32_t auto_reset,
                            void *stream)
{
    return tw_step<CpKernels, CpParams>(h, actions, obs, reward, done, term_obs, auto_reset, stream,
                                        "cashpenalty_step");
}

}  // extern "C"
