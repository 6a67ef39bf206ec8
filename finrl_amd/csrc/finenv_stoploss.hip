// finenv_stoploss.hip -- MI355X (gfx950) kernel + C ABI for the batched stop-loss env
// (finrl/meta/env_stock_trading/env_stocktrading_stoploss.py: step :292-442,
// get_reward :255-290, reset :134-165).
//
// lane = env.  Per-asset books (holdings, previous holdings, the two price-vs-average-buy
// differences, buy counts, average buy price) live in HBM as [N][E] f64 rows, so every per-asset
// access of a wave is one coalesced 512-B row segment.  Three short fp64 passes over the assets:
// (1) previous-state reward terms, (2) transactions + stop-loss override + cash test inputs,
// (3) book update.  Sums run in asset order, like the oracle.
//
// The reference's step() is written once, in the helpers ahead of the kernels: sl_reward, sl_pass1 (the
// reward terms of one asset), sl_closing_diff / sl_transaction (one asset's transaction),
// sl_cash_decision (what the step decides), sl_update / sl_store_book (pass 3 of one asset),
// sl_audit_row, sl_episode_end (terminal observation, auto-reset).  The two step kernels below differ in
// who loads what and when, and in where a transaction waits for pass 3 (registers, or LDS for the
// streamer's assets) -- not in the rule.
//
// Observation rows of up to 320 columns (stoploss_step2_kernel): one 128-thread block per 64 envs,
// two specialised waves --
//   wave 0 "trader"  : passes 1 and 2 over every asset, the cash decision, pass 3 for assets
//                      0..15, scalars, terminal observation / auto-reset.
//   wave 1 "streamer": gathers every env's close row (each env sits on its own date), streams the
//                      market-data chunks of the next observation rows while the trader computes,
//                      loads the books of assets 16.. meanwhile; once the trader has published
//                      its decision (LDS flag, no barrier) it runs pass 3 for those assets from
//                      the transactions the trader parked in LDS, and fetches the observation
//                      chunk that holds cash / holdings.  Two barriers at the end: pass 3 complete,
//                      rows final; both waves then store 32 rows of chunk 0.
// A wave keeps at most 64 vector-memory operations in flight and retires them in order (~47 ns per
// slot under load): the one-wave form (stoploss_kernel, still used for wider rows and for reset)
// pushes ~800 of them per step through one queue.

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
constexpr int kMaxN = FINENV_STOPLOSS_MAX_ASSETS;
struct SlParams : TwoWaveParams<finenv_stoploss_config, finenv_stoploss_panel, finenv_stoploss_state,
                                kMaxN> {};
constexpr int kRow = SlParams::kRow, kClStride = SlParams::kClStride;
constexpr int kWaves = 2;
constexpr int kB = 8;                        // assets per load batch
constexpr int kLdsPerWave = kWave * kRow + kMaxN * kWave * 2;   // rows + f64 transactions [i][lane]
// two-wave step kernel
constexpr int kHalf = 16;                      // assets [0, kHalf): trader's pass 3; the rest: streamer's
constexpr int kL2Rows = kWave * kRow;                          // f32 [el][33]
constexpr int kL2Close = kClStride * kWave * 2;                // f64 closes [el][i]; later: parked chunk 0
constexpr int kL2Trx = (kMaxN - kHalf) * kWave * 2;            // f64 transactions of assets >= kHalf [i][lane]
constexpr int kL2Misc = 6 * kWave + 2;                         // decided, eflags, aflags, ntr (f64), flag
constexpr int kLds2 = kL2Rows + kL2Close + kL2Trx + kL2Misc;
static_assert((kLds2 + kWave) * 4 * 4 <= 160 * 1024, "four blocks per CU");
constexpr int kFix = 4;                        // re-decided rows per block the streamer patches in registers
static_assert(kWave * kWave <= kL2Close, "the parked chunk 0 reuses the close rows");

#define LF(fld) (*at(p.st.f64, (unsigned)(fld) * (unsigned)E + (unsigned)e))
#define LI(fld) (*at(p.st.i32, (unsigned)(fld) * (unsigned)E + (unsigned)e))
#define LV(book, i) LF(FINENV_STOPLOSS_F64_FIELDS + (book) * N + (i))

// get_reward(), :255-290, from its four sums
__device__ __forceinline__ double sl_reward(const finenv_stoploss_config &c, int step,
                                            double total, double cash, double slp_sum,
                                            double lpp_sum, double add)
{
    if (step == 0) return 0.0;
    const double cash_penalty = fmax(0.0, total * c.cash_penalty_proportion - cash);   // :270
    const double slp = step > 1 ? -slp_sum : 0.0;                                       // :271-277
    const double lpp = -lpp_sum;                                                        // :278-280
    const double total_penalty = cash_penalty + slp + lpp;                              // :281
    double r = ((total - total_penalty + add) / c.initial_amount) - 1;                  // :285-287
    r /= (double)step;                                                                  // :288
    return r;
}

// One asset's share of get_reward()'s sums (and of the trade counter), from the books as the
// previous step left them.  The last-date loop (pass 1) and the pass-2 loop of both kernels call it.
__device__ __forceinline__ void sl_pass1(float act, double h, double ph, double ps, double cd,
                                         double &sum_trades, double &slp_sum, double &lpp_sum,
                                         double &add)
{
    sum_trades += fabs((double)act);                                 // :294
    slp_sum += ph * fmin(cd, 0.0);                                   // :262,:273-275
    lpp_sum += h * fmin(ps, 0.0);                                    // :263-265,:278-280
    add += h * fmax(ps, 0.0);                                        // :266-268,:283
}

// closing_diff_avg_buy of one asset: pass 2 takes it for the stop-loss, pass 3 stores it
__device__ __forceinline__ double sl_closing_diff(const finenv_stoploss_config &c, double cl, double abp)
{
    return cl - (c.stoploss_penalty * abp);                          // :350-352
}

// The transaction of one asset (:321-360) from its action, holdings, close and closing_diff_avg_buy;
// flags collects the audit bit of a stop-loss sale.  (The caller computes cd: with cd and the stop-loss
// bit handed back in a struct the one-wave kernel ran 0.4-0.8 % longer, profiles/twowave_passes.md)
__device__ __forceinline__ double sl_transaction(const finenv_stoploss_config &c, float act, double h,
                                                 double cl, double cd, float hmaxf, bool turbulent,
                                                 bool stop_armed, bool discrete, int &flags)
{
    const float a32 = act * hmaxf;                                   // :321 (float32)
    double a = cl > 0.0 ? (double)a32 : 0.0;                         // :326
    a = turbulent ? -(h * cl) : a;                                   // :327-331
    double tr;
    if (discrete) {                                                  // :333-343
        // integer-valued doubles instead of int64 arithmetic (exact below 2^53; a
        // software 64-bit division per asset, unrolled, doubled the kernel's code)
        const double q = cl > 0.0 ? floordiv_true(a, cl) : 0.0;
        const double inc = (double)c.shares_increment;
        const double num = q >= 0.0 ? q : q + inc;
        tr = floordiv_true(num, inc) * inc;
    } else {
        tr = cl > 0.0 ? a / cl : 0.0;                                // :345
    }
    tr = fmax(tr, -h);                                               // :348
    flags |= (stop_armed && cd < 0.0) ? FINENV_AUDIT_F_STOP_LOSS : 0;   // :359-360
    return (stop_armed && cd < 0.0) ? -h : tr;                       // :353-357
}

// What a step decides once every transaction is known (:313-317, :363-383, :414).  A kernel starts
// one with the last date's values (:302-304: done, nothing traded) and replaces it on any other date.
struct SlDecision {
    double coh_new, reward, logged_total, logged_cash;
    bool keep_buys, done;
    int flags;                                 // audit bits
};
__device__ __forceinline__ SlDecision sl_cash_decision(const finenv_stoploss_config &c, int step,
                                                       double coh, double asset_value,
                                                       double proceeds, double spend, bool turbulent,
                                                       double lt_old, double lc_old, double slp_sum,
                                                       double slp_new, double lpp_sum, double add)
{
    SlDecision d;
    d.keep_buys = true;
    d.done = false;
    d.reward = sl_reward(c, step, lt_old, lc_old, slp_sum, lpp_sum, add);        // :313 (stale log)
    d.logged_cash = coh;                                                         // :315-317
    d.logged_total = coh + asset_value;
    double costs = proceeds * c.sell_cost_pct;                                   // :365
    const double coh1 = coh + proceeds;                                          // :366
    costs += spend * c.buy_cost_pct;                                             // :370
    d.flags = turbulent ? FINENV_AUDIT_F_TURBULENCE : 0;
    if (spend + costs > coh1) {                                                  // :372
        d.flags |= FINENV_AUDIT_F_CASH_SHORTAGE;
        if (c.patient) {                                                         // :373-378
            d.keep_buys = false;
            spend = 0.0;
            costs = 0.0;
        } else {                                                                 // :379-383
            d.done = true;
            d.reward = sl_reward(c, step, d.logged_total, d.logged_cash, slp_new, lpp_sum, add);
        }
    }
    d.coh_new = coh1 - spend - costs;                                            // :414
    return d;
}

// pass 3 (:388-428) for one asset: new books from (transaction, close, holdings, average buy price,
// buy count).  Returns the new holdings; *ntr counts applied transactions, *flags the audit bits.
struct SlBook { double ps, hu, nb, abp; };
__device__ __forceinline__ SlBook sl_update(const finenv_stoploss_config &c, double tr0, double cl,
                                            double h, double abp, double nb, bool keep_buys,
                                            double &ntr, int &flags)
{
    const bool sold = tr0 < 0.0;                                     // sells > 0
    const bool bought = tr0 > 0.0;                                   // buys > 0 (:418)
    const double tr = (bought && !keep_buys) ? 0.0 : tr0;            // :376
    const double scp = sold ? cl : 0.0;                              // :388-390
    const bool profit = scp - abp > 0.0;                             // :391-393
    SlBook b;
    b.ps = profit ? cl - (c.min_profit_penalty * abp) : 0.0;         // :395-399
    flags |= b.ps < 0.0 ? FINENV_AUDIT_F_LOW_PROFIT                  // :401-405
                        : (b.ps > 0.0 ? FINENV_AUDIT_F_HIGH_PROFIT : 0);
    ntr += tr != 0.0 ? 1.0 : 0.0;                                    // :411
    b.hu = h + tr;                                                   // :415
    nb += bought ? 1.0 : 0.0;                                        // :419
    const double abp_new = abp + ((cl - abp) / nb);                  // :420-424
    abp = bought ? abp_new : abp;
    const bool held = b.hu > 0.0;                                    // :427-428
    b.nb = held ? nb : 0.0;
    b.abp = held ? abp : 0.0;
    return b;
}

// pass 3's stores of asset i: `h` becomes the previous holdings, `b` the rest
__device__ __forceinline__ void sl_store_book(const SlParams &p, int e, int i, double h, const SlBook &b)
{
    const int E = p.cfg.n_envs, N = p.cfg.n_assets;
    LV(FINENV_LV_PROFIT_SELL_DIFF_AVG_BUY, i) = b.ps;
    LV(FINENV_LV_PREV_HOLDINGS, i) = h;
    LV(FINENV_LV_HOLDINGS, i) = b.hu;
    LV(FINENV_LV_N_BUYS, i) = b.nb;
    LV(FINENV_LV_AVG_BUY_PRICE, i) = b.abp;
}

// harness log row (account_information / transaction_memory); tr_of(i) gives transaction i as pass 2
// left it
template <class Tr>
__device__ __forceinline__ void sl_audit_row(const SlParams &p, int e, double coh_begin,
                                             double asset_value, double reward, int flags,
                                             bool at_end, bool keep_buys, Tr tr_of)
{
    const int N = p.cfg.n_assets;
    double *au = p.audit + (size_t)e * (size_t)(FINENV_AUDIT_HEAD + N);
    au[FINENV_AUDIT_BEGIN_CASH] = coh_begin;                                     // :307
    au[FINENV_AUDIT_ASSET_VALUE] = asset_value;                                  // :311
    au[FINENV_AUDIT_REWARD] = reward;
    au[FINENV_AUDIT_FLAGS] = (double)flags;
#pragma unroll
    for (int i = 0; i < kMaxN; ++i) {
        if (i >= N) continue;
        const double tr = at_end ? 0.0 : tr_of(i);
        au[FINENV_AUDIT_HEAD + i] = (tr > 0.0 && !keep_buys) ? 0.0 : tr;         // :376 / :385
    }
}

// The end of a step in both kernels, once rows[] hold this step's rows: the terminal observation of
// the envs whose episode ended here and, under auto_reset, reset() (:134-165) for them -- next_start()
// gives the restart row; di, coh and turb are the lane's registers, which the kernel stores last.
template <bool WIN, class NextStart>
__device__ __forceinline__ void sl_episode_end(const SlParams &p, int e, int e0, int nenv_w,
                                               float *rows, int lane, bool valid, bool done,
                                               NextStart next_start, int &di, double &coh,
                                               double &turb)
{
    const int E = p.cfg.n_envs, N = p.cfg.n_assets;
    float *row = rows + lane * kRow;
    const unsigned long long done_mask = __ballot(done && valid);
    if (done_mask == 0ull) return;
    if (p.term_obs != nullptr)
        tw_write_rows<true>(p.term_obs, p, e0, nenv_w, di, done_mask, rows, lane);   // once per episode
    if (!p.auto_reset) return;
    wave_sync();                                                                 // reset()
    if (done) {
        const int ns = next_start();
        di = ns;
        coh = p.cfg.initial_amount;
        turb = 0.0;
        row[0] = (float)coh;
        for (int i = 0; i < N; ++i) row[1 + i] = 0.0f;
        if (valid) {
            for (int i = 0; i < FINENV_STOPLOSS_BOOKS * N; ++i) LV(0, i) = 0.0;
            tw_win_promote<WIN>(p, e);
            LI(FINENV_LI_START) = ns;
            LI(FINENV_LI_EPISODE) += 1;
            LF(FINENV_LF_SUM_TRADES) = 0.0;
            LF(FINENV_LF_ACTUAL_NUM_TRADES) = 0.0;
        }
    }
    wave_sync();
}

// The one-wave kernel: reset, and steps whose observation rows are wider than 320 columns.  (WIN =
// per-env episode windows, finenv_stoploss_set_windows: the helpers in finenv_twowave.h)
template <bool RESET_ONLY, bool WIN>
__global__ void __launch_bounds__(kWave *kWaves, 1) stoploss_kernel(const SlParams p)
{
    __shared__ __attribute__((aligned(16))) float lds_all[kWaves * kLdsPerWave];
    const int lane = threadIdx.x & (kWave - 1);
    const int wib = threadIdx.x >> 6;
    float *rows = lds_all + wib * kLdsPerWave;
    const int E = p.cfg.n_envs, N = p.cfg.n_assets;
    const int e0 = (blockIdx.x * kWaves + wib) * kWave;
    if (e0 >= E) return;
    const int nenv_w = min(kWave, E - e0);
    const bool valid = lane < nenv_w;
    const int e = valid ? e0 + lane : e0;
    float *row = rows + lane * kRow;
    const finenv_stoploss_config &c = p.cfg;

    if (RESET_ONLY) {                                                          // :134-165
        const bool sel = valid && (p.mask == nullptr || p.mask[e] != 0);
        const int start = TW_NEXT_START(WIN, LI(FINENV_LI_EPISODE), LI(FINENV_LI_NEXT_START));
        if (sel) {
            tw_win_promote<WIN>(p, e);
            LI(FINENV_LI_START) = start;
            LI(FINENV_LI_DATE_INDEX) = start;
            LI(FINENV_LI_EPISODE) += 1;
            LF(FINENV_LF_TURBULENCE) = 0.0;
            LF(FINENV_LF_SUM_TRADES) = 0.0;
            LF(FINENV_LF_ACTUAL_NUM_TRADES) = 0.0;
            LF(FINENV_LF_COH) = c.initial_amount;
            for (int i = 0; i < FINENV_STOPLOSS_BOOKS * N; ++i) LV(0, i) = 0.0;
        }
        if (p.obs == nullptr) return;
        row[0] = (float)c.initial_amount;
        for (int i = 0; i < N; ++i) row[1 + i] = 0.0f;
        wave_sync();
        tw_write_rows(p.obs, p, e0, nenv_w, start, __ballot(sel), rows, lane);
        return;
    }

    // ---- action tile -> LDS rows --------------------------------------------------------------
    stage_action_tile(rows, kRow, p.actions + (size_t)e0 * N, nenv_w, N, p.magicN, lane);
    int di = tw_date<WIN>(p, LI(FINENV_LI_DATE_INDEX));
    const int start = LI(FINENV_LI_START);
    const int end = tw_win_end<WIN>(p, e);
    double coh = LF(FINENV_LF_COH);
    double turb = c.use_turbulence ? LF(FINENV_LF_TURBULENCE) : 0.0;
    double sum_trades = LF(FINENV_LF_SUM_TRADES);
    const double lt_old = LF(FINENV_LF_LOGGED_TOTAL), lc_old = LF(FINENV_LF_LOGGED_CASH);
    double actual_num_trades = LF(FINENV_LF_ACTUAL_NUM_TRADES);
    const int step = di - start;                                                 // current_step
    const bool at_end = tw_last_date<WIN>(di, end);                              // :302
    const unsigned cb = (unsigned)(di * N);
    wave_sync();

    // ---- pass 1: reward terms of the state as the previous step left it (:313 / :304).  On every
    // step but the last date these sums ride along in pass 2 (same assets, same order), which saves
    // re-reading the holdings and previous-holdings books: the three-pass form moved 1.34x the
    // algorithmic bytes (PMC, profiles/side_traffic.json).
    double slp_sum = 0.0, lpp_sum = 0.0, add = 0.0;
    // (every per-asset loop below runs in batches of kB assets with the batch's global loads issued
    //  first: a rolled loop exposes one HBM round trip per asset at one wave per SIMD)
    if (at_end) {
        for (int i0 = 0; i0 < N; i0 += kB) {
            double hh[kB], ps[kB], ph[kB], cd[kB];
#pragma unroll
            for (int j = 0; j < kB; ++j) {
                const int i = min(i0 + j, N - 1);
                hh[j] = LV(FINENV_LV_HOLDINGS, i);
                ps[j] = LV(FINENV_LV_PROFIT_SELL_DIFF_AVG_BUY, i);
                ph[j] = LV(FINENV_LV_PREV_HOLDINGS, i);
                cd[j] = LV(FINENV_LV_CLOSING_DIFF_AVG_BUY, i);
            }
#pragma unroll
            for (int j = 0; j < kB; ++j) { pin(hh[j]); pin(ps[j]); pin(ph[j]); pin(cd[j]); }
#pragma unroll
            for (int j = 0; j < kB; ++j) {
                if (i0 + j >= N) continue;
                sl_pass1(row[i0 + j], hh[j], ph[j], ps[j], cd[j], sum_trades, slp_sum, lpp_sum, add);
            }
        }
    }
    SlDecision d = {coh, at_end ? sl_reward(c, step, lt_old, lc_old, slp_sum, lpp_sum, add) : 0.0,   // :304
                    lt_old, lc_old, true, at_end, at_end ? FINENV_AUDIT_F_LAST_DATE : 0};

    // ---- pass 2: transactions (:320-357), proceeds / spend (:363-370) --------------------------
    const float hmaxf = (float)c.hmax;
    const bool turbulent = c.use_turbulence && turb >= c.turbulence_threshold;
    const bool stop_armed = coh >= c.stoploss_penalty * c.initial_amount;        // :353
    double asset_value = 0.0, proceeds = 0.0, spend = 0.0, slp_new = 0.0;
    const double coh_begin = coh;
    int audit_flags = d.flags;
    // holdings, closes, average buy prices and transactions stay in statically indexed registers
    // from pass 2 to pass 3 (the batch loops are unrolled over the kMaxN slots): pass 3 used to
    // re-read the first three (1.22x the algorithmic traffic, profiles/side_traffic.json)
    double hS[kMaxN], clS[kMaxN], abS[kMaxN], trS[kMaxN];
    if (!at_end) {
#pragma unroll
        for (int i0 = 0; i0 < kMaxN; i0 += kB) {
            if (i0 >= N) continue;
            double hb[kB], clb[kB], ab[kB], pb[kB], pso[kB], cdo[kB];
#pragma unroll
            for (int j = 0; j < kB; ++j) {
                const int i = min(i0 + j, N - 1);
                hb[j] = LV(FINENV_LV_HOLDINGS, i);
                clb[j] = *at(p.panel.close, cb + (unsigned)i);
                ab[j] = LV(FINENV_LV_AVG_BUY_PRICE, i);
                pb[j] = LV(FINENV_LV_PREV_HOLDINGS, i);
                pso[j] = LV(FINENV_LV_PROFIT_SELL_DIFF_AVG_BUY, i);      // pass-1 terms (old books)
                cdo[j] = LV(FINENV_LV_CLOSING_DIFF_AVG_BUY, i);
            }
#pragma unroll
            for (int j = 0; j < kB; ++j) {
                pin(hb[j]); pin(clb[j]); pin(ab[j]); pin(pb[j]); pin(pso[j]); pin(cdo[j]);
            }
#pragma unroll
            for (int j = 0; j < kB; ++j) {
                const int i = i0 + j;
                if (i >= N) continue;          // (continue, not break: keeps the loop fully unrollable)
                const double h = hb[j], cl = clb[j], abp = ab[j];
                sl_pass1(row[i], h, pb[j], pso[j], cdo[j], sum_trades, slp_sum, lpp_sum, add);
                asset_value += h * cl;                                           // :311
                const double cd = sl_closing_diff(c, cl, abp);
                if (valid) LV(FINENV_LV_CLOSING_DIFF_AVG_BUY, i) = cd;
                slp_new += pb[j] * fmin(cd, 0.0);
                const double tr = sl_transaction(c, row[i], h, cl, cd, hmaxf, turbulent, stop_armed,
                                                 c.discrete_actions, audit_flags);
                hS[i] = h;
                clS[i] = cl;
                abS[i] = abp;
                trS[i] = tr;
                proceeds += (tr < 0.0 ? -tr : 0.0) * cl;                         // :363-364
                spend += (tr > 0.0 ? tr : 0.0) * cl;                             // :368-369
            }
        }
        d = sl_cash_decision(c, step, coh, asset_value, proceeds, spend, turbulent, lt_old, lc_old,
                             slp_sum, slp_new, lpp_sum, add);
        audit_flags |= d.flags;
    }
    const bool done = d.done;

    // ---- pass 3: book update (:388-428) --------------------------------------------------------
    const bool advance = !done;
    if (advance) {
        coh = d.coh_new;
        double ntr = 0.0;
        // buy counts: the one book pass 2 did not read -- all of them in one batch, before this
        // pass's first store
        double nbS[kMaxN];
#pragma unroll
        for (int i = 0; i < kMaxN; ++i) nbS[i] = LV(FINENV_LV_N_BUYS, min(i, N - 1));
#pragma unroll
        for (int i0 = 0; i0 < kMaxN; i0 += kB) {
            if (i0 >= N) continue;
#pragma unroll
            for (int j = 0; j < kB; ++j) {
                const int i = i0 + j;
                if (i >= N) continue;          // (continue, not break: keeps the loop fully unrollable)
                const SlBook b = sl_update(c, trS[i], clS[i], hS[i], abS[i], nbS[i], d.keep_buys, ntr,
                                           audit_flags);
                if (valid) sl_store_book(p, e, i, hS[i], b);
                row[1 + i] = (float)b.hu;
            }
        }
        actual_num_trades = ntr;
        di += 1;                                                                 // :430
        if (c.use_turbulence) turb = *at(p.panel.turb, (unsigned)di);            // :431-434
    } else {
        for (int i = 0; i < N; ++i) row[1 + i] = (float)LV(FINENV_LV_HOLDINGS, i);
    }
    if (p.audit != nullptr && valid)
        sl_audit_row(p, e, coh_begin, asset_value, d.reward, audit_flags, at_end, d.keep_buys,
                     [&](int i) { return trS[i]; });
    row[0] = (float)coh;
    if (valid) {
        *at(p.reward, (unsigned)e) = (float)d.reward;
        *at(p.done, (unsigned)e) = done ? 1 : 0;
        LF(FINENV_LF_SUM_TRADES) = sum_trades;
        LF(FINENV_LF_LOGGED_TOTAL) = d.logged_total;
        LF(FINENV_LF_LOGGED_CASH) = d.logged_cash;
        LF(FINENV_LF_ACTUAL_NUM_TRADES) = actual_num_trades;
    }
    wave_sync();
    const unsigned long long valid_mask = __ballot(valid);
    sl_episode_end<WIN>(p, e, e0, nenv_w, rows, lane, valid, done, [&]() {
        return TW_NEXT_START(WIN, LI(FINENV_LI_EPISODE), LI(FINENV_LI_NEXT_START));
    }, di, coh, turb);
    tw_write_rows(p.obs, p, e0, nenv_w, di, valid_mask, rows, lane);
    if (valid) {
        LF(FINENV_LF_COH) = coh;
        LI(FINENV_LI_DATE_INDEX) = di;
        if (c.use_turbulence) LF(FINENV_LF_TURBULENCE) = turb;
    }
}

template <int NCH, bool DISCRETE, bool WIN>
__global__ void __launch_bounds__(kWave *kWaves) __attribute__((amdgpu_waves_per_eu(2)))
stoploss_step2_kernel(const SlParams p)
{
    // (WIN: + [lane] the active ends, which the streamer loads beside its date index and hands to the
    //  trader over the staging barrier: the trader has no register to spare)
    __shared__ __attribute__((aligned(16))) float lds_all[kLds2 + (WIN ? kWave : 0)];
    int *const wend = reinterpret_cast<int *>(lds_all + kLds2);
    const int lane = threadIdx.x & (kWave - 1);
    const int role = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float *rows = lds_all;
    double *trl = reinterpret_cast<double *>(lds_all + kL2Rows);
    double *trx = reinterpret_cast<double *>(lds_all + kL2Rows + kL2Close);
    int *decided = reinterpret_cast<int *>(lds_all + kL2Rows + kL2Close + kL2Trx);
    int *eflags = decided + kWave;             // bit 0 advance, bit 1 keep_buys, bit 2 last date
    int *aflags = eflags + kWave;              // audit bits of the streamer's pass 3
    double *ntrx = reinterpret_cast<double *>(aflags + kWave);   // its count of applied transactions
    volatile int *const flag = reinterpret_cast<int *>(ntrx + kWave);
    const int E = p.cfg.n_envs, N = p.cfg.n_assets;
    const int e0 = blockIdx.x * kWave;
    const int nenv_w = min(kWave, E - e0);
    const bool valid = lane < nenv_w;
    const int e = valid ? e0 + lane : e0;
    float *row = rows + lane * kRow;
    const finenv_stoploss_config &c = p.cfg;
    const int W = p.D - 1 - N;
    if (role == 0 && lane == 0) *flag = 0;     // (visible after the staging barrier)

    if (role != 0) {
        // ================================ streamer ===============================================
        STAMP64(8);
        const int di_s = tw_date<WIN>(p, LI(FINENV_LI_DATE_INDEX));
        const int end_s = tw_win_end<WIN>(p, e);
        const bool last = tw_last_date<WIN>(di_s, end_s);                         // :302
        if (WIN) wend[lane] = end_s;
        int ns = 0;
        if (p.auto_reset && __any(last))
            ns = TW_NEXT_START(WIN, LI(FINENV_LI_EPISODE), LI(FINENV_LI_NEXT_START));
        // the row the next observation shows unless a cash shortage ends the episode here
        const int row_spec = last ? (p.auto_reset ? ns : di_s) : di_s + 1;
        tw_gather_closes(trl, p, di_s, lane);
        lds_barrier();                        // staging barrier: the trader reads its close rows
        STAMP64(9);
        const unsigned long long valid_mask = __ballot(valid);
        float *const base = p.obs + (size_t)e0 * p.D;
        // market-data columns [64, D) of every row (NCH == 2: 64 < D <= 320): ONE 16-byte-per-lane load
        // and store per row at 4-byte aligned addresses, the last quad shifted back to end at D; 32
        // rows of loads ahead of their stores (see finenv_cashpenalty.hip)
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
#pragma unroll
                for (int j = 0; j < 32; ++j)
                    if (g + j < nenv_w && qa) *quad_dst(g + j) = t[j];
            }
        }
        STAMP64(10);
        // books of its assets (they do not depend on the decision): in flight while it waits
        double hx[kMaxN - kHalf], ax[kMaxN - kHalf], nx[kMaxN - kHalf];
#pragma unroll
        for (int u = 0; u < kMaxN - kHalf; ++u) {
            const int i = min(kHalf + u, N - 1);
            hx[u] = LV(FINENV_LV_HOLDINGS, i);
            ax[u] = LV(FINENV_LV_AVG_BUY_PRICE, i);
            nx[u] = LV(FINENV_LV_N_BUYS, i);
        }
        while (*flag == 0) __builtin_amdgcn_s_sleep(2);       // the trader has decided
        asm volatile("" ::: "memory");
        STAMP64(11);
        const int dec = decided[lane], ef = eflags[lane];
        const bool adv = (ef & 1) != 0, keepb = (ef & 2) != 0, at_end_s = (ef & 4) != 0;
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
        // ---- pass 3 for assets kHalf.. (:388-428) -------------------------------------------------
        double ntr = 0.0;
        int fl = 0;
        const bool keep_cd = valid && !at_end_s && !(p.auto_reset && !adv);   // (a reset zeroes the books)
#pragma unroll
        for (int u = 0; u < kMaxN - kHalf; ++u) {
            const int i = kHalf + u;
            if (i >= N) continue;              // (continue, not break: keeps the loop fully unrollable)
            const double cl = trl[lane * kClStride + i], h = hx[u], abp = ax[u];
            if (keep_cd) LV(FINENV_LV_CLOSING_DIFF_AVG_BUY, i) = sl_closing_diff(c, cl, abp);
            const SlBook b = sl_update(c, trx[u * kWave + lane], cl, h, abp, nx[u], keepb, ntr, fl);
            if (valid && adv) sl_store_book(p, e, i, h, b);
            row[1 + i] = (float)(adv ? b.hu : h);
        }
        ntrx[lane] = adv ? ntr : 0.0;
        aflags[lane] = adv ? fl : 0;
        STAMP64(12);
        lds_barrier();                        // #1: pass 3 complete, rows[] hold every new holding
        float *const park = reinterpret_cast<float *>(trl);      // (nobody reads the closes any more)
#pragma unroll
        for (int el = 0; el < kWave; ++el) park[el * kWave + lane] = t0[el];
        lds_barrier();                        // #2: terminal observation / reset done, chunk 0 parked
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
        STAMP64(13);
        return;
    }

    // ==================================== trader =================================================
    STAMP64(0);
    int di = tw_date<WIN>(p, LI(FINENV_LI_DATE_INDEX));
    const int start = LI(FINENV_LI_START);
    double coh = LF(FINENV_LF_COH);
    double turb = c.use_turbulence ? LF(FINENV_LF_TURBULENCE) : 0.0;
    double sum_trades = LF(FINENV_LF_SUM_TRADES);
    const double lt_old = LF(FINENV_LF_LOGGED_TOTAL), lc_old = LF(FINENV_LF_LOGGED_CASH);
    double actual_num_trades = LF(FINENV_LF_ACTUAL_NUM_TRADES);
    stage_action_tile(rows, kRow, p.actions + (size_t)e0 * N, nenv_w, N, p.magicN, lane);
    const int step = di - start;                                                 // current_step
    bool at_end = tw_last_date<false>(di, c.n_days);                             // :302
    lds_barrier();                            // staging barrier: close rows gathered by the streamer
    if (WIN) at_end = tw_last_date<WIN>(di, wend[lane]);                         // (its active ends too)
    STAMP64(1);

    double slp_sum = 0.0, lpp_sum = 0.0, add = 0.0;
    double hS[kHalf], abS[kHalf], trS[kHalf];  // own assets, pass 2 -> pass 3 (statically indexed)
#pragma unroll
    for (int i = 0; i < kHalf; ++i) { hS[i] = 0.0; abS[i] = 0.0; trS[i] = 0.0; }
    // ---- pass 1 (last date only): reward terms of the state as the previous step left it (:304) --
    if (at_end) {
#pragma unroll
        for (int i0 = 0; i0 < kMaxN; i0 += kB) {
            if (i0 >= N) continue;
            double hh[kB], ps[kB], ph[kB], cd[kB];
#pragma unroll
            for (int j = 0; j < kB; ++j) {
                const int i = min(i0 + j, N - 1);
                hh[j] = LV(FINENV_LV_HOLDINGS, i);
                ps[j] = LV(FINENV_LV_PROFIT_SELL_DIFF_AVG_BUY, i);
                ph[j] = LV(FINENV_LV_PREV_HOLDINGS, i);
                cd[j] = LV(FINENV_LV_CLOSING_DIFF_AVG_BUY, i);
            }
#pragma unroll
            for (int j = 0; j < kB; ++j) { pin(hh[j]); pin(ps[j]); pin(ph[j]); pin(cd[j]); }
#pragma unroll
            for (int j = 0; j < kB; ++j) {
                const int i = i0 + j;
                if (i >= N) continue;
                sl_pass1(row[i], hh[j], ph[j], ps[j], cd[j], sum_trades, slp_sum, lpp_sum, add);
                if (i < kHalf) hS[i < kHalf ? i : 0] = hh[j];
                else trx[(i >= kHalf ? i - kHalf : 0) * kWave + lane] = 0.0;
            }
        }
    }
    SlDecision d = {coh, at_end ? sl_reward(c, step, lt_old, lc_old, slp_sum, lpp_sum, add) : 0.0,   // :304
                    lt_old, lc_old, true, at_end, at_end ? FINENV_AUDIT_F_LAST_DATE : 0};

    // ---- pass 2: transactions (:320-357), proceeds / spend (:363-370) --------------------------
    const float hmaxf = (float)c.hmax;
    const bool turbulent = c.use_turbulence && turb >= c.turbulence_threshold;
    const bool stop_armed = coh >= c.stoploss_penalty * c.initial_amount;        // :353
    double asset_value = 0.0, proceeds = 0.0, spend = 0.0, slp_new = 0.0;
    const double coh_begin = coh;
    int audit_flags = d.flags;
    if (!at_end) {
#pragma unroll
        for (int i0 = 0; i0 < kMaxN; i0 += kB) {
            if (i0 >= N) continue;
            double hb[kB], ab[kB], pb[kB], pso[kB], cdo[kB];
#pragma unroll
            for (int j = 0; j < kB; ++j) {
                const int i = min(i0 + j, N - 1);
                hb[j] = LV(FINENV_LV_HOLDINGS, i);
                ab[j] = LV(FINENV_LV_AVG_BUY_PRICE, i);
                pb[j] = LV(FINENV_LV_PREV_HOLDINGS, i);
                pso[j] = LV(FINENV_LV_PROFIT_SELL_DIFF_AVG_BUY, i);      // pass-1 terms (old books)
                cdo[j] = LV(FINENV_LV_CLOSING_DIFF_AVG_BUY, i);
            }
#pragma unroll
            for (int j = 0; j < kB; ++j) {
                pin(hb[j]); pin(ab[j]); pin(pb[j]); pin(pso[j]); pin(cdo[j]);
            }
#pragma unroll
            for (int j = 0; j < kB; ++j) {
                const int i = i0 + j;
                if (i >= N) continue;          // (continue, not break: keeps the loop fully unrollable)
                const double h = hb[j], cl = trl[lane * kClStride + i], abp = ab[j];
                sl_pass1(row[i], h, pb[j], pso[j], cdo[j], sum_trades, slp_sum, lpp_sum, add);
                asset_value += h * cl;                                           // :311
                const double cd = sl_closing_diff(c, cl, abp);
                slp_new += pb[j] * fmin(cd, 0.0);
                const double tr = sl_transaction(c, row[i], h, cl, cd, hmaxf, turbulent, stop_armed, DISCRETE,
                                                 audit_flags);
                if (i < kHalf) {
                    hS[i < kHalf ? i : 0] = h;
                    abS[i < kHalf ? i : 0] = abp;
                    trS[i < kHalf ? i : 0] = tr;
                } else {
                    trx[(i >= kHalf ? i - kHalf : 0) * kWave + lane] = tr;   // for the streamer's pass 3
                }
                proceeds += (tr < 0.0 ? -tr : 0.0) * cl;                         // :363-364
                spend += (tr > 0.0 ? tr : 0.0) * cl;                             // :368-369
            }
        }
        d = sl_cash_decision(c, step, coh, asset_value, proceeds, spend, turbulent, lt_old, lc_old,
                             slp_sum, slp_new, lpp_sum, add);
        audit_flags |= d.flags;
    }
    const bool done = d.done, keep_buys = d.keep_buys, advance = !done;
    STAMP64(2);
    // ---- the decision is published (LDS is in-order per wave: data first, then the flag) --------
    int ns_reset = 0;
    if (p.auto_reset && __any(done))
        ns_reset = TW_NEXT_START(WIN, LI(FINENV_LI_EPISODE), LI(FINENV_LI_NEXT_START));
    const int row_final = done ? (p.auto_reset ? ns_reset : di) : di + 1;
    decided[lane] = row_final;
    eflags[lane] = (advance ? 1 : 0) | (keep_buys ? 2 : 0) | (at_end ? 4 : 0);
    asm volatile("" ::: "memory");
    *flag = 1;

    // ---- pass 3 for assets 0..kHalf-1 (:388-428) ------------------------------------------------
    double ntr = 0.0;
    {
        double nbS[kHalf];
#pragma unroll
        for (int i = 0; i < kHalf; ++i) nbS[i] = LV(FINENV_LV_N_BUYS, min(i, N - 1));
        const bool keep_cd = valid && !at_end && !(p.auto_reset && !advance);    // (a reset zeroes the books)
#pragma unroll
        for (int i = 0; i < kHalf; ++i) {
            if (i >= N) continue;
            const double cl = trl[lane * kClStride + i], h = hS[i], abp = abS[i];
            if (keep_cd) LV(FINENV_LV_CLOSING_DIFF_AVG_BUY, i) = sl_closing_diff(c, cl, abp);
            int fl = 0;
            double nt = 0.0;
            const SlBook b = sl_update(c, trS[i], cl, h, abp, nbS[i], keep_buys, nt, fl);
            if (advance) {
                ntr += nt;
                audit_flags |= fl;
                if (valid) sl_store_book(p, e, i, h, b);
            }
            row[1 + i] = (float)(advance ? b.hu : h);
        }
    }
    if (advance) {
        coh = d.coh_new;
        di += 1;                                                                 // :430
        if (c.use_turbulence) turb = *at(p.panel.turb, (unsigned)di);            // :431-434
    }
    STAMP64(3);
    lds_barrier();                            // #1: the streamer's pass 3 is complete
    STAMP64(4);
    if (advance) {
        actual_num_trades = ntr + ntrx[lane];    // (counts: exact in any order)
        audit_flags |= aflags[lane];
    }
    if (p.audit != nullptr && valid)
        sl_audit_row(p, e, coh_begin, asset_value, d.reward, audit_flags, at_end, keep_buys, [&](int i) {
            return i < kHalf ? trS[i < kHalf ? i : 0] : trx[(i >= kHalf ? i - kHalf : 0) * kWave + lane];
        });
    row[0] = (float)coh;
    if (valid) {
        *at(p.reward, (unsigned)e) = (float)d.reward;
        *at(p.done, (unsigned)e) = done ? 1 : 0;
        LF(FINENV_LF_SUM_TRADES) = sum_trades;
        LF(FINENV_LF_LOGGED_TOTAL) = d.logged_total;
        LF(FINENV_LF_LOGGED_CASH) = d.logged_cash;
        LF(FINENV_LF_ACTUAL_NUM_TRADES) = actual_num_trades;
    }
    wave_sync();
    const unsigned long long valid_mask = __ballot(valid);
    sl_episode_end<WIN>(p, e, e0, nenv_w, rows, lane, valid, done, [&]() { return ns_reset; }, di, coh,
                        turb);
    STAMP64(5);
    lds_barrier();                            // #2: rows final, chunk 0 parked by the streamer
    tw_head_store<NCH>(p.obs, p, e0, nenv_w, valid_mask, rows, reinterpret_cast<const float *>(trl),
                       lane, 0, kWave / 2);
    STAMP64(6);
    if (valid) {
        LF(FINENV_LF_COH) = coh;
        LI(FINENV_LI_DATE_INDEX) = di;
        if (c.use_turbulence) LF(FINENV_LF_TURBULENCE) = turb;
    }
}

}  // namespace

struct finenv_stoploss : TwoWaveHandle<finenv_stoploss_config, finenv_stoploss_panel,
                                      finenv_stoploss_state> {};

namespace {
dim3 sl_grid(int E)
{
    const int waves = (E + kWave - 1) / kWave;
    return dim3((unsigned)((waves + kWaves - 1) / kWaves));
}
// rows of up to 320 columns: the two-wave kernel; wider rows: the one-wave kernel, two 64-env groups per block
struct SlKernels {
    template <int NCH, bool DISCRETE, bool WIN>
    static constexpr auto step()
    {
        if constexpr (NCH == 0) return &stoploss_kernel<false, WIN>;
        else return &stoploss_step2_kernel<NCH, DISCRETE, WIN>;
    }
    static dim3 wide_grid(int E) { return sl_grid(E); }
};
}  // namespace

extern "C" {

int finenv_stoploss_create(const finenv_stoploss_config *cfg, finenv_stoploss **out)
{
    return tw_create(cfg, out, FINENV_STOPLOSS_MAX_ASSETS, FINENV_STOPLOSS_F64_FIELDS,
                     FINENV_STOPLOSS_BOOKS);
}

void finenv_stoploss_destroy(finenv_stoploss *h) { delete h; }
const char *finenv_stoploss_last_error(const finenv_stoploss *h)
{
    return finenv_host::last_error(h);
}
int finenv_stoploss_obs_dim(const finenv_stoploss *h) { return finenv_host::obs_dim(h); }

int finenv_stoploss_bind(finenv_stoploss *h, const finenv_stoploss_panel *panel,
                         const finenv_stoploss_state *st)
{
    return tw_bind(h, panel, st);
}

int finenv_stoploss_set_random_start(finenv_stoploss *h, int32_t hi, uint64_t seed)
{
    return tw_set_random_start(h, hi, seed);
}

int finenv_stoploss_set_audit(finenv_stoploss *h, double *audit) { return tw_set_audit(h, audit); }

int finenv_stoploss_set_windows(finenv_stoploss *h, int32_t *win) { return tw_set_windows(h, win); }

int finenv_stoploss_set_history(finenv_stoploss *h, const finenv_twowave_history *hist)
{
    return tw_set_history(h, hist);
}

int finenv_stoploss_history_arm(finenv_stoploss *h, const uint8_t *mask, void *stream)
{
    return finenv_host::history_arm(h, mask, stream, "stoploss_history_arm",
                                    tw_launch_history_arm<finenv_stoploss>);
}

int finenv_stoploss_history_metrics(finenv_stoploss *h, double annualization, double *out, void *stream)
{
    return finenv_host::history_metrics(h, annualization, out, stream, "stoploss_history_metrics",
                                        tw_history_series<finenv_stoploss>);
}

int finenv_stoploss_reset(finenv_stoploss *h, const uint8_t *mask, float *obs_out, void *stream)
{
    if (const int rc = finenv_host::ready(h, "reset")) return rc;
    const finenv_host::DeviceGuard guard(h->device);
    SlParams p = tw_params<SlParams>(h);
    p.mask = mask;
    p.obs = obs_out;
    const auto reset = p.win != nullptr ? &stoploss_kernel<true, true> : &stoploss_kernel<true, false>;
    hipLaunchKernelGGL(reset, sl_grid(h->cfg.n_envs), dim3(kWave * kWaves), 0, (hipStream_t)stream, p);
    if (h->has_hist) tw_launch_history_arm(h, mask, (hipStream_t)stream);
    return finenv_host::check_launch(h, "stoploss_reset");
}

int finenv_stoploss_step(finenv_stoploss *h, const float *actions, float *obs, float *reward,
                         uint8_t *done, float *term_obs, int32_t auto_reset, void *stream)
{
    return tw_step<SlKernels, SlParams>(h, actions, obs, reward, done, term_obs, auto_reset, stream,
                                        "stoploss_step");
}

}  // extern "C"
