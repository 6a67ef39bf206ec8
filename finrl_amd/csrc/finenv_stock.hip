// finenv_stock.hip -- MI355X (gfx950) kernels + C ABI for the batched StockTradingEnv.
//
// Replaces the per-timestep work of the reference's
//   finrl/meta/env_stock_trading/env_stocktrading.py  step() :220-357, reset() :359-393,
//   _sell_stock :102-169, _buy_stock :171-213, _update_state :453-478
// for E independent environments in one launch.  Not a translation: the reference is a
// Python list + pandas object per env; here the state is a structure-of-arrays in HBM and
// one wavefront lane owns one environment.
//
// Mapping (see DESIGN.md "stock_step"; kernels in finenv_stock_kernels.inc / finenv_stock_wide.inc,
// compiled per padded ticker count in finenv_stock_np{32,64,128}.hip):
//   * lane = env; one 128-thread block per 64 envs with TWO SPECIALISED WAVES: the "trader" owns
//     the env state (staging, sort, sells, buys, assets, reward, state write-back), the "streamer"
//     writes the market-data part of the observation rows from the first microsecond on; they meet
//     at one hand-off barrier, after which both write the rows' cash / holdings chunk(s);
//   * the wave's [64][N] action tile is read coalesced and transposed through LDS;
//   * (action, ticker) pairs become composite int keys per lane, sorted in VGPRs by a Batcher
//     network == the reference's stable argsort order;
//   * sells then buys walk the sorted keys; holdings live in LDS as [ticker][lane]; the cash chain
//     is fp64 with the reference's operation order (-ffp-contract=off), floor division is exact
//     (reciprocal + FMA-remainder correction);
//   * the [64][D] f32 observation block -- 76 % of all bytes -- comes from a pre-packed f32 panel
//     row (L2-resident); cash / holdings are patched in from LDS.
// HBM-bound by design (no MFMA: there is no contraction here).

#include "finenv_stock_common.h"

namespace {

// end_total_asset of env e from its state in memory (:226-228, :344-347): cash + sum_i close * shares,
// summed sequentially from ticker 0 on the prices of the current observation.  `p` is any argument
// struct with the state blocks in p.st (the SF / SI / HOLD accessors).  One lane owns the env, so the N
// (price, shares) pairs are loaded kAssetBatch at a time before the first add of the batch: a rolled
// load / wait / add loop exposes one memory round trip per ticker (the callers run one wave per SIMD).
constexpr int kAssetBatch = 16;
template <typename P>
__device__ __forceinline__ double end_total_asset(const P &p, const double *close, int E, int N, int e)
{
    const double *prow = close + (size_t)SI(FINENV_SI_PRICE_DAY) * N;
    double s = 0.0;
    for (int i0 = 0; i0 < N; i0 += kAssetBatch) {
        double pr[kAssetBatch];
        int hd[kAssetBatch];
#pragma unroll
        for (int j = 0; j < kAssetBatch; ++j) {
            const int i = min(i0 + j, N - 1);
            pr[j] = prow[i];
            hd[j] = HOLD(i);
        }
#pragma unroll
        for (int j = 0; j < kAssetBatch; ++j) {
            pin(pr[j]);
            pin(hd[j]);
        }
#pragma unroll
        for (int j = 0; j < kAssetBatch; ++j)
            if (i0 + j < N) s = s + fabs(pr[j]) * (double)hd[j];   // sign bit = flag
    }
    return SF(FINENV_SF_CASH) + s;
}

// Terminal summary :226-264 from current state: one lane per env.
__global__ void stock_stats_kernel(const Params p)
{
    const int E = p.cfg.n_envs, N = p.cfg.n_tickers;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const double end = end_total_asset(p, p.panel.close, E, N, e);
    const double a0 = SF(FINENV_SF_ASSET0);
    double *out = p.stats_out + (size_t)e * 6;
    out[0] = a0;
    out[1] = end;
    out[2] = end - a0;
    out[3] = SF(FINENV_SF_COST);
    out[4] = (double)SI(FINENV_SI_TRADES);
    const int n = SI(FINENV_SI_DAY) - SI(FINENV_SI_START_DAY);   // daily returns accumulated
    out[5] = sharpe_from_sums(n, SF(FINENV_SF_RET_SUM), SF(FINENV_SF_RET_SUMSQ));
}

// The same six columns for the episodes latched in the last-episode block (finenv_stock_step).
__global__ void stock_last_stats_kernel(const Params p)
{
    const int E = p.cfg.n_envs;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    double *out = p.stats_out + (size_t)e * 6;
    if (SL(FINENV_SL_COUNT) == 0.0) {
        for (int j = 0; j < 6; ++j) out[j] = __builtin_nan("");
        return;
    }
    const double a0 = SL(FINENV_SL_BEGIN_ASSET), end = SL(FINENV_SL_END_ASSET);
    out[0] = a0;
    out[1] = end;
    out[2] = end - a0;
    out[3] = SL(FINENV_SL_COST);
    out[4] = SL(FINENV_SL_TRADES);
    out[5] = sharpe_from_sums((int)SL(FINENV_SL_RET_N), SL(FINENV_SL_RET_SUM), SL(FINENV_SL_RET_SUMSQ));
}

// -------------------------------------------------------------------------------------
// Episode history (finenv_stock_set_history): asset_memory / date_memory / actions_memory of every
// env's current episode, kept on the device.  Two small kernels with their own argument struct (the
// metrics kernel is every kind's, finenv_history.hip); they ride behind the step / init / reset kernels
// as separate launches on the same stream and read the state those left in memory.  Time-major layout
// ([k][E], actions [k][E][N]): a lock-step batch writes whole contiguous rows.
// -------------------------------------------------------------------------------------
struct HistoryArgs {
    finenv_stock_history h;
    finenv_stock_state st;
    const double *close;          // panel closes [T][N]
    const uint8_t *done;          // record: this step's done [E]
    const int32_t *realised;      // record: this step's realised trades [E][N] (NULL without actions)
    const uint8_t *mask;          // arm: envs to arm, or NULL = all
    double *out;                  // (unused since the metrics kernel is finenv_history.hip's: the two stay so
    double annualization;         //  that the record kernel behind every step keeps the bytes it was timed with)
    int32_t E, N;
    uint32_t magicN;              // ceil(2^32 / N) for N >= 2
};

constexpr int kHistThreads = 256;     // envs per block of the record kernel
constexpr int kHistBatch = 16;        // dwords of `realised` each lane has in flight

// After a step.  Block b owns envs [256 b, 256 b + 256): each lane first decides for its own env whether
// entry k = len[e] is written, publishes k in LDS, then the whole block copies the block's [nenv][N]
// tile of `realised` flat (consecutive lanes = consecutive dwords of both the source and, where
// neighbouring envs share k, the destination), and each lane writes its env's two scalar columns.
// len[e] is read before the barrier and written after it by the lane that owns it.
__global__ __launch_bounds__(kHistThreads) void stock_history_record_kernel(const HistoryArgs p)
{
    __shared__ int ks[kHistThreads];
    const int E = p.E, N = p.N, cap = p.h.capacity;
    const int e0 = blockIdx.x * kHistThreads;
    const int e = e0 + (int)threadIdx.x;
    int k = 0;                                        // 0 = this env writes no entry on this step
    if (e < E) {
        const int len = p.h.len[e], fl = p.h.flags[e];
        if (!(fl & FINENV_HIST_COMPLETE) && len >= 1) {
            if (p.done[e]) p.h.flags[e] = fl | FINENV_HIST_COMPLETE;      // :222-301 appends nothing
            else if (len >= cap) p.h.flags[e] = fl | FINENV_HIST_OVERFLOW;
            else k = len;
        }
    }
    ks[threadIdx.x] = k;
    __syncthreads();
    if (p.h.actions != nullptr) {
        const int nenv = min(kHistThreads, E - e0);
        const int total = nenv * N;                   // <= 256 * 128: magicN is exact below 2^16
        const int32_t *src = p.realised + (size_t)e0 * N;
        for (int f0 = 0; f0 < total; f0 += kHistBatch * kHistThreads) {      // loads first, then stores
            int v[kHistBatch];
#pragma unroll
            for (int j = 0; j < kHistBatch; ++j) {
                const int f = f0 + j * kHistThreads + (int)threadIdx.x;
                v[j] = src[f < total ? f : total - 1];
            }
#pragma unroll
            for (int j = 0; j < kHistBatch; ++j) pin(v[j]);
#pragma unroll
            for (int j = 0; j < kHistBatch; ++j) {
                const int f = f0 + j * kHistThreads + (int)threadIdx.x;
                if (f < total) {
                    const int el = (N == 1) ? f : (int)__umulhi((unsigned)f, p.magicN);
                    const int kk = ks[el];
                    if (kk >= 1) p.h.actions[((size_t)(kk - 1) * E + e0) * N + f] = v[j];
                }
            }
        }
    }
    if (k >= 1) {
        p.h.asset[(size_t)k * E + e] = end_total_asset(p, p.close, E, N, e);
        p.h.row[(size_t)k * E + e] = SI(FINENV_SI_DAY);                    // _get_date() after :335-336
        p.h.len[e] = k + 1;
    }
}

// What __init__ (:85-97) / reset() (:359-393) leave in asset_memory / date_memory, for the envs of the
// mask: one entry.  At the start of an episode that entry is asset_memory[0] as init / reset evaluated
// it (FINENV_SF_ASSET0: the reference sums it in another order than a step does, and with
// initial == 0 it is the previous total asset); armed mid-episode, the record starts at the current
// total asset.
__global__ void stock_history_arm_kernel(const HistoryArgs p)
{
    const int E = p.E, N = p.N;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E || (p.mask != nullptr && p.mask[e] == 0)) return;
    p.h.asset[e] = SI(FINENV_SI_DAY) == SI(FINENV_SI_START_DAY) ? SF(FINENV_SF_ASSET0)
                                                                : end_total_asset(p, p.close, E, N, e);
    p.h.row[e] = SI(FINENV_SI_DAY);
    p.h.len[e] = 1;
    p.h.flags[e] = 0;
}

}  // namespace

// =====================================================================================
// Host side: handle, validation, launches.  No allocation on the device, no sync.
// =====================================================================================
struct finenv_stock : finenv_host::Handle {
    finenv_stock_config cfg;
    finenv_stock_panel panel;
    finenv_stock_state st;
    int obs_pitch;        // row pitch of the obs buffers handed to step / reset / observe (floats)
    int desync_hint;      // finenv_stock_set_desync_hint
    uint32_t magicN;
    double *last;         // finenv_stock_set_last_episode
    int32_t *win;         // finenv_stock_set_windows
    int has_hist;         // finenv_stock_set_history
    finenv_stock_history hist;
    finenv_stock_impl::StepPlan plan;     // how step() launches: plan_step()
};

namespace {

Params make_params(const finenv_stock *h)
{
    Params p;
    memset(&p, 0, sizeof(p));
    p.cfg = h->cfg;
    p.panel = h->panel;
    p.st = h->st;
    p.D = h->D;
    p.obs_pitch = h->obs_pitch;
    p.desync_hint = h->desync_hint;
    p.magicN = h->magicN;
    p.last = h->last;
    p.win = h->win;
    return p;
}

int launch_aux(finenv_stock *h, const Params &p, int mode, hipStream_t stream)
{
    if (h->cfg.n_tickers <= 32) finenv_stock_impl::launch_aux_np32(p, mode, stream);
    else if (h->cfg.n_tickers <= 64) finenv_stock_impl::launch_aux_np64(p, mode, stream);
    else finenv_stock_impl::launch_aux_np128(p, mode, stream);
    return 0;
}

// Decide how step() launches, once per change of what decides it (bind, set_windows, set_desync_hint), so that
// a step makes no HIP call but its launches.  The kernel: 33..64 tickers use the 128-wide code paths at half
// the padding (34 KB of LDS, four blocks per CU instead of two).  The round: occupancy x CUs on the device
// that owns the state block (the current one where none does, as for the launches).  A failed query leaves
// one block per CU on 256 CUs and no error behind; only a refused LDS opt-in is reported, by step().
void plan_step(finenv_stock *h)
{
    const bool win = h->win != nullptr, desync = h->desync_hint != 0;
    const int N = h->cfg.n_tickers;
    finenv_stock_impl::StepPlan &pl = h->plan;
    pl = N <= 32   ? finenv_stock_impl::choose_step_np32(h->cfg, win, desync)
         : N <= 64 ? finenv_stock_impl::choose_step_np64(h->cfg, win, desync)
                   : finenv_stock_impl::choose_step_np128(h->cfg, win, desync);
    const void *fn = reinterpret_cast<const void *>(pl.kernel);
    const finenv_host::DeviceGuard guard(h->device);
    int dev = h->device, cus = 0, per_cu = 0;
    if (dev < 0) (void)hipGetDevice(&dev);
    // > 64 KiB of dynamic LDS needs an explicit opt-in on every device that runs the kernel
    pl.lds_refused = pl.lds_bytes > 64 * 1024 &&
                     hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds_bytes) != hipSuccess;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, pl.threads, pl.lds_bytes) != hipSuccess || per_cu < 1)
        per_cu = 1;
    (void)hipGetLastError();
    pl.round = per_cu * cus;
}

// The step kernels are built for ONE resident round of blocks (every block in the same phase: traders
// loading while nobody stores yet, streamers streaming while traders compute).  Handed more blocks than
// fit at once, the hardware refills slots as blocks finish, phases mix -- traders' loads queue behind
// other blocks' stores -- and the per-env cost rises by a third (DOW30: 65,536 envs 0.64 of the
// roofline, 262,144 envs 0.47; profiles/r03_placement.md).  So a large batch is stepped as
// ceil(blocks / round) launches of equal size on the caller's stream, each one resident round or less.
void launch_step_rounds(const finenv_stock_impl::StepPlan &pl, const Params &p, hipStream_t stream)
{
    // one block of pl.threads threads per 64 envs
    const int blocks = (p.cfg.n_envs + kWave - 1) / kWave;
    const int k = (blocks + pl.round - 1) / pl.round;              // launches
    const int chunk = k > 1 ? (blocks + k - 1) / k : blocks;
    Params q = p;
    int b = 0;
    do {
        q.block_base = b;
        const int nb = blocks - b < chunk ? blocks - b : chunk;
        hipLaunchKernelGGL(pl.kernel, dim3((unsigned)nb), dim3((unsigned)pl.threads), pl.lds_bytes, stream, q);
        b += chunk;
    } while (b < blocks);
}

HistoryArgs make_history_args(const finenv_stock *h)
{
    HistoryArgs a;
    memset(&a, 0, sizeof(a));
    a.h = h->hist;
    a.st = h->st;
    a.close = h->panel.close;
    a.E = h->cfg.n_envs;
    a.N = h->cfg.n_tickers;
    a.magicN = h->magicN;
    return a;
}

// init / reset (re)start episodes: the reference's __init__ / reset() start the memories afresh
void launch_history_arm(const finenv_stock *h, const uint8_t *mask, hipStream_t stream)
{
    HistoryArgs a = make_history_args(h);
    a.mask = mask;
    hipLaunchKernelGGL(stock_history_arm_kernel, dim3((a.E + 255) / 256), dim3(256), 0, stream, a);
}

// the metrics' series: asset_memory and its pct_change()
finenv_host::HistorySeries history_series(const finenv_stock *h)
{
    return {h->hist.asset, nullptr, nullptr, h->hist.len, h->hist.flags, 0, h->hist.capacity, h->cfg.n_envs};
}

}  // namespace

#ifdef FINENV_DIAG
unsigned long long *g_finenv_dbg = nullptr;      // shared with the other kernels' diagnostic builds
#define g_dbg g_finenv_dbg
extern "C" void finenv_diag_set_stamp_buffer(void *ptr) { g_finenv_dbg = (unsigned long long *)ptr; }
#endif

extern "C" {

int finenv_abi_version(void) { return FINENV_ABI_VERSION; }

int finenv_struct_size(int which)
{
    switch (which) {
    case 0: return (int)sizeof(finenv_stock_config);
    case 1: return (int)sizeof(finenv_stock_panel);
    case 2: return (int)sizeof(finenv_stock_state);
    case 3: return (int)sizeof(finenv_portfolio_config);
    case 4: return (int)sizeof(finenv_portfolio_panel);
    case 5: return (int)sizeof(finenv_portfolio_state);
    case 6: return (int)sizeof(finenv_crypto_config);
    case 7: return (int)sizeof(finenv_crypto_panel);
    case 8: return (int)sizeof(finenv_crypto_state);
    case 9: return (int)sizeof(finenv_stocknp_config);
    case 10: return (int)sizeof(finenv_stocknp_panel);
    case 11: return (int)sizeof(finenv_stocknp_state);
    case 12: return (int)sizeof(finenv_cashpenalty_config);
    case 13: return (int)sizeof(finenv_cashpenalty_panel);
    case 14: return (int)sizeof(finenv_cashpenalty_state);
    case 15: return (int)sizeof(finenv_stoploss_config);
    case 16: return (int)sizeof(finenv_stoploss_panel);
    case 17: return (int)sizeof(finenv_stoploss_state);
    // (18 stays invalid: the end of the first v3 list, include/finenv.h)
    case 19: return (int)sizeof(finenv_btc_config);
    case 20: return (int)sizeof(finenv_btc_panel);
    case 21: return (int)sizeof(finenv_btc_state);
    // (22 stays invalid: bindings of the list that ended at 21 probe it as its end)
    case 23: return (int)sizeof(finenv_replay_view);
    case 24: return (int)sizeof(finenv_replay_batch);
    // (25 stays invalid: bindings of the list that ended at 24 probe it as its end)
    case 26: return (int)sizeof(finenv_replay_nstep);
    // (27 stays invalid: bindings of the list that ended at 26 probe it as its end)
    case 28: return (int)sizeof(finenv_replay_per);
    // (29 stays invalid: bindings of the list that ended at 28 probe it as its end)
    case 30: return (int)sizeof(finenv_rollout_view);
    case 31: return (int)sizeof(finenv_rollout_batch);
    // (32 stays invalid: bindings of the list that ended at 31 probe it as its end)
    case 33: return (int)sizeof(finenv_vecnorm);
    default: return FINENV_ERR_INVALID;
    }
}

const char *finenv_strerror(int code)
{
    switch (code) {
    case FINENV_OK: return "ok";
    case FINENV_ERR_INVALID: return "invalid argument";
    case FINENV_ERR_UNBOUND: return "panel/state not bound";
    case FINENV_ERR_HIP: return "HIP runtime error";
    case FINENV_ERR_NOMEM: return "out of host memory";
    default: return "unknown error";
    }
}

int finenv_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return FINENV_ERR_HIP;
    }
    return n;
}

int finenv_stock_create(const finenv_stock_config *cfg, finenv_stock **out)
{
    if (!cfg || !out) return FINENV_ERR_INVALID;
    *out = nullptr;
    if (cfg->n_envs < 1 || cfg->n_tickers < 1 || cfg->n_tickers > FINENV_STOCK_MAX_TICKERS ||
        cfg->n_tech < 0 || cfg->n_days < 1 || cfg->hmax < 0 ||
        cfg->hmax > (cfg->n_tickers <= 32 ? (1 << 24) : (1 << 22)))
        return FINENV_ERR_INVALID;
    if (cfg->single_ticker && cfg->n_tickers != 1) return FINENV_ERR_INVALID;
    if ((long long)cfg->n_envs * (1 + 2 * cfg->n_tickers + cfg->n_tech * cfg->n_tickers) >
        (1ll << 40))
        return FINENV_ERR_INVALID;
    {   // every device offset is a 32-bit byte offset from a uniform base (see at())
        const long long E = cfg->n_envs, N = cfg->n_tickers, T = cfg->n_days;
        const long long D = 1 + 2 * N + (long long)cfg->n_tech * N;
        const long long lim = (1ll << 32) - 1;
        if ((FINENV_STOCK_I32_FIELDS + 2 * N) * E * 4 > lim || FINENV_STOCK_F64_FIELDS * E * 8 > lim ||
            T * D * 4 > lim || T * N * 8 > lim || E * N * 4 > lim)
            return FINENV_ERR_INVALID;
    }
    finenv_stock *h = finenv_host::new_handle<finenv_stock>(
        cfg, 1 + 2 * cfg->n_tickers + cfg->n_tech * cfg->n_tickers);
    if (!h) return FINENV_ERR_NOMEM;
    h->obs_pitch = h->D;
    h->magicN = finenv_host::magic_for(cfg->n_tickers);
    *out = h;
    return FINENV_OK;
}

void finenv_stock_destroy(finenv_stock *h) { delete h; }

const char *finenv_stock_last_error(const finenv_stock *h) { return finenv_host::last_error(h); }

int finenv_stock_obs_dim(const finenv_stock *h) { return finenv_host::obs_dim(h); }

int finenv_stock_set_desync_hint(finenv_stock *h, int32_t on)
{
    if (!h) return FINENV_ERR_INVALID;
    const int was = h->desync_hint;
    h->desync_hint = on != 0;
    if (h->bound && was != h->desync_hint) plan_step(h);
    return FINENV_OK;
}

int finenv_stock_set_obs_pitch(finenv_stock *h, int32_t pitch)
{
    if (!h) return FINENV_ERR_INVALID;
    if (pitch == 0) pitch = h->D;
    if (pitch < h->D || (long long)pitch * 64 * 4 > (1ll << 32) - 1)
        return finenv_host::fail(h, FINENV_ERR_INVALID, "set_obs_pitch: pitch must be >= obs_dim");
    h->obs_pitch = pitch;
    return FINENV_OK;
}

int finenv_stock_bind(finenv_stock *h, const finenv_stock_panel *panel,
                      const finenv_stock_state *st)
{
    if (!h || !panel || !st) return FINENV_ERR_INVALID;
    if (!panel->close || !panel->obs_tmpl ||
        (h->cfg.use_turbulence && !panel->risk))
        return finenv_host::fail(h, FINENV_ERR_INVALID, "bind: null panel pointer");
    if (!st->f64 || !st->i32)
        return finenv_host::fail(h, FINENV_ERR_INVALID, "bind: null state pointer");
    finenv_host::bind(h, panel, st);
    plan_step(h);
    return FINENV_OK;
}

int finenv_stock_init(finenv_stock *h, int32_t day0, void *stream)
{
    if (const int rc = finenv_host::ready(h, "init")) return rc;
    const finenv_host::DeviceGuard guard(h->device);
    if (day0 < 0 || day0 >= h->cfg.n_days)
        return finenv_host::fail(h, FINENV_ERR_INVALID, "init: bad day0");
    Params p = make_params(h);
    p.day0 = day0;
    launch_aux(h, p, 0, (hipStream_t)stream);
    if (h->has_hist) launch_history_arm(h, nullptr, (hipStream_t)stream);
    return finenv_host::check_launch(h, "stock_init");
}

int finenv_stock_reset(finenv_stock *h, const uint8_t *mask, float *obs_out, void *stream)
{
    if (const int rc = finenv_host::ready(h, "reset")) return rc;
    const finenv_host::DeviceGuard guard(h->device);
    Params p = make_params(h);
    p.mask = mask;
    p.obs = obs_out;
    launch_aux(h, p, 1, (hipStream_t)stream);
    if (h->has_hist) launch_history_arm(h, mask, (hipStream_t)stream);
    return finenv_host::check_launch(h, "stock_reset");
}

int finenv_stock_observe(finenv_stock *h, float *obs_out, void *stream)
{
    if (!h || !obs_out) return FINENV_ERR_INVALID;
    if (const int rc = finenv_host::ready(h, "observe")) return rc;
    const finenv_host::DeviceGuard guard(h->device);
    Params p = make_params(h);
    p.obs = obs_out;
    launch_aux(h, p, 2, (hipStream_t)stream);
    return finenv_host::check_launch(h, "stock_observe");
}

int finenv_stock_refresh(finenv_stock *h, void *stream)
{
    if (const int rc = finenv_host::ready(h, "refresh")) return rc;
    const finenv_host::DeviceGuard guard(h->device);
    Params p = make_params(h);
    launch_aux(h, p, 3, (hipStream_t)stream);
    return finenv_host::check_launch(h, "stock_refresh");
}

int finenv_stock_step(finenv_stock *h, const float *actions, float *obs, float *reward,
                      uint8_t *done, float *term_obs, int32_t *realised, int32_t auto_reset,
                      void *stream)
{
    if (const int rc = finenv_host::ready(h, "step")) return rc;
    const finenv_host::DeviceGuard guard(h->device);
    if (!actions || !obs || !reward || !done)
        return finenv_host::fail(h, FINENV_ERR_INVALID, "step: null actions/obs/reward/done");
    if (h->has_hist && h->hist.actions && !realised)
        return finenv_host::fail(h, FINENV_ERR_INVALID,
                                 "step: the attached history records actions and needs `realised`");
    Params p = make_params(h);
    p.actions = actions;
    p.obs = obs;
    p.reward = reward;
    p.done = done;
    p.term_obs = term_obs;
    p.realised = realised;
    p.auto_reset = auto_reset;
#ifdef FINENV_DIAG
    {
        const char *d = getenv("FINENV_DIAG");
        p.diag = d ? atoi(d) : 0;
        p.dbg = g_dbg;
    }
#endif
    const hipStream_t s = (hipStream_t)stream;
    if (h->plan.lds_refused) return finenv_host::fail(h, FINENV_ERR_HIP, "step: cannot raise the dynamic LDS limit");
    launch_step_rounds(h->plan, p, s);
    if (h->has_hist) {      // behind the step kernel (its last round): reads done, realised and the new state
        HistoryArgs a = make_history_args(h);
        a.done = done;
        a.realised = realised;
        hipLaunchKernelGGL(stock_history_record_kernel, dim3((a.E + kHistThreads - 1) / kHistThreads),
                           dim3(kHistThreads), 0, s, a);
    }
    return finenv_host::check_launch(h, "stock_step");
}

int finenv_stock_episode_stats(finenv_stock *h, double *out, void *stream)
{
    if (!h || !out) return FINENV_ERR_INVALID;
    if (const int rc = finenv_host::ready(h, "episode_stats")) return rc;
    const finenv_host::DeviceGuard guard(h->device);
    Params p = make_params(h);
    p.stats_out = out;
    const int E = h->cfg.n_envs;
    hipLaunchKernelGGL(stock_stats_kernel, dim3((E + 255) / 256), dim3(256), 0,
                       (hipStream_t)stream, p);
    return finenv_host::check_launch(h, "stock_episode_stats");
}

int finenv_stock_set_last_episode(finenv_stock *h, double *last)
{
    if (!h) return FINENV_ERR_INVALID;
    h->last = last;
    return FINENV_OK;
}

int finenv_stock_set_windows(finenv_stock *h, int32_t *win)
{
    if (!h) return FINENV_ERR_INVALID;
    const bool was = h->win != nullptr;
    h->win = win;
    if (h->bound && was != (win != nullptr)) plan_step(h);
    return FINENV_OK;
}

int finenv_stock_last_episode_stats(finenv_stock *h, double *out, void *stream)
{
    if (!h || !out) return FINENV_ERR_INVALID;
    if (const int rc = finenv_host::ready_last_episode(h, "last_episode_stats")) return rc;
    const finenv_host::DeviceGuard guard(h->device);
    Params p = make_params(h);
    p.stats_out = out;
    const int E = h->cfg.n_envs;
    hipLaunchKernelGGL(stock_last_stats_kernel, dim3((E + 255) / 256), dim3(256), 0,
                       (hipStream_t)stream, p);
    return finenv_host::check_launch(h, "stock_last_episode_stats");
}

int finenv_stock_set_history(finenv_stock *h, const finenv_stock_history *hist)
{
    if (!h) return FINENV_ERR_INVALID;
    const bool missing = hist && (!hist->asset || !hist->row || !hist->len || !hist->flags);
    return finenv_host::set_history(h, h->hist, h->has_hist, hist,
                                    missing ? "set_history: null asset/row/len/flags" : nullptr);
}

int finenv_stock_history_arm(finenv_stock *h, const uint8_t *mask, void *stream)
{
    return finenv_host::history_arm(h, mask, stream, "stock_history_arm", launch_history_arm);
}

int finenv_stock_history_metrics(finenv_stock *h, double annualization, double *out, void *stream)
{
    return finenv_host::history_metrics(h, annualization, out, stream, "stock_history_metrics", history_series);
}

}  // extern "C"
